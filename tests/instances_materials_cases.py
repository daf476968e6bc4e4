"""The cases of the instanced full-shading tests (tests/test_instances_materials_host.py, tests/test_gpu_instances_materials.py): two BLASes
with their per-triangle shading data, ONE material and texture list, instances, cameras and lights.  Chosen with the restatement
(tests/instances_materials_ref.py) alone, on the CPU; what each must exercise is asserted on the restatement's diagnostics, with and without
a GPU.  Everything is seeded and float32; nothing here touches a device."""
from __future__ import annotations

import functools
import math

import numpy as np

from snail_amd import FPSCamera, scenes
from snail_amd.camera import _rotate
from tests import dbvh_ref as R
from tests import instances_materials_ref as IM
from tests import materials_cases as MK
from tests import materials_ref as M
from tests import oracle_lib as O

F = np.float32

# ONE scene-wide list.  4 is the UBER material that both BLASes' maps name.
DESCS = [("simple", (0.3, 0.8, 0.6), False), ("tex", 0, True), ("tex", 1, False), ("uber", (0.9, 0.4, 0.1), (0.2, 0.6, 1.0), 0.0), ("uber", (0.2, 0.7, 0.5), (1.0, 0.3, 0.1), 1.0)]
SHEET_MAP = [-1, 0, 1, 2, 3, 4]     # the sheet's classes 0 .. 5
BOX_MAP = [4, -1, 1]                # the box's classes 0 .. 2
TEXTURES = lambda: [MK.checker_texture(64, 64, 3), MK.checker_texture(32, 8, 4)]      # noqa: E731  (the second is not square)
BACK = (-3.0, 2.0, -2.4, 2.8, 1.5)  # the sheet BLAS's backdrop: x0, x1, y0, y1, z


def sheet_tris(nu=12, nv=10, seed=5):
    """A materials_cases.patch_scene-like BLAS with the class of every triangle given directly: a bumpy sheet of nu x nv quads whose classes
    form horizontal bands on its left two thirds and 2 x 2 patches on the rest, a backdrop of two LARGE triangles (class 5: the shared UBER
    material) that shows around it, and a slab floating before the sheet that throws shadows on it.  -> (tri_verts [n, 3, 3], class [n])"""
    rng = np.random.RandomState(seed)
    x0, x1, y0, y1 = -2.6, 1.0, -1.0, 2.2
    us, vs = np.meshgrid(np.arange(nu + 1), np.arange(nv + 1), indexing="ij")
    x = x0 + us * ((x1 - x0) / nu); y = y0 + vs * ((y1 - y0) / nv)
    z = 0.25 * np.sin(x * 1.7) * np.cos(y * 2.3) + 0.04 * rng.rand(nu + 1, nv + 1)
    p = (np.round(np.stack([x, y, z], axis=-1) * 1024.0) / 1024.0).astype(np.float32)
    tris, cls = [], []
    pc = rng.randint(0, 6, size=(nu // 2 + 1, nv // 2 + 1))
    band = rng.permutation(np.arange(nv // 2 + 1) % 5)
    nb = int(nu * 0.65)
    for i in range(nu):
        for j in range(nv):
            if i >= nb and (i // 3 + j // 2) % 7 == 6 and (i % 3 == 1):      # holes in the patched part: the backdrop shows through
                continue
            a, b, c, d = p[i, j], p[i + 1, j], p[i + 1, j + 1], p[i, j + 1]
            tris += [(a, b, c), (a, c, d)]
            cls += [band[j // 2] if i < nb else pc[i // 2, j // 2]] * 2
    bx0, bx1, by0, by1, bz = BACK
    big = [np.array(v, dtype=np.float32) for v in ((bx0, by0, bz), (bx1, by0, bz), (bx1, by1, bz), (bx0, by1, bz))]
    tris += [(big[0], big[2], big[1]), (big[0], big[3], big[2])]
    cls += [5, 5]
    sl = [np.array(v, dtype=np.float32) for v in ((-0.1, 0.3, -1.0), (0.7, 0.3, -1.0), (0.7, 1.0, -1.0), (-0.1, 1.0, -1.0))]
    tris += [(sl[0], sl[1], sl[2]), (sl[0], sl[2], sl[3])]
    cls += [3, 4]
    return np.ascontiguousarray(np.array(tris, dtype=np.float32)), np.array(cls, dtype=np.int32)


def box_tris():
    """scenes.box_scene() at half its size: [-0.5, 0.5]^3"""
    return np.ascontiguousarray((scenes.box_scene().astype(np.float32).reshape(-1, 3, 3) * F(0.5)).astype(np.float32))


def box_data(osc, tv, seed):
    """flat records: the flag set, the three normals still different (the OUTWARD plane normal bent a little), classes by input index"""
    uv, nrm, _ = MK.vertex_data(osc, tv.reshape(-1, 9), seed, uv_scales=(3.0, 0.4))
    plane = np.zeros((len(tv), 3), dtype=np.float32)
    plane[osc.perm] = osc.tris["plane"][:, :3]
    rng = np.random.RandomState(seed + 1)
    nrm = (-plane[:, None, :] + (rng.rand(len(tv), 3, 3) - 0.5) * 0.5).astype(np.float32)
    cls = np.array([2, 0, 1, 0, 2, 0, 0, 1, 0, 0, 2, 0], dtype=np.int32)[:len(tv)]
    return uv, nrm, cls, np.ones(len(tv), dtype=bool)


def rot_axis(axis, radians):
    return np.array(_rotate(axis, radians), dtype=np.float32)


def general_rotation():
    """a rotation with nine non-zero entries"""
    r = (rot_axis((0, 1, 0), 0.5).astype(np.float64) @ rot_axis((1, 0, 0), 0.35).astype(np.float64) @ rot_axis((0, 0, 1), -0.4).astype(np.float64)).astype(np.float32)
    assert (r != 0).all()
    return r


ROT90Y = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], dtype=np.float32)       # exact
ROT180Z = np.array([[-1, 0, 0], [0, -1, 0], [0, 0, 1]], dtype=np.float32)     # exact


def main_instances():
    """(rot [n, 3, 3], tr [n, 3], blas index [n]); BLAS 0 = the sheet, 1 = the box.
      0  sheet, the identity
      1  sheet, turned by 180 degrees about z and moved so that its backdrop abuts instance 0's along x = BACK.x1: the rows of pixels across
         the seam see the SAME triId of the same BLAS in two slots
      2  box, an exact quarter turn about y, standing on instance 0's backdrop (touching it) below the sheet: rows across its silhouette see
         the box's shared UBER material beside the backdrop's
      3  box, a general rotation, floating before the sheet (it throws shadows)
      4  sheet, a general rotation, below and before the others
      5  box, the identity, close to the camera: its front face's triangles fill whole blocks (one of them textured)"""
    g = general_rotation()
    rot = np.stack([np.eye(3, dtype=np.float32), ROT180Z, ROT90Y, g, g, np.eye(3, dtype=np.float32)])
    tr = np.array([[0, 0, 0], [2 * BACK[1], 0.4, 0], [-0.4, -1.75, BACK[4] - 0.5], [-1.6, 1.1, -1.3], [4.0, -4.3, 0.6], [2.0, 1.0, -2.6]], dtype=np.float32)
    return rot, tr, np.array([0, 0, 1, 1, 0, 1], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def blas_data():
    """-> [(tv, oracle scene, (uv, nrm, mat_index, flat, material_map))] of the sheet and the box"""
    stv, scls = sheet_tris()
    sosc = O.OracleScene(stv.reshape(-1, 9))
    suv, snrm, sflat = MK.vertex_data(sosc, stv.reshape(-1, 9), 22)
    btv = box_tris()
    bosc = O.OracleScene(btv.reshape(-1, 9))
    buv, bnrm, bcls, bflat = box_data(bosc, btv, 31)
    return [(stv.reshape(-1, 9), sosc, (suv, snrm, scls, sflat, SHEET_MAP)), (btv.reshape(-1, 9), bosc, (buv, bnrm, bcls, bflat, BOX_MAP))]


def degenerate_data():
    """every map entry -1 and every record flat with the triangle's plane normal: full shading must coincide with simple shading"""
    out = []
    for tv, osc, _ in blas_data():
        n = len(tv)
        out.append((np.zeros((n, 3, 2), dtype=np.float32), MK.plane_normals(osc), np.zeros(n, dtype=np.int32), np.ones(n, dtype=bool), [-1]))
    return out


def cpu_ref(oscs, rot, tr, bi):
    """The restatement's scene, its tree from the restated builder (equal to snail_instances_build's: tests/test_instances_host.py)"""
    xf = np.concatenate([np.asarray(rot, dtype=np.float32).reshape(-1, 9), np.asarray(tr, dtype=np.float32).reshape(-1, 3)], axis=1)
    bb = np.stack([np.concatenate([o.nodes[0]["bmin"], o.nodes[0]["bmax"]]) for o in oscs]).astype(np.float32)
    nodes, _depth, perm = R.build(xf, bi, bb)
    return R.Ref(list(oscs), nodes, xf[perm], np.asarray(bi)[perm])


def updated_instances():
    """new rotations for every instance and one changed BLAS index (instance 5: the box becomes a sheet)"""
    rot, tr, bi = main_instances()
    turn = rot_axis((0, 1, 0), 0.2)
    rot2 = np.stack([(turn.astype(np.float64) @ r.astype(np.float64)).astype(np.float32) for r in rot])
    bi2 = bi.copy(); bi2[5] = 0
    tr2 = tr.copy(); tr2[5] = (4.2, 0.6, 2.5)
    return rot2, tr2, bi2


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(tvs, oscs, per_blas, rot, tr, bi, ref (restatement scene), cam (resx -> camera), lights)"""
    data = blas_data()
    tvs = [d[0] for d in data]
    oscs = [d[1] for d in data]
    per_blas = [d[2] for d in data]
    if name in ("main", "degenerate", "updated"):
        rot, tr, bi = updated_instances() if name == "updated" else main_instances()
        if name == "degenerate":
            per_blas = degenerate_data()
        cam96 = FPSCamera(np.array([1.1, 0.1, -4.6], dtype=np.float32), 0.0, 0.0).camera()
        cam70 = FPSCamera(np.array([0.6, -0.3, -3.6], dtype=np.float32), 0.08, 0.05).camera()
        # before the sheets, above the slab; the second light's radius lets the packet-level cull remove it for some packets
        lights = np.array([[-0.6, 1.6, -3.0, 1.0, 0.9, 0.8, 16.0], [1.9, -1.0, -0.9, 0.4, 0.6, 1.0, 2.2]], dtype=np.float32)
        cams = {96: cam96, 70: cam70, 64: cam96}
    elif name == "quirk":
        # ONE sheet instance (slot 0) seen past the edge of its triangle 0 from close by, background beside it
        rot, tr, bi = np.eye(3, dtype=np.float32)[None], np.zeros((1, 3), dtype=np.float32), np.zeros(1, dtype=np.int32)
        tvs, oscs, per_blas = tvs[:1], oscs[:1], per_blas[:1]
        cam = quirk_camera(oscs[0])
        lights = np.array([[-0.6, 1.6, -3.0, 1.0, 0.9, 0.8, 16.0]], dtype=np.float32)
        cams = {48: cam}
    elif name == "deep":
        # a DEEP BLAS (scenes.chain, depth 63) in two instances under one light: the DEEP shadow walk on full shading's samples
        tv = scenes.chain()
        osc = O.OracleScene(tv)
        uv, nrm, flat = MK.vertex_data(osc, tv, 23)
        tvs, oscs, per_blas = [tv], [osc], [(uv, nrm, np.arange(len(tv), dtype=np.int32) % 6, flat, SHEET_MAP)]
        ext = (osc.nodes[0]["bmax"] - osc.nodes[0]["bmin"]).astype(np.float32)
        rot = np.stack([np.eye(3, dtype=np.float32), general_rotation()])
        tr = np.array([[0, 0, 0], [0.2 * ext[0], 0.0, 0.3 * ext[2]]], dtype=np.float32)
        bi = np.zeros(2, dtype=np.int32)
        cams = {64: FPSCamera(np.array([-0.25, 0.004, 0.002], dtype=np.float32), -math.pi / 2, 0.0).camera()}
        lights = MK.centre_lights(osc, [(0.3, 0.9, 0.8, (1.0, 0.9, 0.8), 2.0)])
    else:
        raise KeyError(name)
    return dict(tvs=tvs, oscs=oscs, per_blas=per_blas, rot=rot, tr=tr, bi=bi, ref=cpu_ref(oscs, rot, tr, bi), cams=cams, lights=lights)


def quirk_camera(osc):
    """materials_cases.quirk_camera for a triangle 0 that need not face the camera's side: from a point on the normal through a point just
    outside an edge, looking back at it, so that in some quad lane 0 misses and another lane hits triangle 0"""
    t = osc.tris[0]
    a = t["a"].astype(np.float64); ba = t["ba"].astype(np.float64); ca = t["ca"].astype(np.float64)
    nrm = t["plane"][:3].astype(np.float64)
    target = a + 0.5 * ba - 0.02 * ca
    size = max(np.linalg.norm(ba), np.linalg.norm(ca))
    pos = target - nrm / np.linalg.norm(nrm) * size * 2.5
    dirv = target - pos
    ang = math.atan2(dirv[0], dirv[2])
    pitch = -math.atan2(dirv[1], math.hypot(dirv[0], dirv[2]))
    return FPSCamera(pos.astype(np.float32), ang, pitch).camera()


def ref_textures():
    return [M.RefTexture(t) for t in TEXTURES()]


def reference(name, transform=True):
    c = case(name)
    return IM.InstMaterialsRef(c["ref"], c["per_blas"], MK.ref_materials(DESCS), ref_textures(), transform=transform)
