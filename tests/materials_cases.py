"""The cases of the full-shading tests (tests/test_gpu_materials.py): scenes, per-triangle shading data, materials, textures, cameras and
lights.  Chosen with the restatement (tests/materials_ref.py) alone, on the CPU; what each must exercise is asserted by the GPU tests on the
restatement's diagnostics and, for the cameras picked here, by tests/test_materials_host.py without a GPU.  Everything is seeded and
float32; nothing here touches the product library."""
from __future__ import annotations

import functools
import math

import numpy as np

from snail_amd import FPSCamera, scenes
from tests import materials_ref as M
from tests import oracle_lib as O

F = np.float32


def checker_texture(w, h, seed):
    """uint8 [h, w, 3]: a seeded noise over a coarse checker, so that neighbouring texels and neighbouring mip levels all differ"""
    rng = np.random.RandomState(seed)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    base = (((xs // max(w // 8, 1)) + (ys // max(h // 4, 1))) & 1) * 120 + 40
    return np.clip(base[..., None] + rng.randint(-40, 90, size=(h, w, 3)), 0, 255).astype(np.uint8)


def vertex_data(osc, tv, seed, uv_scales=(3.0,)):
    """Per INPUT triangle: uv [n,3,2] in [-3, 3] (the triangle's span scaled by uv_scales[i % len]), per-vertex normals [n,3,3] = the plane
    normal bent by up to ~25 degrees (not normalised again), flat flags for a third of the triangles (whose three normals still differ, so
    that a path that ignores or honours the flag wrongly shows).  Triangles of scale 3 take the corners (-3,-3), (3,3), (-3,3)."""
    n = len(tv)
    rng = np.random.RandomState(seed)
    plane = np.zeros((n, 3), dtype=np.float32)
    plane[osc.perm] = osc.tris["plane"][:, :3]
    plane[~np.isfinite(plane).all(axis=1)] = (0.0, 1.0, 0.0)      # (a sliver's plane may not be finite; the shading data must be)
    sc = np.array([uv_scales[i % len(uv_scales)] for i in range(n)], dtype=np.float64)
    centre = (rng.rand(n, 1, 2) * 2.0 - 1.0) * (3.0 - sc)[:, None, None]
    uv = (centre + (rng.rand(n, 3, 2) * 2.0 - 1.0) * sc[:, None, None]).astype(np.float32)
    corners = np.array([[-3.0, -3.0], [3.0, 3.0], [-3.0, 3.0]], dtype=np.float32)
    for i in np.flatnonzero(sc >= 3.0):      # the full span, both coordinates along one edge: the steepest steps per quad (the last mip levels)
        uv[i] = corners[rng.permutation(3)] * (1.0 if rng.rand() < 0.5 else -1.0)
    nrm = (plane[:, None, :] + (rng.rand(n, 3, 3) - 0.5) * 0.9).astype(np.float32)
    flat = (np.arange(n) % 3) == 1
    return uv, nrm, flat


def plane_normals(osc):
    """nrm [n,3,3] of the INPUT triangles = their plane normal at all three vertices (the degenerate case: with every triangle flat and every
    material the default, full shading must coincide with simple shading)"""
    n = len(osc.tris)
    plane = np.zeros((n, 3), dtype=np.float32)
    plane[osc.perm] = osc.tris["plane"][:, :3]
    return np.repeat(plane[:, None, :], 3, axis=1).copy()


def centre_lights(osc, spec):
    """lights7 from (fx, fy, fz, colour, radius factor): positions as fractions of the scene's box, radius in units of its largest extent"""
    lo, hi = osc.nodes[0]["bmin"], osc.nodes[0]["bmax"]
    ext = float((hi - lo).max())
    out = []
    for fx, fy, fz, col, rf in spec:
        p = lo + (hi - lo) * np.array([fx, fy, fz], dtype=np.float32)
        out.append([p[0], p[1], p[2], col[0], col[1], col[2], rf * ext])
    return np.array(out, dtype=np.float32)


TEXTURES = lambda: [checker_texture(64, 64, 3), checker_texture(32, 8, 4)]      # noqa: E731


def materials_large():
    """the large-triangle case: TEX over 64 x 64 and over 32 x 8 (one with, one without N.R), a SIMPLE colour, the default"""
    return [("tex", 0, True), ("tex", 1, False), ("simple", (0.9, 0.5, 0.2), True)], [0, 1, -1, 2]


def materials_mod5():
    """by input index mod 5: default, SIMPLE without N.R, TEX, UBER dissolve 0, UBER dissolve 1"""
    return [("simple", (0.3, 0.8, 0.6), False), ("tex", 0, True), ("uber", (0.9, 0.4, 0.1), (0.2, 0.6, 1.0), 0.0), ("uber", (0.2, 0.7, 0.5), (1.0, 0.3, 0.1), 1.0)], [-1, 0, 1, 2, 3]


def ref_materials(descs):
    out = []
    for d in descs:
        if d[0] == "simple":
            out.append(M.RefMaterial(M.SIMPLE, d[2], d[1]))
        elif d[0] == "tex":
            out.append(M.RefMaterial(M.TEX, d[2], texture=d[1]))
        else:
            out.append(M.RefMaterial(M.UBER, True, d[1], d[2], d[3]))
    return out


def small_scene():
    """a few thousand small triangles: scenes.offgrid's blob (the degenerate case and the quirk)"""
    return scenes.offgrid(n_blob=3000)


def patch_scene(nu=18, nv=14, patch=2, seed=5, flip=True, x0=-2.6, x1=1.0, y0=-1.0, y1=2.2, bands=0.65):
    """The small-triangle case.  A bumpy sheet of nu x nv quads (triangles of a few pixels at 96 x 64) in front of a backdrop of two large
    triangles that shows beside it, and a slab floating before the sheet that throws shadows on it.  Materials go by INPUT INDEX mod 5, so
    the triangles are ORDERED to put the wanted class at every index: on the sheet's left two thirds the classes form horizontal bands two
    quads high (a pixel row inside a band: several triangles, one material), on the rest patches of `patch` x `patch` quads (several materials in
    most blocks, the default among them).  -> tri_verts [n,3,3]"""
    rng = np.random.RandomState(seed)
    us, vs = np.meshgrid(np.arange(nu + 1), np.arange(nv + 1), indexing="ij")
    x = x0 + us * ((x1 - x0) / nu); y = y0 + vs * ((y1 - y0) / nv)
    z = 0.25 * np.sin(x * 1.7) * np.cos(y * 2.3) + 0.04 * rng.rand(nu + 1, nv + 1)
    p = (np.round(np.stack([x, y, z], axis=-1) * 1024.0) / 1024.0).astype(np.float32)
    tris, cls = [], []
    pc = rng.randint(0, 5, size=(nu // patch + 1, nv // patch + 1))
    band = rng.permutation(np.arange(nv // 2 + 1) % 5)
    nb = int(nu * bands)
    for i in range(nu):
        for j in range(nv):
            if i >= nb and (i // 3 + j // 2) % 7 == 6 and (i % 3 == 1):      # holes in the patched part: the backdrop shows through
                continue
            a, b, c, d = p[i, j], p[i + 1, j], p[i + 1, j + 1], p[i, j + 1]
            tris += [(a, b, c), (a, c, d)] if flip else [(a, c, b), (a, d, c)]
            cls += [band[j // 2] if i < nb else pc[i // patch, j // patch]] * 2
    big = [np.array(v, dtype=np.float32) for v in ((-9.0, -6.0, 3.0), (9.0, -6.0, 3.0), (9.0, 6.0, 3.0), (-9.0, 6.0, 3.0))]
    tris += [(big[0], big[2], big[1]), (big[0], big[3], big[2])]
    cls += [2, 0]
    sl = [np.array(v, dtype=np.float32) for v in ((-0.1, 0.3, -1.0), (0.7, 0.3, -1.0), (0.7, 1.0, -1.0), (-0.1, 1.0, -1.0))]
    tris += [(sl[0], sl[1], sl[2]), (sl[0], sl[2], sl[3])]
    cls += [3, 4]
    # classes with fewer triangles than the largest are filled up with small triangles far outside the view, so that EVERY triangle sits at an
    # index of its class: input index 5 j + k <- the j-th triangle of class k
    buckets = [[t for t, k in zip(tris, cls) if k == c] for c in range(5)]
    m = max(len(b) for b in buckets)
    for c in range(5):
        for f in range(m - len(buckets[c])):
            o = np.array([40.0 + 0.5 * f, 30.0 + c, 5.0], dtype=np.float32)
            buckets[c].append((o, o + np.array([0.25, 0.0, 0.0], dtype=np.float32), o + np.array([0.0, 0.25, 0.0], dtype=np.float32)))
    return np.ascontiguousarray(np.array([buckets[k][j] for j in range(m) for k in range(5)], dtype=np.float32))


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(tv, osc, uv, nrm, mat_index, flat, descs, material_map, textures (level-0 arrays), cam, cam70, lights); cam is the camera of the
    96 x 64 frame, cam70 that of the 70 x 50 one"""
    if name in ("large", "degenerate_box"):
        tv = scenes.box_scene()
        osc = O.OracleScene(tv)
        # inside the box, near one corner, looking along the walls: the far wall's triangles fill whole blocks, the side walls run off at
        # grazing angles (large texture-coordinate steps per quad: the last mip levels), the small-uv triangles give level 0
        # (found by a seeded search over cameras close to a wall, with the restatement's diagnostics as the criterion)
        cam = FPSCamera(np.array([0.07409662753343582, -0.38917264342308044, -0.9855359196662903], dtype=np.float32), 5.381215413471316, -0.5624271423966315).camera()
        # one light inside the box, one outside it (the box's normals point inwards: only a light behind a wall lights its inner face)
        lights = centre_lights(osc, [(0.45, 0.6, 0.55, (1.0, 0.9, 0.8), 1.4), (0.7, 1.8, 0.4, (0.3, 0.5, 1.0), 2.5)])
        uv, nrm, flat = vertex_data(osc, tv, 21, uv_scales=(3.0, 0.02, 3.0, 0.4))
        descs, mmap = materials_large()
        mat_index = np.arange(len(tv), dtype=np.int32) % len(mmap)
    elif name == "small":
        tv = patch_scene()
        osc = O.OracleScene(tv)
        cam = FPSCamera(np.array([0.0, 0.0, -3.2], dtype=np.float32), 0.0, 0.0).camera()
        # before the sheet, above the slab; the second light's radius lets the packet-level cull remove it for some packets
        lights = np.array([[-0.6, 1.6, -2.6, 1.0, 0.9, 0.8, 14.0], [1.6, -1.2, -0.8, 0.4, 0.6, 1.0, 1.6]], dtype=np.float32)
        uv, nrm, flat = vertex_data(osc, tv, 22)
        descs, mmap = materials_mod5()
        mat_index = np.arange(len(tv), dtype=np.int32) % 5
    elif name in ("degenerate_small", "quirk"):
        tv = small_scene()
        osc = O.OracleScene(tv)
        o = np.asarray(scenes.OFFGRID_ORIGIN, dtype=np.float32)
        if name == "quirk":
            cam = quirk_camera(osc, tv)
        else:
            cam = FPSCamera(o + np.array([0.0, 0.0, -9.0], dtype=np.float32), 0.0, 0.0).camera()
        lights = centre_lights(osc, [(0.5, 0.55, 0.45, (1.0, 0.9, 0.8), 1.5), (0.35, 0.6, 0.4, (0.4, 0.6, 1.0), 0.06)])
        uv, nrm, flat = vertex_data(osc, tv, 22)
        descs, mmap = materials_mod5()
        mat_index = np.arange(len(tv), dtype=np.int32) % 5
    elif name == "deep":
        tv = scenes.chain()
        osc = O.OracleScene(tv)
        cam = FPSCamera(np.array([-0.25, 0.004, 0.002], dtype=np.float32), -math.pi / 2, 0.0).camera()
        lights = centre_lights(osc, [(0.3, 0.9, 0.8, (1.0, 0.9, 0.8), 2.0)])
        uv, nrm, flat = vertex_data(osc, tv, 23)
        descs, mmap = materials_mod5()
        mat_index = np.arange(len(tv), dtype=np.int32) % 5
    else:
        raise KeyError(name)
    if name.startswith("degenerate"):
        nrm = plane_normals(osc)
        flat = np.ones(len(tv), dtype=bool)
        descs, mmap = [], [-1]
        mat_index = np.zeros(len(tv), dtype=np.int32)
    cam70 = FPSCamera(np.array([-0.5, -0.7, -2.5], dtype=np.float32), 0.0, 0.0).camera() if name == "small" else cam      # (the 70 x 50 frame of the small case: closer)
    return dict(cam70=cam70, tv=tv, osc=osc, uv=uv, nrm=nrm, mat_index=mat_index, flat=flat, descs=descs, material_map=mmap, textures=TEXTURES(), cam=cam, lights=lights)


def quirk_camera(osc, tv):
    """A camera that looks at triangle triId 0 past its edge from close by, so that in some quad lane 0 misses and another lane hits triId 0:
    from a point on the triangle's normal through an edge midpoint, aimed at that midpoint, with the blob behind the camera"""
    t = osc.tris[0]
    a = t["a"].astype(np.float64); ba = t["ba"].astype(np.float64); ca = t["ca"].astype(np.float64)
    nrm = t["plane"][:3].astype(np.float64)
    target = a + 0.5 * ba + 0.02 * ca
    size = max(np.linalg.norm(ba), np.linalg.norm(ca))
    pos = target + nrm / np.linalg.norm(nrm) * size * 2.5
    dirv = target - pos
    ang = math.atan2(dirv[0], dirv[2])
    pitch = -math.atan2(dirv[1], math.hypot(dirv[0], dirv[2]))
    return FPSCamera(pos.astype(np.float32), ang, pitch).camera()


def reference(name):
    c = case(name)
    return M.MaterialsRef(c["osc"], c["uv"], c["nrm"], c["mat_index"], c["flat"], c["material_map"], ref_materials(c["descs"]), [M.RefTexture(t) for t in c["textures"]])
