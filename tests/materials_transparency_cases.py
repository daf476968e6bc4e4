"""Inputs of the transparency stages' tests (tests/test_materials_transparency_host.py, tests/test_gpu_materials_transparency.py), chosen with the
restatement alone, on the CPU.  The stages take their hit records from the caller, so the SYNTHETIC records of tests/materials_synth.py serve:
its triangles, map, packets and ten noise textures, with another material list behind the same map --
  TRANSPARENT over the noise textures (colour k, opacity (k + 3) % 10; with and without N.R), one whose opacity map is 255 everywhere (opacity
  exactly 1: flagged, never selected), one whose opacity map is 0 everywhere, TEX kept for every third texture, SIMPLE, and UBER with dissolve
  0 (not flagged), 0.5 (selects) and 1.0 (flagged, never selected, and overwrites a neighbour's lanes in the selector)
-- and, for the generator, selectors and generic rays of their own.  Seeded numpy, float32; nothing here touches the product library."""
from __future__ import annotations

import functools

import numpy as np

from tests import materials_cases as K
from tests import materials_ref as M
from tests import materials_synth as Y
from tests import materials_transparency_ref as T
from tests import oracle_lib as O

F = np.float32
INF = F(np.inf)
N_TEX = len(Y.SHAPES)
TEX_OPAQUE, TEX_CLEAR = N_TEX, N_TEX + 1       # two more textures: 255 everywhere, 0 everywhere (4 x 4)


def descs():
    """the 14 materials behind materials_synth.MAP, in the form of tests/materials_cases.py plus ("transp", colour map, opacity map, N.R)"""
    d = []
    for k in range(N_TEX):
        if k % 3 == 0:
            d.append(("tex", k, k % 2 == 0))
        else:
            d.append(("transp", k, TEX_OPAQUE if k == 1 else TEX_CLEAR if k == 2 else (k + 3) % N_TEX, k % 2 == 0))
    d += [("simple", (0.9, 0.5, 0.2), True), ("uber", (0.3, 0.8, 0.6), (0.4, 0.1, 0.7), 0.5)]
    d += [("uber", (0.9, 0.4, 0.1), (0.2, 0.6, 1.0), 0.0), ("uber", (0.2, 0.7, 0.5), (1.0, 0.3, 0.1), 1.0)]
    return d


def descs_opaque():
    """the same list with opaque stand-ins: a set of the new creator WITHOUT a transparent-capable material (TRANSPARENT -> TEX over the colour
    map, UBER 0.5 -> UBER 0)"""
    out = []
    for d in descs():
        if d[0] == "transp":
            out.append(("tex", d[1], d[3]))
        elif d[0] == "uber" and 0.0 < d[3] < 1.0:
            out.append(("uber", d[1], d[2], 0.0))
        else:
            out.append(d)
    return out


def textures():
    s = Y.synth()
    return list(s.textures) + [np.full((4, 4, 3), 255, dtype=np.uint8), np.zeros((4, 4, 3), dtype=np.uint8)]


def ref_materials(ds):
    return [T.TranspMaterial(d[1], d[2], d[3]) if d[0] == "transp" else K.ref_materials([d])[0] for d in ds]


@functools.lru_cache(maxsize=None)
def reference(opaque=False):
    """the restatement over the synthetic triangles with the lists above"""
    s = Y.synth()
    tx = Y.ref_textures() + [M.RefTexture(t) for t in textures()[N_TEX:]]
    return T.TranspRef(M.MaterialsRef(s.osc, s.uv, s.nrm, s.mat_index, s.flat, s.material_map, ref_materials(descs_opaque() if opaque else descs()), tx))


def stack(outs):
    """per-packet (hit, nrm, diffuse, specular, opacity, sel) -> dict(samples [n,9,64,4], opacity [n,256], sel uint8 [n,64]), read-only"""
    r = dict(samples=np.stack([Y.to_planes(o[1], o[2], o[3]) for o in outs]), opacity=np.stack([o[4] for o in outs]).reshape(len(outs), 256),
             sel=np.stack([T.sel_bytes(o[5]) for o in outs]))
    for a in r.values():
        a.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def expected_primary(mode, opaque=False):
    """the restatement's samples, opacity and selector of materials_synth's primary list -> (dict, TranspDiag); computed once, shared"""
    s, ref, diag = Y.synth(), reference(opaque), T.TranspDiag()
    xy = s.packet_xy()
    outs = []
    for p in range(Y.N_PACKETS):
        pk = s.packet(p)
        outs.append(ref.samples(Y.primary_dirs(int(xy[p, 0]), int(xy[p, 1]), mode), pk["t"], Y.clamp_ids(pk["tri"], s.n), pk["bary"], None, diag))
    return stack(outs), diag


@functools.lru_cache(maxsize=None)
def expected_generic(opaque=False):
    """... of the generic list (the packets' own directions and selectors; no arithmetic mode enters)"""
    s, ref, diag = Y.synth(), reference(opaque), T.TranspDiag()
    outs = []
    for p in range(Y.N_PACKETS):
        pk = s.packet(p, generic=True)
        outs.append(ref.samples(pk["dirs"], pk["t"], Y.clamp_ids(pk["tri"], s.n), pk["bary"], pk["bits"], diag))
    return stack(outs), diag


def check_conditions(d: T.TranspDiag, generic):
    """what a list must exercise for a comparison over it to mean something"""
    assert d.blocks_a_flag >= 32 and d.blocks_b_flag >= 16 and d.blocks_c_flag >= 32, (d.blocks_a_flag, d.blocks_b_flag, d.blocks_c_flag)
    assert d.a_transparent >= 32 and d.a_transparent_texdiff >= 8, (d.a_transparent, d.a_transparent_texdiff)
    assert d.c_overwritten >= 16 and d.c_overwritten_by_opaque_uber >= 2 and d.c_lost_selectable >= 16, (d.c_overwritten, d.c_overwritten_by_opaque_uber, d.c_lost_selectable)
    assert d.flagged_opaque_lanes >= 64 and d.opacity_zero_lanes >= 64 and d.selected_lanes >= 1024, (d.flagged_opaque_lanes, d.opacity_zero_lanes, d.selected_lanes)
    assert d.packets_some >= 16, d.packets_some      # (every packet of these lists selects a lane; packets that select none are the generator's inputs')


def describe(d: T.TranspDiag):
    return ("flagged blocks a/b/c %d/%d/%d; (a) TRANSPARENT %d, with a texDiff that mip-mapping would have used %d; (c) overwritten %d, by UBER >= 1 %d, selectable "
            "lanes lost %d; flagged lanes with opacity >= 1 %d, selected with opacity 0 %d, selected %d; packets none/some/all %d/%d/%d" % (
                d.blocks_a_flag, d.blocks_b_flag, d.blocks_c_flag, d.a_transparent, d.a_transparent_texdiff, d.c_overwritten, d.c_overwritten_by_opaque_uber,
                d.c_lost_selectable, d.flagged_opaque_lanes, d.opacity_zero_lanes, d.selected_lanes, d.packets_none, d.packets_some, d.packets_all))


# ---- the generator's inputs ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def continue_inputs():
    """the packets and distances of materials_synth.mirror_inputs() (20 packets of the 70 x 50 frame: all lanes hit, none, half, ...) with
    selectors of their own -> dict(xy [n,2], t [n,64,4], sel bool [n,64,4], origin / dir / idir [n,64,3,4]): per packet k % 5 == 0 every hit lane
    selected (packet 0: all 256), 1 none hit, 2 / 3 a random subset INCLUDING bits on lanes that missed (which the generator must drop), 4 no
    bit at all although lanes hit.  The generic rays: unit directions, origins in a box, and inverse directions that are NOT SafeInv(dir)
    (random values: the generator hands a level's idir on, it does not compute it)"""
    xy, t, _ = Y.mirror_inputs()
    n = len(xy)
    rng = np.random.RandomState(9107)
    sel = rng.rand(n, 64, 4) < 0.5
    for p in range(n):
        if p % 5 == 0:
            sel[p] = True
        elif p % 5 == 4:
            sel[p] = False
    d = rng.normal(size=(n, 64, 3, 4)); d /= np.sqrt((d * d).sum(axis=2, keepdims=True))
    r = dict(xy=xy, t=t, sel=sel, origin=rng.uniform(-5.0, 5.0, size=(n, 64, 3, 4)).astype(np.float32), dir=np.ascontiguousarray(d.astype(np.float32)),
             idir=rng.uniform(-40.0, 40.0, size=(n, 64, 3, 4)).astype(np.float32))
    for a in r.values():
        a.setflags(write=False)
    return r


KEYS = ("origin", "dir", "idir", "mask", "distance", "object")


@functools.lru_cache(maxsize=None)
def expected_continue(mode, generic):
    """TranspRef.continue_packets on continue_inputs() -> (dict of stacked arrays + order int32 [n], the selected lanes)"""
    c = continue_inputs()
    n = len(c["xy"])
    org = np.repeat(Y.CAM13[:3].reshape(1, 3, 1), 4, axis=2).astype(np.float32)
    outs = []
    for p in range(n):
        if generic:
            outs.append(T.TranspRef.continue_packets(c["dir"][p], c["origin"][p], c["idir"][p], c["t"][p], c["sel"][p], mode))
        else:
            outs.append(T.TranspRef.continue_packets(Y.primary_dirs(int(c["xy"][p, 0]), int(c["xy"][p, 1]), mode), org, None, c["t"][p], c["sel"][p], mode))
    want = {k: np.ascontiguousarray(np.stack([o[k] for o in outs])) for k in KEYS}
    want["order"] = np.array([p if outs[p]["order_on"] else -1 for p in range(n)], dtype=np.int32)
    return want, int((c["sel"] & (c["t"] < INF)).sum())


# ---- the existing cases with one material swapped for a transparent kind -----------------------------------------------------------------
SWAPPED = ["small", "large"]
SWAP_FRAME = (70, 50)                                              # 5 x 4 packets, the last column and row partial


@functools.lru_cache(maxsize=None)
def swapped_case(name):
    """tests/materials_cases.py's case with its first TEX material swapped for TRANSPARENT (the other texture as the opacity map) and, where it
    has one, UBER 0 for UBER 0.5 -> (case dict with the new descs, TranspRef)"""
    c = dict(K.case(name))
    ds, first = [], True
    for d in c["descs"]:
        if d[0] == "tex" and first:
            ds.append(("transp", d[1], 1 - d[1], d[2])); first = False
        elif d[0] == "uber" and d[3] == 0.0:
            ds.append(("uber", d[1], d[2], 0.5))
        else:
            ds.append(d)
    assert not first
    c["descs"] = ds
    ref = M.MaterialsRef(c["osc"], c["uv"], c["nrm"], c["mat_index"], c["flat"], c["material_map"], ref_materials(ds), [M.RefTexture(t) for t in c["textures"]])
    return c, T.TranspRef(ref)


@functools.lru_cache(maxsize=None)
def swapped_descent(name, mode):
    """materials_transparency_ref.descend over the 70 x 50 frame of a swapped case -> (levels, stats, packet list, TranspDiag)"""
    from tests import dbvh_shade_ref as S
    c, tr = swapped_case(name)
    xy = S.frame_packets(*SWAP_FRAME)
    diag = T.TranspDiag()
    levels, stats = T.descend(tr, c["cam70"].as_array13(), SWAP_FRAME[0], SWAP_FRAME[1], xy, mode, diag)
    return levels, stats, np.asarray(xy, dtype=np.int32).reshape(-1, 2), diag


# ---- panes: five two-triangle panes one behind the other, then a back wall ---------------------------------------------------------------
PANES_FRAMES = [(96, 64), (70, 50)]


def opacity_texture():
    """64 x 64, byte 0 (the opacity channel) by column: 0 for columns 0..15, 255 for 16..31, then a ramp 0..255 -- so bilinear taps give exactly
    0, exactly 1, and everything between; the other two bytes are noise"""
    t = np.random.RandomState(77).randint(0, 256, size=(64, 64, 3)).astype(np.uint8)
    col = np.concatenate([np.zeros(16), np.full(16, 255), np.round(np.linspace(0, 255, 32))]).astype(np.uint8)
    t[:, :, 0] = col[None, :]
    return t


@functools.lru_cache(maxsize=None)
def panes():
    """-> dict in the form of materials_cases.case(): the centre pane (UBER 0.5) covers whole packets; panes 1 and 4 pair a TRANSPARENT triangle
    with an UBER 1.0 one, in either order, and pane 3 with an UBER 0.5 one, along diagonals that cross blocks -- UBER 1.0 comes later in a
    block's material list than its TRANSPARENT neighbour both among the primary hits (pane 1) and at nested levels (pane 4); panes overlap only partly and the wall is smaller than the view, so
    continuations hit, miss and nest up to five levels; the second light's radius lets the cull remove it for packets of the deeper levels"""
    from snail_amd import FPSCamera
    rects = [(-1.2, 1.2, -0.8, 0.8, 0.0), (-2.6, 0.6, -1.9, 0.7, 1.0), (-0.7, 2.2, -0.6, 1.5, 2.0), (-1.5, 1.5, -1.1, 1.1, 3.0), (-0.9, 1.9, -1.3, 0.9, 4.0),
             (-2.5, 2.5, -1.2, 1.8, 5.5)]
    tv, uv = [], []
    for x0, x1, y0, y1, z in rects:
        a, b, c, d = (x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)
        for tri in ((a, b, c), (a, c, d)):
            tv.append(tri)
            uv.append([(0.37 * v[0] + 0.05 * z, 0.41 * v[1] - 0.03 * z) for v in tri])
    tv = np.ascontiguousarray(np.array(tv, dtype=np.float32))
    osc = O.OracleScene(tv)
    rng = np.random.RandomState(31)
    nrm = (np.array([0.0, 0.0, 1.0]) + (rng.rand(len(tv), 3, 3) - 0.5) * 0.5).astype(np.float32)      # away from the lights in front: N.L > 0 there
    descs = [("uber", (0.9, 0.4, 0.1), (0.2, 0.6, 1.0), 0.5), ("transp", 0, 2, True), ("uber", (0.2, 0.7, 0.5), (1.0, 0.3, 0.1), 1.0), ("transp", 1, 2, False),
             ("simple", (0.3, 0.8, 0.6), True), ("tex", 0, True)]
    #            pane 0   pane 1   pane 2   pane 3   pane 4   wall
    mat_index = [0, 0,    2, 1,    3, 3,    0, 1,    1, 2,    4, 5]
    lights = np.array([[-0.5, 0.6, -2.0, 1.0, 0.9, 0.8, 30.0], [0.8, -0.3, -0.7, 0.4, 0.6, 1.0, 1.6]], dtype=np.float32)
    cam = FPSCamera(np.array([0.1, 0.05, -3.0], dtype=np.float32), 0.0, 0.0).camera()
    return dict(tv=tv, osc=osc, uv=np.array(uv, dtype=np.float32), nrm=nrm, mat_index=np.array(mat_index, dtype=np.int32), flat=np.arange(len(tv)) % 3 == 1, descs=descs,
                material_map=[0, 1, 2, 3, 4, 5], textures=[K.checker_texture(64, 64, 3), K.checker_texture(32, 8, 4), opacity_texture()], cam=cam, cam70=cam, lights=lights)


def case_ref(c, opaque=False):
    ds = c["descs"]
    if opaque:
        ds = [("tex", d[1], d[3]) if d[0] == "transp" else ("uber", d[1], d[2], 0.0) if d[0] == "uber" and 0.0 < d[3] < 1.0 else d for d in ds]
    return T.TranspFrames(T.TranspRef(M.MaterialsRef(c["osc"], c["uv"], c["nrm"], c["mat_index"], c["flat"], c["material_map"], ref_materials(ds), [M.RefTexture(t) for t in c["textures"]])))


def eight_lights(c):
    rng = np.random.RandomState(5)
    l = np.zeros((8, 7), dtype=np.float32)
    l[:, 0:3] = rng.uniform([-2.5, -1.5, -2.5], [2.5, 1.5, 5.0], size=(8, 3)); l[:, 3:6] = rng.uniform(0.2, 1.0, size=(8, 3)); l[:, 6] = rng.uniform(1.0, 12.0, size=8)
    l[0:2] = c["lights"]
    return l


def lights_of(c, key):
    return None if key == "none" else eight_lights(c) if key == "eight" else c["lights"]


@functools.lru_cache(maxsize=None)
def panes_frame(resx, resy, mode, max_depth=8, lights="case"):
    """the restatement's frame of `panes` -> (frame, stats, truncated, FrameDiag, packet list); computed once, shared"""
    c = panes()
    out = case_ref(c).render(c["cam"].as_array13(), resx, resy, lights_of(c, lights), mode=mode, max_depth=max_depth)
    out[0].setflags(write=False)
    return out


def describe_frame(d):
    s = d.samples
    return ("deepest %d; nested <0,0> %s <0,1> %s none %s; continuation hits/misses %d/%d; truncated %d; culled pairs per level %s; %s" % (
        d.deepest, dict(d.nested_full), dict(d.nested_masked), dict(d.nested_none), d.continuation_hits, d.continuation_misses, d.truncated,
        {k: len(v.culled) for k, v in sorted(d.lights.items())}, describe(s))) + "; UBER >= 1 overwrites per level %s" % dict(sorted(d.opaque_uber_overwrites.items()))
