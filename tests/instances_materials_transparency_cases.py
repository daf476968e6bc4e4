"""The cases of the instanced transparency tests (tests/test_instances_materials_transparency_host.py,
tests/test_gpu_instances_materials_transparency.py), chosen with the restatement (tests/instances_materials_transparency_ref.py) alone, on the
CPU; what they must exercise is asserted on the restatement's counters in the host test, with and without a GPU.
  glasshouse   the sheet and box BLASes of tests/instances_materials_cases.py in its six instances as the backdrop, and before them
               BLAS `pane` -- one rect of a TRANSPARENT material whose opacity map holds texels with first byte 0, mid values and 255 -- in three
               instances staggered so that rays cross one, two and three of them (the identity, an exact quarter turn about z, a general
               rotation), and BLAS `pane2` -- one rect whose triangles map to UBER dissolve 0.5 and to the UBER dissolve 1.0 entry that the sheet's and
               the box's maps name as well (flagged, never selected, de-selects neighbours in branch (c)) -- in two instances
  deep         the depth > 62 `chain` BLAS of the bounce cases in its two instances behind one pane, under one light
  moved        glasshouse after an update: every instance turned a little, the panes pushed aside
  invisible    panes whose opacity map is zero everywhere before SIMPLE materials without N.R, no lights: the panes must not show
Everything is seeded and float32; nothing here touches a device."""
from __future__ import annotations

import functools

import numpy as np

from snail_amd import FPSCamera
from tests import instances_materials_cases as K
from tests import instances_materials_ref as IM
from tests import instances_materials_transparency_ref as IT
from tests import materials_ref as M
from tests import materials_transparency_cases as TK
from tests import oracle_lib as O

F = np.float32
FRAMES = [(96, 64), (70, 50), (64, 48)]       # 24, 20 (partial packets) and 12 packets
# ONE scene-wide list: instances_materials_cases.DESCS (4 = UBER dissolve 1.0, which both of its maps name), then the kinds that can select
DESCS = list(K.DESCS) + [("transp", 0, 2, True), ("uber", (0.8, 0.5, 0.3), (0.3, 0.2, 0.9), 0.5), ("transp", 1, 3, False)]
M_PANE, M_HALF, M_CLEAR, M_SHARED = 5, 6, 7, 4
PANE_MAP = [M_PANE]
PANE2_MAP = [M_HALF, M_SHARED]
ROT90Z = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], dtype=np.float32)       # exact


def textures():
    """instances_materials_cases' two, materials_transparency_cases' opacity map (byte 0 by column: 0, 255, then a ramp) and one that is 0 everywhere"""
    return K.TEXTURES() + [TK.opacity_texture(), np.zeros((4, 4, 3), dtype=np.uint8)]


def rect_blas(w, h, classes, seed):
    """one rect [-w, w] x [-h, h] at z = 0 of two triangles, uv over [0, 1]^2, normals towards -z bent a little (the lights stand before the
    panes: N.L > 0) -> (tv [2, 9], oracle scene, (uv, nrm, mat_index, flat, map left to the caller))"""
    a, b, c, d = (-w, -h, 0.0), (w, -h, 0.0), (w, h, 0.0), (-w, h, 0.0)
    tv = np.ascontiguousarray(np.array([(a, b, c), (a, c, d)], dtype=np.float32))
    uvs = {a: (0.0, 0.0), b: (1.0, 0.0), c: (1.0, 1.0), d: (0.0, 1.0)}
    uv = np.array([[uvs[v] for v in tri] for tri in ((a, b, c), (a, c, d))], dtype=np.float32)
    rng = np.random.RandomState(seed)
    nrm = (np.array([0.0, 0.0, 1.0]) + (rng.rand(2, 3, 3) - 0.5) * 0.4).astype(np.float32)
    osc = O.OracleScene(tv.reshape(-1, 9))
    return tv.reshape(-1, 9), osc, (uv, nrm, np.array(classes, dtype=np.int32), np.zeros(2, dtype=bool))


@functools.lru_cache(maxsize=None)
def pane_blases():
    p = rect_blas(1.0, 0.8, [0, 0], 41)
    q = rect_blas(0.9, 0.6, [0, 1], 42)
    return [(p[0], p[1], p[2] + (PANE_MAP,)), (q[0], q[1], q[2] + (PANE2_MAP,))]


def glasshouse_instances():
    """(rot, tr, blas index); BLAS 0 = sheet, 1 = box, 2 = pane, 3 = pane2.  Given order: instances_materials_cases.main_instances' six, then
      6  pane, the identity                       7  pane, an exact quarter turn about z           8  pane, a general rotation
      9  pane2, the identity, low on the left     10 pane2, turned by 180 degrees about z, overlapping 9 and the panes on screen"""
    rot, tr, bi = K.main_instances()
    g = K.general_rotation()
    rot = np.concatenate([rot, np.stack([np.eye(3, dtype=np.float32), ROT90Z, g, np.eye(3, dtype=np.float32), K.ROT180Z])])
    tr = np.concatenate([tr, np.array([[0.3, 0.3, -1.9], [1.3, 0.0, -2.5], [1.9, 0.5, -3.1], [0.2, -0.9, -2.2], [1.0, -0.7, -2.8]], dtype=np.float32)])
    return rot, tr, np.concatenate([bi, np.array([2, 2, 2, 3, 3], dtype=np.int32)])


@functools.lru_cache(maxsize=None)
def case(name, panes=True):
    """-> dict(tvs, oscs, per_blas, rot, tr, bi, ref (restatement scene), cams (resx -> camera), lights, descs); panes=False: the same scene
    without the instances of the pane BLASes (the BLAS list stays)"""
    base = K.blas_data()
    pb = pane_blases()
    if name in ("glasshouse", "moved"):
        data = list(base) + pb
        rot, tr, bi = glasshouse_instances()
        if name == "moved":      # every instance turned a little and the panes pushed aside: what an update of the same handle brings
            turn = K.rot_axis((0, 1, 0), 0.15)
            rot = np.stack([(turn.astype(np.float64) @ r.astype(np.float64)).astype(np.float32) for r in rot])
            tr = tr.copy(); tr[bi >= 2] += np.array([0.35, -0.2, 0.1], dtype=np.float32)
        m = K.case("main")
        cams, lights = dict(m["cams"]), m["lights"]
        descs = DESCS
    elif name == "deep":
        d = K.case("deep")
        data = [(d["tvs"][0], d["oscs"][0], d["per_blas"][0]), pb[0]]
        cam = d["cams"][64]
        # one pane a little before the camera, which looks along +x: an exact quarter turn about y brings the rect into the yz-plane, its normal
        # to +x; moved up so that its lower edge crosses the view -- packets wholly behind it, across its edge and beside it
        rot = np.concatenate([d["rot"], K.ROT90Y[None]])
        pos = np.asarray(cam.as_array13()[:3], dtype=np.float32)
        tr = np.concatenate([d["tr"], (pos + np.array([0.2, 0.75, 0.5], dtype=np.float32))[None]])
        bi = np.concatenate([d["bi"], np.array([1], dtype=np.int32)])
        cams, lights = {64: cam}, d["lights"]
        descs = DESCS
    elif name == "invisible":
        data = list(base) + pb
        rot, tr, bi = glasshouse_instances()
        bi = bi.copy()
        m = K.case("main")
        # (the camera was moved until the restatement's frame equals its frame of the scene without the panes, at all three frame sizes: from
        # instances_materials_cases' own, 12 to 14 continuation rays across an edge of the backdrop land on the other side of it)
        cam = FPSCamera(np.array([0.9, 0.15, -4.7], dtype=np.float32), 0.04, -0.02).camera()
        cams, lights = {96: cam, 70: cam, 64: cam}, np.zeros((0, 7), dtype=np.float32)
        # every backdrop material SIMPLE without N.R; both pane BLASes map to the TRANSPARENT material over the all-zero opacity map
        descs = [("simple", (0.1 + 0.1 * k, 0.9 - 0.1 * k, 0.3 + 0.05 * k), False) for k in range(5)] + [DESCS[5], DESCS[6], ("transp", 1, 3, False)]
        data = data[:2] + [(pb[0][0], pb[0][1], pb[0][2][:4] + ([M_CLEAR],)), (pb[1][0], pb[1][1], pb[1][2][:4] + ([M_CLEAR, M_CLEAR],))]
    else:
        raise KeyError(name)
    if not panes:
        first_pane = len(data) - (1 if name == "deep" else 2)
        keep = bi < first_pane
        rot, tr, bi = rot[keep], tr[keep], bi[keep]
    tvs, oscs, per_blas = [d[0] for d in data], [d[1] for d in data], [d[2] for d in data]
    return dict(tvs=tvs, oscs=oscs, per_blas=per_blas, rot=rot, tr=tr, bi=bi, ref=K.cpu_ref(oscs, rot, tr, bi), cams=cams, lights=lights, descs=descs)


def ref_textures():
    return [M.RefTexture(t) for t in textures()]


def opaque_descs(ds):
    """the list with opaque stand-ins: TRANSPARENT -> TEX over the colour map, UBER with 0 < dissolve < 1 -> UBER 0"""
    return [("tex", d[1], d[3]) if d[0] == "transp" else ("uber", d[1], d[2], 0.0) if d[0] == "uber" and 0.0 < d[3] < 1.0 else d for d in ds]


def materials_ref(name, panes=True, opaque=False):
    c = case(name, panes)
    ds = opaque_descs(c["descs"]) if opaque else c["descs"]
    return IM.InstMaterialsRef(c["ref"], c["per_blas"], TK.ref_materials(ds), ref_textures())


def lights_of(name, key):
    """the case's lights, none, or eight before the sheets with radii large enough that none is culled everywhere"""
    if key == "case":
        return case(name)["lights"]
    if key == "none":
        return None
    return np.array([[-2.0 + 0.6 * k, -0.8 + 0.3 * k, -3.6 - 0.1 * k, 1.0 - 0.1 * k, 0.5, 0.2 + 0.1 * k, 3.0 + 0.8 * k] for k in range(8)], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def reference(name, resx, resy, mode=O.MODE_IEEE, lights_key="case", max_depth=8, mutation=None, panes=True, opaque=False, shadows=False):
    """the restatement's frame, TreeStats, truncated lanes, counters, packet list and per-packet level records: computed once per argument
    list, shared, never changed.  shadows=True also counts the shadow lanes that only the pane instances occlude."""
    c = case(name, panes)
    d = IT.FrameDiag()
    rec = []
    fr = IT.InstTranspFrames(IT.InstTranspRef(materials_ref(name, panes, opaque), mutation), without=case(name, False)["ref"] if shadows else None)
    frame, st, trunc, d, xy = fr.render(c["cams"][resx].as_array13(), resx, resy, lights_of(name, lights_key), mode=mode, max_depth=max_depth, diag=d, record=rec)
    for a in (frame, st, xy):
        a.setflags(write=False)
    return frame, st, trunc, d, xy, rec


@functools.lru_cache(maxsize=None)
def plain_reference(name, resx, resy, mode=O.MODE_IEEE, lights_key="case", panes=True, opaque=True):
    """tests/instances_materials_ref.py's frame of a set without capable materials: what the existing frame functions give"""
    c = case(name, panes)
    frame, st, _smp, _xy = materials_ref(name, panes, opaque).render(c["cams"][resx].as_array13(), resx, resy, lights_of(name, lights_key), mode=mode)
    frame.setflags(write=False); st.setflags(write=False)
    return frame, st


def level_records(rec, level):
    """reference()'s records of one level, stacked over the packets that reached it -> (packet indices, dict of arrays)"""
    idx, rows = [], []
    for p, levels in enumerate(rec):
        for r in levels:
            if r["level"] == level:
                idx.append(p); rows.append(r)
    if not rows:
        return np.zeros(0, dtype=np.int64), {}
    out = {k: np.ascontiguousarray(np.stack([r[k] for r in rows])) for k in ("t", "inst", "tri_id", "bary", "samples", "opacity", "sel")}
    if level:
        for k in ("origin", "dir", "idir", "mask", "distance"):
            out[k] = np.ascontiguousarray(np.stack([r["rays"][k] for r in rows]))
    return np.array(idx, dtype=np.int64), out


def packet_results(rec):
    """reference()'s per-packet bytes [n,256,3], TreeStats [n,4] and truncated lanes [n]"""
    last = [levels[-1] for levels in rec]
    assert all(r["level"] == -1 for r in last)
    return np.stack([r["bgr"] for r in last]), np.stack([r["stats"] for r in last]), np.array([r["truncated"] for r in last], dtype=np.uint64)


def describe(d):
    s = d.samples
    return ("deepest %d; lanes per level %s; nested <0,0> %s <0,1> %s none %s; truncated %d; (c) overwritten %d, lanes de-selected %d; same triId on two slots in (b) %d; "
            "two BLASes one material %d (flagged %d); TRANSPARENT lanes with opacity >= 1 %d; culled / kept (packet, light) per level %s; pane-shadowed lanes %d; "
            "slots hit per level %s" % (d.deepest, dict(d.level_selected), dict(d.nested_full), dict(d.nested_masked), dict(d.nested_none), d.truncated, s.c_overwritten,
                                        s.c_deselected_lanes, s.same_tri_two_slots_b, s.two_blas_one_material, s.two_blas_one_flagged, s.transparent_opaque_lanes,
                                        {k: (len(v.culled), len(v.not_culled)) for k, v in sorted(d.lights.items())}, d.pane_shadow_lanes,
                                        {k: sorted(v) for k, v in sorted(d.level_hit_slots.items())}))
