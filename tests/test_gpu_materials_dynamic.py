"""The material set of a deforming mesh on the MI355X (include/snail_materials_dynamic.h; MaterialSet.from_dev / .rebuild_dev / .update_dev).
Everything is compared for equality, against code that exists and is pinned already: the records against snail_shtris_pack on the host over
the downloaded perm, frames and TreeStats against a STATIC TWIN -- Scene.from_fast + MaterialSet over the same vertices and shading data
(the device's fast tree is byte-equal to the host's: tests/test_gpu_bvh_fast.py).  The scene is the small case's sheet
(tests/materials_cases.py) between two poses A and B."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

from snail_amd import _lib
from snail_amd import materials as P
from snail_amd.scene import Scene
from tests import materials_cases as K
from tests import shtris_dev_ref as R
from tests.test_gpu_materials_transparency import product_materials
from tests.test_materials_dynamic_host import build_c_program

pytestmark = pytest.mark.gpu
ARITH = ["ieee", "host_sse"]
FRAMES = [(96, 64), (70, 50)]       # 24 and 20 packets, the second with partial packets
F = np.float32
TINT = (0.9, 1.0, 0.6)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")      # (a copy: the cached host arrays are read-only)


# ---- the two poses and their shading data (host arrays, computed once, never changed) ----
@functools.lru_cache(maxsize=None)
def poses():
    c = K.case("small")
    tvA = np.ascontiguousarray(c["tv"], dtype=F)
    # a smooth displacement of every vertex by its own position: shared vertices stay shared
    x, y = tvA[..., 0].astype(np.float64), tvA[..., 1].astype(np.float64)
    tvB = tvA.copy()
    tvB[..., 2] = (tvA[..., 2] + 0.22 * np.sin(1.9 * x + 0.4) * np.cos(1.3 * y - 0.2)).astype(F)
    tvB[..., 0] = (tvA[..., 0] + 0.05 * np.sin(2.1 * y)).astype(F)
    nrmA = np.ascontiguousarray(c["nrm"], dtype=F)
    rng = np.random.RandomState(31)
    nrmB = (nrmA + (rng.rand(*nrmA.shape) - 0.5) * 0.5).astype(F)
    out = dict(A=(tvA, nrmA), B=(tvB, nrmB), uv=np.ascontiguousarray(c["uv"], dtype=F), mat_index=np.ascontiguousarray(c["mat_index"], dtype=np.int32),
               flat=np.ascontiguousarray(c["flat"]).astype(np.uint8), cam=c["cam"], cam70=c["cam70"], lights=c["lights"], textures=c["textures"])
    for v in (tvA, tvB, nrmA, nrmB, out["uv"], out["mat_index"], out["flat"]):
        v.setflags(write=False)
    return out


def materials(transparent):
    """(material_map, materials): by input index mod 5 -- default, SIMPLE, TEX, UBER, UBER; the transparent set has UBER with dissolve 0.5 and
    the transparent kind instead of the two opaque UBERs"""
    if transparent:
        descs = [("simple", (0.3, 0.8, 0.6), False), ("tex", 0, True), ("uber", (0.9, 0.4, 0.1), (0.2, 0.6, 1.0), 0.5), ("transp", 0, 1, True)]
        return [-1, 0, 1, 2, 3], product_materials(descs)
    descs, mmap = K.materials_mod5()
    return mmap, product_materials(descs)


def normals_of(pose, kind):
    """the normals a twin is given: the pose's own, or (kind 'face') the restatement's face normals"""
    tv, nrm = poses()[pose]
    return R.vertex_normals_from_faces(tv) if kind == "face" else nrm


_twins = {}


def twin(pose, kind, transparent=False):
    """(Scene.from_fast, MaterialSet) over a pose's vertices and normals: the yardstick, built once per (pose, normals, kind of set)"""
    key = (pose, kind, transparent)
    if key not in _twins:
        p = poses()
        sc = Scene.from_fast(p[pose][0], 0)
        mmap, mats = materials(transparent)
        ms = P.MaterialSet(sc, p["uv"], normals_of(pose, kind), p["mat_index"], p["flat"], mmap, mats, [P.Texture(t) for t in p["textures"]], transparent=transparent)
        _twins[key] = (sc, ms)
    return _twins[key]


def dynamic(torch, kind, transparent=False, pose="A"):
    """a fresh (Scene.from_fast_dev, MaterialSet.from_dev, device tensors) on a pose"""
    p = poses()
    d = {k: (dev(torch, p[k][0]), dev(torch, p[k][1])) for k in "AB"}
    sc = Scene.from_fast_dev(d[pose][0], 0)
    mmap, mats = materials(transparent)
    ms = P.MaterialSet.from_dev(sc, dev(torch, p["uv"]), dev(torch, p["mat_index"]), dev(torch, p["flat"]), mmap, mats, [P.Texture(t) for t in p["textures"]],
                                transparent=transparent, d_nrm=d[pose][1] if kind == "given" else None, d_verts=d[pose][0])
    return sc, ms, d


def nrm_arg(d, pose, kind):
    return d[pose][1] if kind == "given" else None


def frame_of(sc, ms, cam, resx, resy, arith, **kw):
    """(frame bytes, TreeStats) of ms.render in an arithmetic"""
    sc.set_arith(arith)
    try:
        st = sc.new_stats()
        fr = ms.render(cam, resx, resy, poses()["lights"], stats=st, **kw).cpu().numpy()
        return fr, st.cpu().numpy()
    finally:
        sc.set_arith("ieee")


def same(what, got, want):
    bad = int((got[0] != want[0]).sum())
    print("%s: %d differing bytes of %d; stats %s / %s" % (what, bad, want[0].size, got[1].tolist(), want[1].tolist()))
    assert bad == 0 and got[0].shape == want[0].shape, (what, bad)
    assert np.array_equal(got[1], want[1]), (what, got[1], want[1])


def camera(resx):
    return poses()["cam70"] if resx == 70 else poses()["cam"]


def records(ms, n):
    """the set's records now (the workbench library's read-back: test-only, in no header)"""
    fn = _lib.debug_lib().snail_materials_debug_records
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int]
    out = np.zeros((n, 64), dtype=np.uint8)
    assert fn(ms._h, _lib.ptr(out), n) == 0, _lib.debug_lib().snail_last_error()
    return out


# ---- 1. the records ----
@pytest.mark.parametrize("n", [1, 4, 5, 255, 256, 257, 1000])
def test_records_equal_the_host_pack(torch_mod, n):
    """one thread per record in 256-thread blocks, and the builder's hand-offs (root leaf, small list, big levels); random finite data, at
    creation and after a rebuild, with given normals and with face normals"""
    torch = torch_mod
    rng = np.random.RandomState(100 + n)
    tv = [(rng.rand(n, 3, 3) * 4.0 - 2.0 + rng.rand(n, 1, 3) * 6.0).astype(F) for _ in range(2)]
    uv = (rng.rand(n, 3, 2) * 6.0 - 3.0).astype(F)
    nrm = [(rng.rand(n, 3, 3) * 2.0 - 1.0).astype(F) for _ in range(2)]
    nrm[0][0, 1, 2] = F(1e-42)                                                   # a denormal stays one
    mi = rng.randint(0, 7, size=n).astype(np.int32)
    flat = (rng.rand(n) < 0.4).astype(np.uint8)
    mmap = [-1] * 7
    dtv = [dev(torch, t) for t in tv]
    dnrm = [dev(torch, t) for t in nrm]
    for kind in ("given", "face"):
        sc = Scene.from_fast_dev(dtv[0], 0)
        ms = P.MaterialSet.from_dev(sc, dev(torch, uv), dev(torch, mi), dev(torch, flat), mmap, d_nrm=dnrm[0] if kind == "given" else None, d_verts=dtv[0])
        for step in (0, 1):
            if step:
                info = ms.rebuild_dev(dtv[1], dnrm[1] if kind == "given" else None)
                assert info.cpu().numpy().tolist()[0::3] == [0, n] and info.cpu().numpy().tolist()[4:] == [1, 0]
            perm = sc.d_perm.cpu().numpy()
            assert sorted(perm.tolist()) == list(range(n)) and np.array_equal(perm, sc.perm)
            want = P.pack_shtris(uv, nrm[step] if kind == "given" else R.vertex_normals_from_faces(tv[step]), mi, flat, perm)
            got = records(ms, n)
            bad = np.argwhere((got != want).any(axis=1)).ravel()
            print("n = %d, %s normals, step %d: %d differing records" % (n, kind, step, len(bad)))
            assert len(bad) == 0, (bad[:5].tolist(), got[bad[0]].view(np.uint32).tolist(), want[bad[0]].view(np.uint32).tolist())
        if n == 5:      # flat = None means none flat
            ms2 = P.MaterialSet.from_dev(sc, dev(torch, uv), dev(torch, mi), None, mmap, d_nrm=dnrm[1], d_verts=None)
            assert np.array_equal(records(ms2, n), P.pack_shtris(uv, nrm[1], mi, None, sc.d_perm.cpu().numpy()))
            ms2.close()
        ms.close()
        sc.close()


def test_creation_refusals_on_the_device(torch_mod):
    """what snail_shtris_pack and the creators refuse on the host, found on the device before any record is written; and the scenes of
    another kind"""
    torch = torch_mod
    p = poses()
    n = len(p["uv"])
    dv, dn = dev(torch, p["A"][0]), dev(torch, p["A"][1])
    sc = Scene.from_fast_dev(dv, 0)
    mmap, mats = materials(False)
    tex = [P.Texture(t) for t in p["textures"]]
    good = dict(d_uv=dev(torch, p["uv"]), d_mat_index=dev(torch, p["mat_index"]), d_flat=dev(torch, p["flat"]))

    def refused(text, **kw):
        a = dict(good, **kw)
        with pytest.raises(_lib.SnailError, match=text):
            P.MaterialSet.from_dev(sc, a["d_uv"], a["d_mat_index"], a["d_flat"], mmap, mats, tex, d_nrm=dn)

    for bad in (np.inf, np.nan, 1048576.0, -2.0e6):
        uv = p["uv"].copy()
        uv[7, 2, 1] = bad
        refused("triangle 7: texture coordinate not finite or not below 2\\^20", d_uv=dev(torch, uv))
    for bad in (-1, 5):
        mi = p["mat_index"].copy()
        mi[11] = bad
        refused("triangle 11: material index outside the map of 5 entries", d_mat_index=dev(torch, mi))
    keep = sc.d_perm
    sc.d_perm = keep.clone()
    sc.d_perm[3] = n
    refused("perm\\[3\\] is outside")
    sc.d_perm = keep
    # a scene whose tree is never rebuilt: through the C-ABI (the Python class refuses it before)
    host = twin("A", "given")[0]
    with pytest.raises(_lib.SnailError, match="not made by snail_scene_create_fast_dev"):
        P.create_set_dev(host._h, good["d_uv"], good["d_mat_index"], None, n, keep, dn, None, mmap, mats, tex)
    # and the static twin's set is not one of this header's
    L = _lib.lib()
    assert L.snail_materials_update_dev(twin("A", "given")[1]._h, _lib.ptr(keep), _lib.ptr(dn), None, None, None) != 0
    assert "not made by snail_materials_create_dev" in L.snail_last_error().decode()
    sc.close()


# ---- 2. a frame after a rebuild equals the static twin ----
@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("kind", ["given", "face"])
def test_frames_follow_the_rebuild(torch_mod, kind, arith):
    torch = torch_mod
    sc, ms, d = dynamic(torch, kind)
    for resx, resy in FRAMES:
        cam = camera(resx)
        wantA = frame_of(*twin("A", kind), cam, resx, resy, arith)
        wantB = frame_of(*twin("B", kind), cam, resx, resy, arith)
        colours = len(np.unique(wantA[0].reshape(-1, 3), axis=0))
        assert colours > 16 and (wantA[0] != wantB[0]).any(), colours               # not vacuous: on the twin
        same("%s A %dx%d %s" % (kind, resx, resy, arith), frame_of(sc, ms, cam, resx, resy, arith), wantA)
        info = ms.rebuild_dev(d["B"][0], nrm_arg(d, "B", kind))
        same("%s B %dx%d %s" % (kind, resx, resy, arith), frame_of(sc, ms, cam, resx, resy, arith), wantB)
        assert info.cpu().numpy().tolist()[0::3] == [0, len(poses()["uv"])] and info.cpu().numpy().tolist()[4:] == [1, 0]
        ms.rebuild_dev(d["A"][0], nrm_arg(d, "A", kind))                            # back, for the next frame size
    twA = twin("A", kind)[0]
    assert np.array_equal(sc.perm, twA.perm) and sc.bvh.nodes[:len(twA.bvh.nodes)].tobytes() == twA.bvh.nodes.tobytes()
    ms.close(); sc.close()


# ---- 3. every entry family sees the new records ----
@pytest.mark.parametrize("arith", ARITH)
def test_every_entry_family_after_a_rebuild(torch_mod, arith):
    torch = torch_mod
    p = poses()
    resx, resy = 70, 50
    cam = camera(resx)
    pw, ph = (resx + 15) // 16, (resy + 15) // 16
    xy = dev(torch, np.array([[x * 16, y * 16] for y in range(ph) for x in range(pw)], dtype=np.int32))
    # the plain set: the bounce; tiles' packets with 4x AA and a tint
    sc, ms, d = dynamic(torch, "given")
    ms.rebuild_dev(d["B"][0], d["B"][1])
    tsc, tms = twin("B", "given")
    same("bounce", frame_of(sc, ms, cam, resx, resy, arith, reflections=True), frame_of(tsc, tms, cam, resx, resy, arith, reflections=True))
    got, want = [], []
    for s, m, o in ((sc, ms, got), (tsc, tms, want)):
        s.set_arith(arith)
        st = s.new_stats()
        o += [m.frame_packets(cam, resx, resy, xy, p["lights"], flags=P.RENDER_AA4, tint=TINT, stats=st).cpu().numpy(), st.cpu().numpy()]
        s.set_arith("ieee")
    same("frame_packets AA4 + tint", got, want)
    ms.close(); sc.close()
    # the transparent set: the continuation; the tree's packets with the bounce
    sc, ms, d = dynamic(torch, "given", transparent=True)
    ms.rebuild_dev(d["B"][0], d["B"][1])
    tsc, tms = twin("B", "given", transparent=True)
    assert ms.can_select_transparent and tms.can_select_transparent
    for what, call in (("render_transparent", lambda m, st: m.render_transparent(cam, resx, resy, p["lights"], stats=st)),
                       ("tree_frame_packets", lambda m, st: m.tree_frame_packets(cam, resx, resy, xy, p["lights"], flags=P.RENDER_REFLECTIONS, stats=st))):
        got, want = [], []
        for s, m, o in ((sc, ms, got), (tsc, tms, want)):
            s.set_arith(arith)
            st = s.new_stats()
            fr, trunc = call(m, st)
            o += [fr.cpu().numpy(), np.concatenate([st.cpu().numpy(), trunc.cpu().numpy()])]
            s.set_arith("ieee")
        same(what, got, want)
        assert len(np.unique(want[0].reshape(-1, 3), axis=0)) > 16
    # the older entry points refuse the set exactly as they refuse its twin
    for m in (ms, tms):
        with pytest.raises(_lib.SnailError, match="transparent lane"):
            m.render(cam, resx, resy, p["lights"])
    ms.close(); sc.close()


# ---- 4. ordering without host waits ----
def test_two_streams_no_host_wait(torch_mod):
    torch = torch_mod
    p = poses()
    resx, resy = 96, 64
    sc, ms, d = dynamic(torch, "given")
    wantA, wantB = (frame_of(*twin(k, "given"), p["cam"], resx, resy, "ieee") for k in "AB")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = [torch.zeros((resy, resx, 3), dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    stats = [sc.new_stats() for _ in range(2)]
    torch.cuda.synchronize()
    ms.render(p["cam"], resx, resy, p["lights"], out=outs[0], stats=stats[0], stream=s1)
    ms.rebuild_dev(d["B"][0], d["B"][1], stream=s2)
    ms.render(p["cam"], resx, resy, p["lights"], out=outs[1], stats=stats[1], stream=s1)
    torch.cuda.synchronize()
    same("before the rebuild", (outs[0].cpu().numpy(), stats[0].cpu().numpy()), wantA)
    same("after the rebuild", (outs[1].cpu().numpy(), stats[1].cpu().numpy()), wantB)
    ms.close(); sc.close()


# ---- 5. a refused rebuild leaves tree and records together ----
def test_a_refused_rebuild_keeps_tree_and_records(torch_mod):
    torch = torch_mod
    p = poses()
    n = len(p["uv"])
    sc, ms, d = dynamic(torch, "given")
    before = records(ms, n)
    perm_before = sc.d_perm.cpu().numpy()
    bad = p["B"][0].copy()
    bad[n // 2, 1, 2] = np.nan
    info = ms.rebuild_dev(dev(torch, bad), d["B"][1])
    torch.cuda.synchronize()
    assert info.cpu().numpy().tolist() == [1, 0, 0, n, 0, 0]
    assert np.array_equal(records(ms, n), before) and np.array_equal(sc.d_perm.cpu().numpy(), perm_before)
    for resx, resy in FRAMES:
        same("after the refused rebuild %dx%d" % (resx, resy), frame_of(sc, ms, camera(resx), resx, resy, "ieee"), frame_of(*twin("A", "given"), camera(resx), resx, resy, "ieee"))
    # and a good one afterwards is taken
    ms.rebuild_dev(d["B"][0], d["B"][1])
    same("the next rebuild", frame_of(sc, ms, p["cam"], 96, 64, "ieee"), frame_of(*twin("B", "given"), p["cam"], 96, 64, "ieee"))
    ms.close(); sc.close()


# ---- 6. staleness ----
def test_a_rebuild_behind_the_set_is_refused_until_update(torch_mod):
    torch = torch_mod
    p = poses()
    resx, resy = 96, 64
    sc, ms, d = dynamic(torch, "given")
    mmap, mats = materials(False)
    ms2 = P.MaterialSet.from_dev(sc, dev(torch, p["uv"]), dev(torch, p["mat_index"]), dev(torch, p["flat"]), mmap, mats, [P.Texture(t) for t in p["textures"]],
                                 d_nrm=None, d_verts=d["A"][0])
    wantB = frame_of(*twin("B", "given"), p["cam"], resx, resy, "ieee")
    sc.rebuild_fast_dev(d["B"][0])
    for m in (ms, ms2):
        with pytest.raises(_lib.SnailError, match="rebuilt"):
            m.render(p["cam"], resx, resy, p["lights"])
        with pytest.raises(_lib.SnailError, match="rebuilt"):
            m.rebuild_dev(d["A"][0], d["A"][1])
    info = ms.update_dev(d_nrm=d["B"][1])
    same("after update_dev", frame_of(sc, ms, p["cam"], resx, resy, "ieee"), wantB)
    assert info.cpu().numpy().tolist() == [1, 0]
    with pytest.raises(_lib.SnailError, match="rebuilt"):                       # the second set is still the earlier tree's
        ms2.render(p["cam"], resx, resy, p["lights"])
    ms2.update_dev(d_verts=d["B"][0])
    same("the second set, face normals", frame_of(sc, ms2, p["cam"], resx, resy, "ieee"), frame_of(*twin("B", "face"), p["cam"], resx, resy, "ieee"))
    # a rebuild through one set leaves the other stale
    ms.rebuild_dev(d["A"][0], d["A"][1])
    with pytest.raises(_lib.SnailError, match="rebuilt"):
        ms2.render(p["cam"], resx, resy, p["lights"])
    same("the first set", frame_of(sc, ms, p["cam"], resx, resy, "ieee"), frame_of(*twin("A", "given"), p["cam"], resx, resy, "ieee"))
    ms2.close(); ms.close(); sc.close()


# ---- 7. the deviation ----
def test_non_finite_normals_become_zero_normals(torch_mod):
    torch = torch_mod
    p = poses()
    n = len(p["uv"])
    resx, resy = 96, 64
    tvA, nrmA = p["A"]
    # a triangle of the sheet that the 96 x 64 frame sees, made zero-area (its third vertex on its second): the handle is not fastOK
    fr = twin("A", "given")[0].trace_primary(p["cam"], resx, resy)
    torch.cuda.synchronize()
    ids, counts = np.unique(fr.tri_id.cpu().numpy()[np.isfinite(fr.t.cpu().numpy())], return_counts=True)
    seen = ids[(counts >= 4) & (counts <= 100)]                                  # (the backdrop's two triangles take thousands)
    assert len(seen) > 10
    z = int(twin("A", "given")[0].perm[seen[len(seen) // 2]])                    # an input triangle of the sheet with several pixels
    tvZ = tvA.copy()
    tvZ[z, 2] = tvZ[z, 1]
    nrmI = nrmA.copy()
    nrmI[z, 1, 0] = np.inf
    mmap, mats = materials(False)
    tex = [P.Texture(t) for t in p["textures"]]
    dZ = dev(torch, tvZ)
    for what, d_nrm, tv, twin_nrm in (("face normal of a zero-area triangle", None, tvZ, R.vertex_normals_from_faces(tvZ)), ("a given inf", dev(torch, nrmI), tvA, nrmI)):
        assert not np.isfinite(twin_nrm[z]).all()
        zeroed, count = R.zero_nonfinite(twin_nrm)
        assert count == 1 and not zeroed[z].any()
        dv = dZ if tv is tvZ else dev(torch, tvA)
        sc = Scene.from_fast_dev(dv, 0)
        ms = P.MaterialSet.from_dev(sc, dev(torch, p["uv"]), dev(torch, p["mat_index"]), dev(torch, p["flat"]), mmap, mats, tex, d_nrm=d_nrm, d_verts=dv)
        info = ms.update_dev(d_nrm=d_nrm, d_verts=dv)
        info6 = ms.rebuild_dev(dv, d_nrm)
        torch.cuda.synchronize()
        assert info.cpu().numpy().tolist() == [1, 1] and info6.cpu().numpy().tolist()[4:] == [1, 1] and info6.cpu().numpy()[0] == 0, (what, info6)
        rec = records(ms, n).view(F).reshape(n, 16)
        slot = int(np.flatnonzero(sc.d_perm.cpu().numpy() == z)[0])
        assert not rec[slot, 6:15].any() and np.isfinite(rec[:, :15]).all()
        tsc = Scene.from_fast(tv, 0)
        tms = P.MaterialSet(tsc, p["uv"], zeroed, p["mat_index"], p["flat"], mmap, mats, tex)
        assert np.array_equal(records(tms, n), records(ms, n))
        for arith in ARITH:
            same("%s, %s" % (what, arith), frame_of(sc, ms, p["cam"], resx, resy, arith), frame_of(tsc, tms, p["cam"], resx, resy, arith))
        tms.close(); tsc.close(); ms.close(); sc.close()


# ---- the C-ABI from a C host ----
def test_c_program_create_rebuild_render_update(torch_mod, tmp_path):
    exe, _ = build_c_program(tmp_path)
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "C materials dynamic frames ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
