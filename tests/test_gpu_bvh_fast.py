"""The fast builder on the device (snail_scene_create_fast_dev / snail_scene_rebuild_fast_dev, include/snail_bvh_fast.h): the handle's
nodes, triangle records and perm are byte-equal to snail_tris_from_verts + snail_bvh_build_fast on the same vertices, frames traced from
the handle equal the oracle's over the downloaded tree in both arithmetics, and a rebuild is ordered against launches without host waits.

Sizes straddle the hand-offs of snail_amd/csrc/bvh_fast.inc: 4 | 5 (root leaf | root onto the small list: SplitBvh::minSplit) and
64 | 65 (kSmall: one wave finishes the subtree | a 256-thread workgroup per node and level); 256 | 257 is the big kernel's block size."""
import numpy as np
import pytest

from tests import oracle_lib as O
from tests import dbvh_ref as D
from tests import util as U
from tests.test_bvh_fast_host import CHAINS, big_leaf_soup, deep_line, empty_side_field, fixture, identical_tris, signed_zero_tris, soup

pytestmark = pytest.mark.gpu
THRESHOLDS = (4, 5, 64, 65, 256, 257)      # SplitBvh::minSplit - 1 | minSplit, devb::kSmall | kSmall + 1, k_build_big's block | + 1


def dev_scene(tv):
    import torch
    from snail_amd.scene import Scene
    return Scene.from_fast_dev(torch.from_numpy(np.ascontiguousarray(tv, np.float32)).cuda())


def check_build(tv):
    import torch
    from snail_amd import HostBVH
    hb = HostBVH.build_fast(tv)
    sc = dev_scene(tv)
    try:
        torch.cuda.synchronize()
        info = sc.d_info.cpu().numpy().tolist()
        assert info == [0, len(hb.nodes), hb.depth, len(tv)], info
        got = sc.bvh
        assert got.depth == hb.depth and len(got.nodes) == len(hb.nodes)
        assert np.array_equal(got.perm, hb.perm)
        assert got.nodes.tobytes() == hb.nodes.tobytes()
        assert got.tris.tobytes() == hb.tris.tobytes()
    finally:
        sc.close()


@pytest.mark.parametrize("n", sorted(set((1, 4, 5, 63, 64, 65, 255, 256, 257, 1000, 5003) + tuple(t + d for t in THRESHOLDS for d in (-1, 0, 1)))))
def test_device_tree_is_byte_equal_to_the_host_tree(n):
    check_build(soup(n, 200 + n))


def test_lancia_is_byte_equal():
    check_build(fixture("lancia"))


@pytest.mark.parametrize("make", [identical_tris, lambda: identical_tris(300), empty_side_field, signed_zero_tris, big_leaf_soup],
                         ids=["identical", "identical300", "empty_side", "signed_zero", "overlapping"])
def test_edge_inputs_through_the_device(make):
    check_build(make())


def test_deep_tree_is_byte_equal():
    from snail_amd import HostBVH
    tv = deep_line()
    assert HostBVH.build_fast(tv).depth >= 56
    check_build(tv)


_lancia = {}


def lancia_scene():
    if not _lancia:
        from snail_amd import survey_camera
        tv = fixture("lancia")
        sc = dev_scene(tv)
        hb = sc.bvh
        _lancia.update(tv=tv, sc=sc, cam=survey_camera(tv), osc=O.OracleScene.from_arrays(hb.tris, hb.nodes, hb.depth, hb.perm))
    return _lancia


def frame_of(sc, cam, stream=None):
    stats = sc.new_stats()
    f = sc.trace_primary(cam, 256, 256, stats=stats, stream=stream)
    return f, stats


def assert_frame_is_oracle(f, stats, osc, cam, mode):
    import torch
    torch.cuda.synchronize()
    t, u, v, tid, ost = osc.render_primary(cam.as_array13(), 256, 256, mode=mode, threads=4)
    for a, b, n in ((f.t, t, "t"), (f.u, u, "u"), (f.v, v, "v"), (f.tri_id, tid, "triId")):
        assert np.array_equal(a.cpu().numpy().view(np.uint32), b.view(np.uint32)), n
    assert np.array_equal(stats.cpu().numpy().astype(np.uint64), ost), "TreeStats"


@pytest.mark.parametrize("arith,mode", [("ieee", O.MODE_IEEE), ("host_sse", O.MODE_SSE)])
def test_primary_frame_equals_the_oracle_over_the_downloaded_tree(arith, mode):
    L = lancia_scene()
    L["sc"].set_arith(arith)
    try:
        f, st = frame_of(L["sc"], L["cam"])
        assert_frame_is_oracle(f, st, L["osc"], L["cam"], mode)
    finally:
        L["sc"].set_arith("ieee")


ARITH = [("ieee", O.MODE_IEEE), ("host_sse", O.MODE_SSE)]


@pytest.mark.parametrize("arith,mode", ARITH)
def test_one_shadow_light_equals_the_oracle_over_the_downloaded_tree(arith, mode):
    """shadow packets towards one light each (Scene::TraceLight's form) and the lit frame of ONE light (primary + shadow stage)"""
    import torch
    L = lancia_scene()
    sc, osc, cam = L["sc"], L["osc"], L["cam"]
    sc.set_arith(arith)
    try:
        npk = 16
        origin, dirs, idir, dist = U.shadow_packets(osc, npk, seed=5, size=64)
        want = dist.copy()
        wst = osc.trace_shadow(origin, dirs, idir, want, npk, 64, mode=mode)
        got = dist.copy()
        st = sc.trace_shadow_host(origin, dirs, idir, got, npk, 64)
        U.assert_bit_equal(got, want, "shadow distance")
        st = np.asarray(st).astype(np.uint64)
        assert st[0] == wst[0] and st[1] == wst[1] and st[3] == wst[3], (st, wst)      # intersects, iters, skips (rays are counted by the caller)
        assert (np.isneginf(want) & ~np.isneginf(dist)).any() and (~np.isneginf(want)).any()      # occluded and lit rays both occur
        nd = osc.nodes[0]
        c, e = (nd["bmin"] + nd["bmax"]) * np.float32(0.5), nd["bmax"] - nd["bmin"]
        lights = np.array([[c[0], c[1] + 0.35 * e[1], c[2], 1.0, 0.9, 0.8, 2.0 * float(e.max())]], np.float32)
        wimg, wst = osc.render_whitted(cam.as_array13(), 256, 256, lights, mode=mode, threads=4)
        stats = sc.new_stats()
        img = sc.render_whitted(cam, 256, 256, lights, stats=stats).cpu().numpy()
        torch.cuda.synchronize()
        assert np.array_equal(img, wimg), int((img != wimg).sum())
        assert np.array_equal(stats.cpu().numpy().astype(np.uint64), wst), "TreeStats"
    finally:
        sc.set_arith("ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("shared", [True, False], ids=["shared_origin", "per_ray_origins"])
def test_a_generic_packet_batch_equals_the_oracle_over_the_downloaded_tree(arith, mode, shared):
    L = lancia_scene()
    sc, osc, cam = L["sc"], L["osc"], L["cam"]
    sc.set_arith(arith)
    try:
        npk = 16
        origin, dirs, idir, mask, dist, obj, bary = U.secondary_packets(osc, cam, 256, 256, npk, seed=21, shared=shared, masked=not shared, size=64)
        d2, o2, b2 = dist.copy(), obj.copy(), bary.copy()
        wst = osc.trace_rays(origin, dirs, idir, mask, d2, o2, b2, npk, 64, shared, mode=mode)
        d3, o3, b3 = dist.copy(), obj.copy(), bary.copy()
        st = sc.trace_rays_host(origin, dirs, idir, mask, d3, o3, b3, npk, 64, shared)
        U.assert_bit_equal(d3, d2, "t"); U.assert_bit_equal(o3, o2, "triId"); U.assert_bit_equal(b3, b2, "barycentric")
        st = np.asarray(st).astype(np.uint64)
        assert st[0] == wst[0] and st[1] == wst[1], (st, wst)
        assert (o2 != 0).any() and wst[0] > 0
    finally:
        sc.set_arith("ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
def test_instanced_frame_over_a_device_built_blas_equals_the_restatement(arith, mode):
    """one instanced frame whose BLAS is a from_fast_dev scene (and a second, host-built BLAS next to it) against tests/dbvh_ref.py over
    the downloaded tree; then the BLAS is rebuilt under the live instances, snail_instances_rebuild_dev follows as the header asks, and
    the next frame equals the restatement over the rebuilt tree"""
    import torch
    from snail_amd import HostBVH, scenes, survey_camera
    from snail_amd.instances import InstancedScene
    from snail_amd.scene import Scene
    tv = fixture("lancia")
    fast = dev_scene(tv)
    box_tv = fixture("box")
    box = Scene(HostBVH.build(box_tv), 0)
    oracles = lambda: [O.OracleScene.from_arrays(fast.bvh.tris, fast.bvh.nodes, fast.bvh.depth, fast.bvh.perm), O.OracleScene(box_tv)]
    osc = oracles()
    lo = np.minimum(osc[0].nodes[0]["bmin"], osc[1].nodes[0]["bmin"])
    hi = np.maximum(osc[0].nodes[0]["bmax"], osc[1].nodes[0]["bmax"])
    rot, tr, bi = scenes.instance_field(lo, hi, 12, seed=3, n_blas=2)
    tr = (tr * np.float32(0.1)).astype(np.float32)
    isc = InstancedScene([fast, box], rot, tr, bi)

    def check(osc):
        xs, bs = isc.slot_transforms()
        ref = D.Ref(osc, isc.nodes(), xs, bs)
        nd = isc.nodes()[0]
        cam = survey_camera(np.concatenate([nd["bmin"], nd["bmax"], nd["bmin"]]).reshape(1, 9))
        st = isc.new_stats()
        t, u, v, inst, tri = isc.trace_primary(cam, 96, 64, stats=st)
        rt, ru, rv, rinst, rtri, rst = ref.render_primary(cam.as_array13(), 96, 64, mode=mode)
        torch.cuda.synchronize()
        for a, b, what in ((t, rt, "t"), (u, ru, "u"), (v, rv, "v")):
            U.assert_bit_equal(a.cpu().numpy(), b, what)
        assert np.array_equal(inst.cpu().numpy(), rinst) and np.array_equal(tri.cpu().numpy(), rtri)
        assert np.array_equal(st.cpu().numpy().astype(np.uint64), rst), (st.cpu().numpy(), rst)
        hit = np.isfinite(rt)
        assert hit.sum() > 20 and (np.asarray(bs)[rinst[hit]] == 0).any()      # the device-built BLAS is hit

    for s in isc.blas:
        s.set_arith(arith)
    try:
        check(osc)
        info = fast.rebuild_fast_dev(torch.from_numpy(displaced(tv, 3) * np.float32(1.5)).cuda())      # (the root box changes)
        from snail_amd.instances import _xf12
        _, info2 = isc.update_dev(torch.from_numpy(_xf12(rot, tr)).cuda(), torch.from_numpy(np.ascontiguousarray(bi, np.int32)).cuda())
        torch.cuda.synchronize()
        assert info.cpu().numpy()[0] == 0 and info2.cpu().numpy()[0] == 0
        check(oracles())
    finally:
        for s in isc.blas:
            s.set_arith("ieee")
    fast.close(); box.close()


def displaced(tv, k):
    rng = np.random.default_rng(40 + k)
    return (tv + rng.uniform(-0.01, 0.01, tv.shape) * np.abs(tv).max()).astype(np.float32)


@pytest.mark.parametrize("two_streams", [False, True], ids=["one_stream", "two_streams"])
def test_rebuild_is_ordered_against_frames_without_host_waits(two_streams):
    import torch
    from snail_amd import survey_camera
    tv0 = fixture("lancia")
    tv1 = displaced(tv0, 1)
    cam = survey_camera(tv0)
    fresh = []
    for tv in (tv0, tv1):
        sc = dev_scene(tv)
        f, st = frame_of(sc, cam)
        torch.cuda.synchronize()
        fresh.append([x.cpu().numpy() for x in (f.t, f.u, f.v, f.tri_id, st)])
        sc.close()
    d0, d1 = (torch.from_numpy(tv).cuda() for tv in (tv0, tv1))
    sc = dev_scene(tv0)
    s1 = torch.cuda.Stream()
    s2 = torch.cuda.Stream() if two_streams else s1
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):      # (the frames' planes and counters are allocated and filled on the stream that traces into them)
        fa, sa = frame_of(sc, cam, stream=s1)
    with torch.cuda.stream(s2):
        info = sc.rebuild_fast_dev(d1, stream=s2)
    with torch.cuda.stream(s1):
        fb, sb = frame_of(sc, cam, stream=s1)
    torch.cuda.synchronize()
    assert info.cpu().numpy()[0] == 0
    for f, st, want in ((fa, sa, fresh[0]), (fb, sb, fresh[1])):
        for a, b in zip((f.t, f.u, f.v, f.tri_id, st), want):
            assert np.array_equal(a.cpu().numpy().view(np.uint8), b.view(np.uint8))
    sc.close()


def test_rebuild_refuses_what_it_must_and_keeps_the_tree():
    import torch
    from snail_amd import _lib, survey_camera
    tv = soup(1000, 77)
    cam = survey_camera(tv)
    sc = dev_scene(tv)
    f0, s0 = frame_of(sc, cam)
    torch.cuda.synchronize()
    before = [x.cpu().numpy().copy() for x in (f0.t, f0.tri_id, s0)]
    nodes0 = sc.bvh.nodes.tobytes()
    # another triangle count: a host-side error, nothing enqueued
    d_less = torch.from_numpy(tv[:999].copy()).cuda()
    info = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.SnailError):
        sc.rebuild_fast_dev(d_less, info=info)
    torch.cuda.synchronize()
    assert info.cpu().numpy().tolist() == [7, 7, 7, 7]
    # a NaN vertex: status 1, the previous tree stays
    bad = tv.copy()
    bad[501, 4] = np.nan
    info = sc.rebuild_fast_dev(torch.from_numpy(bad).cuda())
    f1, s1 = frame_of(sc, cam)
    torch.cuda.synchronize()
    assert info.cpu().numpy().tolist() == [1, 0, 0, 1000]
    for a, b in zip((f1.t, f1.tri_id, s1), before):
        assert np.array_equal(a.cpu().numpy().view(np.uint8), b.view(np.uint8))
    assert sc.bvh.nodes.tobytes() == nodes0
    # ... and a good rebuild afterwards takes
    tv2 = displaced(tv, 2)
    from snail_amd import HostBVH
    info = sc.rebuild_fast_dev(torch.from_numpy(tv2).cuda())
    hb = HostBVH.build_fast(tv2)
    assert sc.bvh.nodes.tobytes() == hb.nodes.tobytes() and sc.bvh.tris.tobytes() == hb.tris.tobytes() and np.array_equal(sc.perm, hb.perm)
    assert info.cpu().numpy().tolist() == [0, len(hb.nodes), hb.depth, 1000] and sc.depth == hb.depth
    sc.close()


# ---- depth: chains of 272 shrinking triangles, 50 / 63 / 64 / 65 levels deep (tests/test_bvh_fast_host.py: CHAINS) ----
def raw_create(tv):
    """snail_scene_create_fast_dev itself -> (handle or None, d_info as a list)"""
    import torch
    from snail_amd import _lib
    d = torch.from_numpy(np.ascontiguousarray(tv, np.float32)).cuda()
    perm = torch.full((len(tv),), -7, dtype=torch.int32, device="cuda")
    info = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    h = _lib.lib().snail_scene_create_fast_dev(_lib.ptr(d), len(tv), 0, _lib.ptr(perm), _lib.ptr(info), None)
    torch.cuda.synchronize()
    return h, info.cpu().numpy().tolist(), perm.cpu().numpy()


def test_a_chain_deeper_than_the_limit_is_status_2_and_no_handle():
    from snail_amd import _lib
    from tests.test_bvh_fast_host import raw_build_fast
    tv = CHAINS[65]()
    assert raw_build_fast(tv)[0] == 2          # the host builder agrees
    h, info, perm = raw_create(tv)
    assert not h and info == [2, 0, 0, len(tv)] and (perm == -7).all()
    assert "deeper" in _lib.lib().snail_last_error().decode()
    with pytest.raises(_lib.SnailError):
        dev_scene(tv)
    check_build(CHAINS[64]())                    # ... and the device is fine afterwards: one level less builds, byte-equal


@pytest.mark.parametrize("depth", [63, 64])
def test_chains_at_the_depth_limit_build_and_trace(depth):
    import torch
    from snail_amd import survey_camera
    tv = CHAINS[depth]()
    check_build(tv)
    sc = dev_scene(tv)
    assert sc.depth == depth
    cam = survey_camera(tv)
    osc = O.OracleScene.from_arrays(sc.bvh.tris, sc.bvh.nodes, sc.bvh.depth, sc.bvh.perm)
    f, st = frame_of(sc, cam)
    assert_frame_is_oracle(f, st, osc, cam, O.MODE_IEEE)
    sc.close()


def frame_bytes(sc, cam):
    import torch
    f, st = frame_of(sc, cam)
    torch.cuda.synchronize()
    return [x.cpu().numpy().tobytes() for x in (f.t, f.u, f.v, f.tri_id, st)]


@pytest.mark.parametrize("created,refused,taken", [(50, (63, 64, 65), 50), (64, (65,), 63)], ids=["shallow_handle", "deep_handle"])
def test_rebuild_too_deep_is_status_2_and_keeps_the_tree(created, refused, taken):
    """A handle created 50 levels deep traverses with the shallow stack: a rebuild deeper than 62 levels is status 2 although the tree
    would be legal; one created 64 deep takes 63 and 64 and refuses 65.  Either way the previous tree stays, frames equal the frame
    before, and a rebuild that fits takes afterwards."""
    import torch
    from snail_amd import HostBVH, survey_camera
    tv = CHAINS[created]()
    cam = survey_camera(CHAINS[50]())
    sc = dev_scene(tv)
    nodes0, tris0, perm0 = sc.bvh.nodes.tobytes(), sc.bvh.tris.tobytes(), sc.perm.copy()
    before = frame_bytes(sc, cam)
    for d in refused:
        info = sc.rebuild_fast_dev(torch.from_numpy(CHAINS[d]()).cuda())
        after = frame_bytes(sc, cam)
        assert info.cpu().numpy().tolist() == [2, 0, 0, len(tv)], d
        assert after == before, d
        assert sc.bvh.nodes.tobytes() == nodes0 and sc.bvh.tris.tobytes() == tris0 and np.array_equal(sc.perm, perm0) and sc.depth == created
    tv2 = CHAINS[taken]() if taken != created else displaced(tv, 4)
    info = sc.rebuild_fast_dev(torch.from_numpy(tv2).cuda())
    hb = HostBVH.build_fast(tv2)
    assert sc.bvh.nodes.tobytes() == hb.nodes.tobytes() and sc.bvh.tris.tobytes() == hb.tris.tobytes() and np.array_equal(sc.perm, hb.perm)
    assert info.cpu().numpy().tolist() == [0, len(hb.nodes), hb.depth, len(tv)]
    fresh = dev_scene(tv2)
    assert frame_bytes(sc, cam) == frame_bytes(fresh, cam)
    fresh.close(); sc.close()


def test_rebuild_outside_the_fast_arithmetics_range_is_status_3_on_a_fastok_handle_only():
    """status 3 (include/snail_bvh_fast.h): a handle created over records the fast arithmetic paths accept refuses a rebuild with a
    zero-area triangle and keeps its tree; a handle created WITH such a triangle takes any finite mesh"""
    import torch
    from snail_amd import HostBVH, survey_camera
    tv = soup(300, 91)
    flat = tv.copy()
    flat[17, 3:6] = flat[17, 0:3]; flat[17, 6:9] = flat[17, 0:3]
    cam = survey_camera(tv)
    sc = dev_scene(tv)
    nodes0 = sc.bvh.nodes.tobytes()
    before = frame_bytes(sc, cam)
    info = sc.rebuild_fast_dev(torch.from_numpy(flat).cuda())
    after = frame_bytes(sc, cam)
    assert info.cpu().numpy().tolist() == [3, 0, 0, 300]
    assert after == before and sc.bvh.nodes.tobytes() == nodes0
    sc.close()
    sc = dev_scene(flat)
    info = sc.rebuild_fast_dev(torch.from_numpy(tv).cuda())
    info2 = sc.rebuild_fast_dev(torch.from_numpy(flat).cuda())
    hb = HostBVH.build_fast(flat)
    assert info.cpu().numpy()[0] == 0 and info2.cpu().numpy().tolist() == [0, len(hb.nodes), hb.depth, 300]
    assert sc.bvh.nodes.tobytes() == hb.nodes.tobytes() and sc.bvh.tris.tobytes() == hb.tris.tobytes()
    osc = O.OracleScene.from_arrays(sc.bvh.tris, sc.bvh.nodes, sc.bvh.depth, sc.bvh.perm)
    f, st = frame_of(sc, cam)
    assert_frame_is_oracle(f, st, osc, cam, O.MODE_IEEE)
    sc.close()
