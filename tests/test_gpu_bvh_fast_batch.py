"""The fast builder over several handles in one batched pass (snail_scenes_rebuild_fast_dev, include/snail_bvh_fast_batch.h;
snail_amd.scene.rebuild_fast_dev_batch): every handle of a batch ends byte-equal -- nodes, triangle records, perm, info words -- to
snail_bvh_build_fast on the host and to snail_scene_rebuild_fast_dev on a handle of its own; the commit rule and the refusals are per entry;
a batch is ordered against frames without host waits.

Sizes: 4 | 5 and 64 | 65 are the builder's size classes (root leaf | root onto the small list | big levels), 255 | 256 | 257 put the boundary
between two entries inside, at the end of and right after a 256-thread workgroup of the boxes and commit kernels; 16 | 17 entries are the
table full and two passes."""
import ctypes as C

import numpy as np
import pytest

from snail_amd import _lib
from tests.test_bvh_fast_host import CHAINS, big_leaf_soup, deep_line, empty_side_field, identical_tris, signed_zero_tris, soup
from tests.test_gpu_bvh_fast import dev_scene, displaced, frame_of

pytestmark = pytest.mark.gpu
SIZES = (1, 4, 5, 64, 65, 255, 256, 257, 1000, 5003)


def dev(tv):
    import torch
    return torch.from_numpy(np.ascontiguousarray(tv, np.float32)).cuda()


def batch(scenes, tvs, stream=None):
    from snail_amd.scene import rebuild_fast_dev_batch
    d = [dev(tv) for tv in tvs]
    infos = rebuild_fast_dev_batch(scenes, d, stream=stream)
    return infos, d


_host = {}


def host(key, make):
    """HostBVH.build_fast of a pose, computed once"""
    if key not in _host:
        from snail_amd import HostBVH
        tv = make()
        _host[key] = (tv, HostBVH.build_fast(tv))
    return _host[key]


def state(sc):
    """what the handle holds now, read back from the device: (nodes, triangle records, perm, depth)"""
    sc._stale = True
    b = sc.bvh
    return b.nodes.tobytes(), b.tris.tobytes(), np.asarray(b.perm).astype(np.int32).tobytes(), b.depth


def host_state(hb):
    return hb.nodes.tobytes(), hb.tris.tobytes(), np.asarray(hb.perm).astype(np.int32).tobytes(), hb.depth


def rebuilds(sc):
    """the builds enqueued on the handle so far (the workbench library's read: test-only, in no header)"""
    fn = _lib.debug_lib().snail_scene_debug_rebuilds
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
    out = C.c_uint64(0)
    assert fn(sc._h, C.addressof(out)) == 0, _lib.debug_lib().snail_last_error()
    return out.value


def pose(n, which):
    return host(("soup", n, which), lambda: soup(n, (200 if which == "A" else 700) + n))


def check_against_host(scenes, infos, hosts, what):
    import torch
    torch.cuda.synchronize()
    for k, (sc, info, (tv, hb)) in enumerate(zip(scenes, infos, hosts)):
        assert info.cpu().numpy().tolist() == [0, len(hb.nodes), hb.depth, len(tv)], (what, k, len(tv), info.cpu().numpy().tolist())
        got, want = state(sc), host_state(hb)
        for part, a, b in zip(("nodes", "triangle records", "perm", "depth"), got, want):
            assert a == b, (what, "entry %d (%d triangles): %s" % (k, len(tv), part))
        assert sc.d_perm.cpu().numpy().tobytes() == want[2], (what, k)


# ---- 1. byte-equality ----
def test_a_batch_is_byte_equal_to_the_host_and_to_single_rebuilds():
    import torch
    scenes = [dev_scene(pose(n, "A")[0]) for n in SIZES]
    alone = [dev_scene(pose(n, "A")[0]) for n in SIZES]
    count0 = [rebuilds(s) for s in scenes]
    infos, keep = batch(scenes, [pose(n, "B")[0] for n in SIZES])
    single = [s.rebuild_fast_dev(d) for s, d in zip(alone, keep)]
    check_against_host(scenes, infos, [pose(n, "B") for n in SIZES], "one batch of ten")
    torch.cuda.synchronize()
    for n, a, b, ia, ib in zip(SIZES, scenes, alone, infos, single):
        assert state(a) == state(b), n
        assert ia.cpu().numpy().tolist() == ib.cpu().numpy().tolist(), n
    assert [rebuilds(s) for s in scenes] == [c + 1 for c in count0]
    assert any(pose(n, "A")[1].nodes.tobytes() != pose(n, "B")[1].nodes.tobytes() for n in SIZES)      # the poses' trees differ
    for s in scenes + alone:
        s.close()


# ---- 2. the table: 1 entry, 16 (full), 17 (two passes); ascending and descending sizes ----
MANY = (1, 2, 4, 5, 33, 64, 65, 66, 129, 255, 256, 257, 300, 512, 700, 1000, 1300)


@pytest.mark.parametrize("order", ["ascending", "descending"])
@pytest.mark.parametrize("count", [1, 16, 17])
def test_table_limits(count, order):
    sizes = MANY[-count:] if count == 1 else MANY[:count]
    if order == "descending":
        sizes = sizes[::-1]
    scenes = [dev_scene(pose(n, "A")[0]) for n in sizes]
    infos, keep = batch(scenes, [pose(n, "B")[0] for n in sizes])
    check_against_host(scenes, infos, [pose(n, "B") for n in sizes], "%d entries, %s" % (count, order))
    assert all(rebuilds(s) == 2 for s in scenes)       # creation and the batch
    for s in scenes:
        s.close()


# ---- 3. edge inputs in one batch ----
def test_edge_inputs_in_one_batch():
    """each handle is created over its mesh in REVERSED triangle order (the same triangles: the same arithmetic paths and a depth the handle
    takes) and rebuilt, all in one batch, to the mesh itself"""
    makes = [("identical", identical_tris), ("identical300", lambda: identical_tris(300)), ("empty_side", empty_side_field), ("signed_zero", signed_zero_tris),
             ("overlapping", big_leaf_soup), ("deep_line", deep_line)]
    hosts = [host(("edge", name), make) for name, make in makes]
    assert 56 <= hosts[-1][1].depth <= 62          # deep, and within what a handle created shallower takes
    scenes = [dev_scene(np.ascontiguousarray(tv[::-1])) for tv, _ in hosts]
    infos, keep = batch(scenes, [tv for tv, _ in hosts])
    check_against_host(scenes, infos, hosts, "edge inputs")
    for s in scenes:
        s.close()


# ---- 4. the commit rule is per entry ----
def flat_soup():
    tv = soup(300, 91).copy()
    tv[17, 3:6] = tv[17, 0:3]; tv[17, 6:9] = tv[17, 0:3]
    return tv


def refused_in_the_middle(created, new, status, others=(257, 65)):
    """three handles; the middle one, created over `created`, is rebuilt to `new` and must answer `status` and keep tree and perm; the outer
    two (soups) commit"""
    import torch
    outer = [dev_scene(pose(n, "A")[0]) for n in others]
    mid = dev_scene(created)
    scenes = [outer[0], mid, outer[1]]
    before = state(mid)
    perm0 = mid.d_perm.cpu().numpy().copy()
    infos, keep = batch(scenes, [pose(others[0], "B")[0], new, pose(others[1], "B")[0]])
    torch.cuda.synchronize()
    assert infos[1].cpu().numpy().tolist() == [status, 0, 0, len(created)], infos[1].cpu().numpy().tolist()
    assert state(mid) == before and np.array_equal(mid.d_perm.cpu().numpy(), perm0)
    check_against_host(outer, [infos[0], infos[2]], [pose(n, "B") for n in others], "beside status %d" % status)
    assert [rebuilds(s) for s in scenes] == [2, 2, 2]      # (a build that the device refuses was enqueued all the same)
    # ... and a good batch afterwards takes on all three
    tv2 = displaced(created, 6)
    infos, keep = batch(scenes, [pose(others[0], "A")[0], tv2, pose(others[1], "A")[0]])
    check_against_host(scenes, infos, [pose(others[0], "A"), host(("again", status), lambda: tv2), pose(others[1], "A")], "after status %d" % status)
    for s in scenes:
        s.close()


def test_status_1_leaves_its_handle_and_the_others_commit():
    tv = pose(1000, "A")[0]
    bad = tv.copy()
    bad[501, 4] = np.nan
    refused_in_the_middle(tv, bad, 1)


def test_status_2_leaves_its_handle_and_the_others_commit():
    """the inputs of test_rebuild_too_deep_is_status_2_and_keeps_the_tree: a handle created 50 levels deep refuses a chain of 63"""
    refused_in_the_middle(CHAINS[50](), CHAINS[63](), 2)


def test_status_3_on_the_fastok_handle_only():
    """a zero-area triangle: status 3 on the handle created over records the fast arithmetic paths accept, taken by the handle beside it that
    was created WITH such a triangle -- the same mesh, in the same batch"""
    import torch
    tv, flat = soup(300, 91), flat_soup()
    refused_in_the_middle(tv, flat, 3)
    ok, lax = dev_scene(tv), dev_scene(flat)
    assert ok.flags()[0] and not lax.flags()[0]
    before = state(ok)
    infos, keep = batch([ok, lax], [flat, tv])
    infos2, keep2 = batch([lax, ok], [flat, flat])
    torch.cuda.synchronize()
    assert infos[0].cpu().numpy().tolist() == [3, 0, 0, 300] and infos2[1].cpu().numpy().tolist() == [3, 0, 0, 300]
    assert state(ok) == before
    check_against_host([lax], [infos2[0]], [host(("flat",), flat_soup)], "the handle created without fastOK")
    ok.close(); lax.close()


# ---- 5. refusals: non-zero, the entry named, nothing enqueued ----
def test_refusals_name_the_entry_and_touch_nothing():
    import torch
    from snail_amd.scene import Scene, _FastRebuild
    L = _lib.lib()
    sizes = (300, 65, 1000)
    scenes = [dev_scene(pose(n, "A")[0]) for n in sizes]
    hostbuilt = Scene.from_fast(pose(65, "A")[0], 0)
    d = [dev(pose(n, "B")[0]) for n in sizes]
    infos = [torch.full((4,), 7, dtype=torch.int32, device="cuda") for _ in sizes]
    before = [state(s) for s in scenes]
    torch.cuda.synchronize()

    def listed():
        arr = (_FastRebuild * 3)()
        for k, s in enumerate(scenes):
            arr[k].scene, arr[k].d_verts9, arr[k].nTris = s._h, d[k].data_ptr(), sizes[k]
            arr[k].d_perm, arr[k].d_info = s.d_perm.data_ptr(), infos[k].data_ptr()
        return arr

    def null_handle(a):
        a[1].scene = None

    def null_verts(a):
        a[1].d_verts9 = None

    def other_kind(a):
        a[1].scene = hostbuilt._h

    def other_count(a):
        a[1].nTris = 64

    def twice(a):
        a[2].scene, a[2].d_verts9, a[2].nTris = a[0].scene, a[0].d_verts9, a[0].nTris

    for change, entry, text in ((null_handle, 1, "invalid scene handle"), (null_verts, 1, "null vertices"), (other_kind, 1, "not made by snail_scene_create_fast_dev"),
                                (other_count, 1, "64 triangles, the handle holds 65"), (twice, 2, "listed twice (entry 0)")):
        arr = listed()
        change(arr)
        rc = L.snail_scenes_rebuild_fast_dev(C.cast(arr, C.c_void_p), 3, None)
        err = L.snail_last_error().decode()
        assert rc != 0 and "snail_scenes_rebuild_fast_dev: entry %d:" % entry in err and text in err, (change.__name__, rc, err)
        torch.cuda.synchronize()
        assert [rebuilds(s) for s in scenes] == [1, 1, 1], change.__name__
        assert [state(s) for s in scenes] == before, change.__name__
        assert all(i.cpu().numpy().tolist() == [7, 7, 7, 7] for i in infos), change.__name__
    # the list as it stands is taken
    assert L.snail_scenes_rebuild_fast_dev(C.cast(listed(), C.c_void_p), 3, None) == 0, L.snail_last_error()
    check_against_host(scenes, infos, [pose(n, "B") for n in sizes], "after the refusals")
    assert [rebuilds(s) for s in scenes] == [2, 2, 2]
    # the binding's own checks
    from snail_amd.scene import rebuild_fast_dev_batch
    with pytest.raises(_lib.SnailError, match="scene 1 was not made by from_fast_dev"):
        rebuild_fast_dev_batch([scenes[0], hostbuilt], [d[0], d[1]])
    with pytest.raises(_lib.SnailError, match="entry 1: the handle is listed twice"):
        rebuild_fast_dev_batch([scenes[0], scenes[0]], [d[0], d[0]])
    hostbuilt.close()
    for s in scenes:
        s.close()


# ---- 6. ordering against frames, without host waits ----
ORDER_SIZES = (1000, 257, 64)
_twins = {}


def twin_frames(arith):
    """{pose: per size, the frame planes and TreeStats of a static scene built on the host from that pose}, once per arithmetic"""
    if arith not in _twins:
        import torch
        from snail_amd import survey_camera
        from snail_amd.scene import Scene
        out = {}
        for which in "AB":
            rows = []
            for n in ORDER_SIZES:
                sc = Scene.from_fast(pose(n, which)[0], 0)
                sc.set_arith(arith)
                f, st = frame_of(sc, survey_camera(pose(n, "A")[0]))
                torch.cuda.synchronize()
                rows.append([x.cpu().numpy().tobytes() for x in (f.t, f.u, f.v, f.tri_id, st)])
                sc.close()
            out[which] = rows
        _twins[arith] = out
    return _twins[arith]


@pytest.mark.parametrize("arith", ["ieee", "host_sse"])
@pytest.mark.parametrize("two_streams", [False, True], ids=["one_stream", "two_streams"])
def test_batches_are_ordered_against_frames_without_host_waits(two_streams, arith):
    import torch
    from snail_amd import survey_camera
    want = twin_frames(arith)
    for k, n in enumerate(ORDER_SIZES):
        assert want["A"][k] != want["B"][k], n          # the poses give different frames: the comparison below can tell them apart
    cams = [survey_camera(pose(n, "A")[0]) for n in ORDER_SIZES]
    scenes = [dev_scene(pose(n, "A")[0]) for n in ORDER_SIZES]
    for s in scenes:
        s.set_arith(arith)
    dA, dB = ([dev(pose(n, which)[0]) for n in ORDER_SIZES] for which in "AB")
    s1 = torch.cuda.Stream()
    s2 = torch.cuda.Stream() if two_streams else s1
    from snail_amd.scene import rebuild_fast_dev_batch
    torch.cuda.synchronize()
    frames, infos = [], []
    for step, verts in enumerate((dB, dA, None)):
        with torch.cuda.stream(s1):      # (the frames' planes and counters are allocated and filled on the stream that traces into them)
            frames.append([frame_of(sc, cam, stream=s1) for sc, cam in zip(scenes, cams)])
        if verts is not None:
            with torch.cuda.stream(s2):
                infos.append(rebuild_fast_dev_batch(scenes, verts, stream=s2))
    torch.cuda.synchronize()
    for row in infos:
        assert all(i.cpu().numpy()[0] == 0 for i in row)
    for step, which in enumerate("ABA"):
        for k, (f, st) in enumerate(frames[step]):
            got = [x.cpu().numpy().tobytes() for x in (f.t, f.u, f.v, f.tri_id, st)]
            assert got == want[which][k], ("frame %d (pose %s), %d triangles, %s" % (step, which, ORDER_SIZES[k], arith))
    for s in scenes:
        s.close()
