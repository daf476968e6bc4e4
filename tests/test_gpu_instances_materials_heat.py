"""Per-packet TreeStats and the gVals[5] heat-map under full shading of instanced scenes on the MI355X
(include/snail_instances_materials_heatmap.h; InstancedMaterialSet.packet_stats / .render_heat_packets / .render_heat_tiles_host /
.render_heat_frame_host), in both arithmetics.  Every comparison is for equality -- of counter words, of bytes, of the four TreeStats and of the
truncated-lane counter; nothing here takes a tolerance.  The expected counters are the restatement's (tests/instances_materials_heat_ref.py: one
RayTrace call per packet, memoised and shared by the tests of this module) on the cases of tests/instances_materials_tree_cases.py at their
shapes (FRAME 96x64, AA_FRAME 48x32, TILE_FRAME 88x56); what those cases exercise is asserted without a GPU by
tests/test_instances_materials_heat_host.py.  The lit frames of include/snail_instances_materials_tree.h, whose kernels this header's launches
leave unchanged, are the second yardstick: the counters' sum and the truncated counter are theirs.

The restatement runs at GPU_DEPTH (maxDepth 2) in test_counters_equal_the_restatement, test_an_explicit_shuffled_list,
test_heat_bytes_of_packets and test_a_heat_launch_an_update_and_a_heat_launch_on_one_stream: at depth 8 the CPU side would take minutes.
test_the_deep_case runs it at CUT_DEPTH, 2 and 8 (its tree is small).  The tile, frame, slicing and opaque-set tests compare device launches with
each other.  Sets and scenes are built once per module (those of tests/test_gpu_instances_materials_transparency.py, by import).  Nothing here
reads outside the repository, and nothing provokes a fault."""
import numpy as np
import pytest

from tests import dbvh_shade_ref as S
from tests import dbvh_tiles_ref as DT
from tests import instances_materials_heat_ref as MH
from tests import instances_materials_transparency_cases as C
from tests import instances_materials_tree_cases as K
from tests import oracle_lib as O
from tests import test_gpu_instances_materials_transparency as G

pytestmark = pytest.mark.gpu
ARITH = [("ieee", O.MODE_IEEE), ("host_sse", O.MODE_SSE)]
REFL, AA4 = MH.REFLECTIONS, MH.AA4
device_set, set_arith, dev = G.device_set, G.set_arith, G.dev


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def word(t):
    return int(t.cpu().numpy()[0]) if hasattr(t, "cpu") else int(t[0])


def u64(t):
    return (t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)).astype(np.uint64)


def u32(t):
    """the counters of a device tensor (int32 holding uint32 words) as uint64"""
    return t.cpu().numpy().view(np.uint32).astype(np.uint64)


def counters(isc, ms, cam, frame, xy, lights, bounce, depth, torch):
    """packet_stats -> (counters uint64 [n, 4], d_stats uint64 [4], truncated)"""
    st = isc.new_stats()
    ps, tr = ms.packet_stats(cam, frame[0], frame[1], None if xy is None else dev(torch, xy), lights, bounce, stats=st, max_depth=depth)
    return u32(ps), u64(st), word(tr)


def lit(isc, ms, cam, frame, xy, lights, flags, depth, torch, tint=None):
    """the lit packets of the same arguments -> (bytes, stats, truncated)"""
    st = isc.new_stats()
    out, tr = ms.tree_frame_packets(cam, frame[0], frame[1], dev(torch, xy), lights, flags, tint, stats=st, max_depth=depth)
    return out.cpu().numpy(), u64(st), word(tr)


def heat(isc, ms, cam, frame, xy, lights, flags, depth, torch, tint=None, aa_counters=True):
    """render_heat_packets with the optional counters -> (bytes, counters uint64 [n, 4] or [n, 4, 4], stats, truncated)"""
    n = len(xy)
    st = isc.new_stats()
    ps = torch.full((n, 4, 4) if flags & AA4 else (n, 4), 0x55, dtype=torch.int32, device="cuda:0")
    out, tr = ms.render_heat_packets(cam, frame[0], frame[1], dev(torch, xy), lights, flags, tint, packet_stats=ps, stats=st, max_depth=depth)
    return out.cpu().numpy(), u32(ps), u64(st), word(tr)


def assert_counters(what, got, want, st, trunc, wtrunc):
    bad = np.argwhere((got != want).any(axis=-1))
    print("%s: %d of %d packets differ; sum %s, d_stats %s; truncated %d / %d" % (what, len(bad), got.reshape(-1, 4).shape[0], got.reshape(-1, 4).sum(axis=0).tolist(), st.tolist(),
                                                                                  trunc, wtrunc))
    assert got.shape == want.shape and len(bad) == 0, (what, bad[:5].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())
    assert np.array_equal(got.reshape(-1, 4).sum(axis=0), st), (what, st)
    assert trunc == wtrunc, (what, trunc, wtrunc)


# ---- 1. counters word for word on the frame's own grid ----
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("n_lights", [0, 2])
@pytest.mark.parametrize("bounce", [True, False])
@pytest.mark.parametrize("name", ["glasshouse", "moved"])
def test_counters_equal_the_restatement(torch_mod, name, bounce, n_lights, arith, mode):
    isc, ms = device_set(name)
    cam, frame, lights = K.camera(name), K.FRAME, K.lights_of(name, n_lights)
    xy = S.frame_packets(*frame)
    want, wtrunc = MH.case_ref(name).packet_stats(cam.as_array13(), frame[0], frame[1], xy, lights, REFL if bounce else 0, mode, K.GPU_DEPTH)
    set_arith(isc, arith)
    try:
        got, st, trunc = counters(isc, ms, cam, frame, None, lights, bounce, K.GPU_DEPTH, torch_mod)      # (no list: the frame's own grid)
        _, lst, ltrunc = lit(isc, ms, cam, frame, xy, lights, REFL if bounce else 0, K.GPU_DEPTH, torch_mod)
    finally:
        set_arith(isc, "ieee")
    assert_counters("%s, bounce %d, %d lights, %s" % (name, bounce, n_lights, arith), got, want, st, trunc, wtrunc)
    assert np.array_equal(st, lst) and trunc == ltrunc, (st, lst, trunc, ltrunc)
    assert len(np.unique(got, axis=0)) >= 3 and (got[:, 2] >= 256).all()


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("depth", [K.CUT_DEPTH, 2, 8])
def test_the_deep_case(torch_mod, depth, arith, mode):
    name = "deep"
    isc, ms = device_set(name)
    cam, frame, lights = K.camera(name), K.FRAME, K.lights_of(name, 1)
    xy = S.frame_packets(*frame)
    want, wtrunc = MH.case_ref(name).packet_stats(cam.as_array13(), frame[0], frame[1], xy, lights, REFL, mode, depth)
    set_arith(isc, arith)
    try:
        got, st, trunc = counters(isc, ms, cam, frame, None, lights, True, depth, torch_mod)
        _, lst, ltrunc = lit(isc, ms, cam, frame, xy, lights, REFL, depth, torch_mod)
    finally:
        set_arith(isc, "ieee")
    assert_counters("deep, maxDepth %d, %s" % (depth, arith), got, want, st, trunc, wtrunc)
    assert np.array_equal(st, lst) and trunc == ltrunc and (trunc > 0) == (depth == K.CUT_DEPTH)


# ---- 2. an explicit list ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_an_explicit_shuffled_list(torch_mod, arith, mode):
    """a packet listed twice, two packets outside the 96x64 frame, eight lights: every entry carries its own packet's counters"""
    name = "moved"
    isc, ms = device_set(name)
    cam, frame, lights = K.camera(name), K.FRAME, K.lights_of(name, 8)
    xy = np.array(((32, 16), (80, 48), (32, 16), (96, 0), (0, 64), (16, 32), (0, 0)), dtype=np.int32)
    want, wtrunc = MH.case_ref(name).packet_stats(cam.as_array13(), frame[0], frame[1], xy, lights, REFL, mode, K.GPU_DEPTH)
    set_arith(isc, arith)
    try:
        got, st, trunc = counters(isc, ms, cam, frame, xy, lights, True, K.GPU_DEPTH, torch_mod)
        _, lst, ltrunc = lit(isc, ms, cam, frame, xy, lights, REFL, K.GPU_DEPTH, torch_mod)
    finally:
        set_arith(isc, "ieee")
    assert_counters("packet list, %s" % arith, got, want, st, trunc, wtrunc)
    assert np.array_equal(got[0], got[2]) and not np.array_equal(got[0], got[1])
    assert np.array_equal(st, lst) and trunc == ltrunc


# ---- 3. heat bytes of packets ----
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("flags", [REFL, REFL | AA4, AA4])
def test_heat_bytes_of_packets(torch_mod, flags, arith, mode):
    """with and without the tint; the optional counters ([n][4][4] with AA4) are the restatement's, the bytes its colours"""
    name = "moved"
    isc, ms = device_set(name)
    cam, frame, lights = K.camera(name), K.AA_FRAME, K.lights_of(name, 2)
    xy = S.frame_packets(*frame)
    ref = MH.case_ref(name)
    set_arith(isc, arith)
    try:
        for tint in (None, K.TINT):
            want, wps, wtrunc = ref.heat_packets(cam.as_array13(), frame[0], frame[1], xy, lights, flags, tint, mode, K.GPU_DEPTH)
            got, ps, st, trunc = heat(isc, ms, cam, frame, xy, lights, flags, K.GPU_DEPTH, torch_mod, tint)
            assert_counters("heat counters, flags %d tint %s, %s" % (flags, tint, arith), ps, wps, st, trunc, wtrunc)
            bad = (got != want).any(axis=2)
            print("heat bytes, flags %d tint %s, %s: %d differing pixels of %d, %d colours" % (flags, tint, arith, int(bad.sum()), bad.size, len(np.unique(got.reshape(-1, 3), axis=0))))
            assert not bad.any(), np.argwhere(bad)[:5].tolist()
            assert len(np.unique(got.reshape(-1, 3), axis=0)) >= 3
            # ... and without the optional counters: the set's own array, the same bytes
            out, _ = ms.render_heat_packets(cam, frame[0], frame[1], dev(torch_mod, xy), lights, flags, tint, max_depth=K.GPU_DEPTH)
            assert np.array_equal(out.cpu().numpy(), got)
    finally:
        set_arith(isc, "ieee")


# ---- 4. tile planes and the pitched frame ----
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("key,flags,tint", [("column", REFL, None), ("right_edge", REFL | AA4, None), ("rect", REFL | AA4, K.TINT), ("shared_packet", REFL, K.TINT)])
def test_tiles_equal_the_packet_form_through_the_planar_store(torch_mod, key, flags, tint, arith, mode):
    """without a tint the packet form's bytes come from k_heat_store and the tiles' from k_heat_colours + k_inst_store: the header promises them equal"""
    name = "moved"
    isc, ms = device_set(name)
    cam, (resx, resy) = K.camera(name), K.TILE_FRAME
    tiles = np.array(K.TILE_LISTS[key], dtype=np.int32)
    lights = K.lights_of(name, 2)
    size = 3 * tiles[:, 2].astype(np.int64) * tiles[:, 3]
    offsets = (np.concatenate([[0], np.cumsum(size + 11)[:-1]]) + 5).astype(np.int64)          # gaps before, between and after the tiles
    data = np.full(int((offsets + size).max()) + 9, 0xa5, dtype=np.uint8)
    set_arith(isc, arith)
    try:
        pk, _, pst, ptr = heat(isc, ms, cam, (resx, resy), DT.tile_packets(tiles), lights, flags, K.GPU_DEPTH, torch_mod, tint)
        data, _, st, trunc = ms.render_heat_tiles_host(cam, resx, resy, tiles, offsets, lights, flags, tint, data=data, max_depth=K.GPU_DEPTH, truncated=np.full(1, 3, dtype=np.uint64))
    finally:
        set_arith(isc, "ieee")
    covered = np.zeros(len(data), dtype=bool)
    k = 0
    for (x, y, w, h), off in zip(tiles.tolist(), offsets.tolist()):
        n = ((w + 15) // 16) * ((h + 15) // 16)
        want = DT.planar_from_packets(pk[k:k + n], w, h, resx - x, resy - y)
        k += n
        assert np.array_equal(data[off:off + 3 * w * h], want), (key, x, y, w, h)
        covered[off:off + 3 * w * h] = True
        if x + w > resx:      # beyond the image: zero in all three planes
            assert not data[off:off + 3 * w * h].reshape(3, h, w)[:, :, resx - x:].any() and want.any()
    assert (data[~covered] == 0xa5).all() and (~covered).sum() >= 14
    assert np.array_equal(u64(st), pst) and int(trunc[0]) == 3 + ptr


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("flags", [REFL, REFL | AA4])
def test_the_pitched_frame_equals_the_packet_form(torch_mod, flags, arith, mode):
    name = "moved"
    isc, ms = device_set(name)
    cam, (resx, resy) = K.camera(name), K.TILE_FRAME
    xy = S.frame_packets(resx, resy)
    lights = K.lights_of(name, 2)
    set_arith(isc, arith)
    try:
        pk, _, pst, ptr = heat(isc, ms, cam, (resx, resy), xy, lights, flags, K.GPU_DEPTH, torch_mod)
        img, ist, itr = ms.render_heat_frame_host(cam, resx, resy, lights, flags, pitch=resx * 3 + 20, fill=0x5a, max_depth=K.GPU_DEPTH, truncated=np.full(1, 7, dtype=np.uint64))
    finally:
        set_arith(isc, "ieee")
    want = S.packets_to_frame(xy, pk, resx, resy)
    assert np.array_equal(img[:, :resx * 3].reshape(resy, resx, 3), want) and (img[:, resx * 3:] == 0x5a).all() and want.any()
    assert np.array_equal(u64(ist), pst) and int(itr[0]) == 7 + ptr


# ---- 5. slicing ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_slicing_changes_nothing(torch_mod, arith, mode):
    """a level budget of ONE output packet's level_bytes on AA_FRAME with REFL | AA4: 6 slices of 4 sub-packets, each booking at its own place"""
    name = "glasshouse"
    isc, ms = device_set(name)
    frame, flags = K.AA_FRAME, REFL | AA4
    xy = S.frame_packets(*frame)
    lights = K.lights_of(name, 2)
    one = ms.level_bytes(2, flags, K.GPU_DEPTH)
    assert one > 0 and len(xy) == 6
    set_arith(isc, arith)
    try:
        whole = heat(isc, ms, K.camera(name), frame, xy, lights, flags, K.GPU_DEPTH, torch_mod, K.TINT)
        ms.set_level_budget(one)
        try:
            sliced = heat(isc, ms, K.camera(name), frame, xy, lights, flags, K.GPU_DEPTH, torch_mod, K.TINT)
            plain = heat(isc, ms, K.camera(name), frame, xy, lights, flags, K.GPU_DEPTH, torch_mod)      # (k_heat_store after the last slice)
        finally:
            ms.set_level_budget(1 << 30)
        plain_whole = heat(isc, ms, K.camera(name), frame, xy, lights, flags, K.GPU_DEPTH, torch_mod)
    finally:
        set_arith(isc, "ieee")
    for what, a, b in (("tinted", sliced, whole), ("plain", plain, plain_whole)):
        assert_counters("one output packet per slice, %s, %s" % (what, arith), a[1], b[1], a[2], a[3], b[3])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and a[0].any()
    assert whole[1].shape == (6, 4, 4) and len(np.unique(whole[1].reshape(-1, 4), axis=0)) >= 3


# ---- 6. an opaque set; nothing is left behind ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_an_opaque_set_and_the_lit_frames_around_a_heat_launch(torch_mod, arith, mode):
    isc, ms = device_set("glasshouse", True, True, False)
    assert ms.can_select_transparent is False
    cam, frame = K.camera("glasshouse"), K.FRAME
    xy = S.frame_packets(*frame)
    lights = K.lights_of("glasshouse", 2)
    set_arith(isc, arith)
    try:
        before = lit(isc, ms, cam, frame, xy, lights, REFL, 2, torch_mod)
        d1 = counters(isc, ms, cam, frame, xy, lights, True, 1, torch_mod)
        d8 = counters(isc, ms, cam, frame, xy, lights, True, 8, torch_mod)
        hb = heat(isc, ms, cam, frame, xy, lights, REFL, 2, torch_mod, K.TINT)
        after = lit(isc, ms, cam, frame, xy, lights, REFL, 2, torch_mod)
    finally:
        set_arith(isc, "ieee")
    assert_counters("an opaque set at maxDepth 1 and 8, %s" % arith, d1[0], d8[0], d1[1], d1[2], 0)
    assert np.array_equal(d1[1], d8[1]) and d8[2] == 0 and np.array_equal(hb[1], d1[0])
    assert np.array_equal(d1[1], before[1])                                 # the lit frame's TreeStats
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2] == after[2] == 0 and before[0].any()


# ---- 7. ordering against updates ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_a_heat_launch_an_update_and_a_heat_launch_on_one_stream(torch_mod, arith, mode):
    torch = torch_mod
    u = C.case("moved")
    isc, ms = G.new_set("glasshouse")                                 # (a handle of this test's own: the cached one keeps its transforms)
    cam, frame = K.camera("moved"), K.FRAME
    xy = S.frame_packets(*frame)
    lights = K.lights_of("moved", 2)
    want, wtrunc = MH.case_ref("moved").packet_stats(cam.as_array13(), frame[0], frame[1], xy, lights, REFL, mode, K.GPU_DEPTH)
    xf = np.concatenate([np.asarray(u["rot"]).reshape(-1, 9), np.asarray(u["tr"]).reshape(-1, 3)], axis=1).astype(np.float32)
    set_arith(isc, arith)
    try:
        d_xy, d_xf, d_bi = dev(torch, xy), dev(torch, xf), dev(torch, np.ascontiguousarray(u["bi"], dtype=np.int32))
        sa, sb = isc.new_stats(), isc.new_stats()
        first, t0 = ms.packet_stats(cam, frame[0], frame[1], d_xy, lights, True, stats=sa, max_depth=K.GPU_DEPTH)
        isc.update_dev(d_xf, d_bi)
        second, t1 = ms.packet_stats(cam, frame[0], frame[1], d_xy, lights, True, stats=sb, max_depth=K.GPU_DEPTH)
        first, second = u32(first), u32(second)
    finally:
        set_arith(isc, "ieee")
        ms.close()
        isc.close()
    assert_counters("after the update, %s" % arith, second, want, u64(sb), word(t1), wtrunc)
    assert (first != second).any(axis=1).sum() >= 3 and not np.array_equal(u64(sa), u64(sb))
