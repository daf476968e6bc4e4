"""Per-packet TreeStats and the gVals[5] heat-map under full shading on the MI355X (include/snail_materials_heatmap.h), word for word and byte for
byte against the restatement (tests/materials_heat_ref.py) on `room` (tests/materials_tree_cases.py) in both arithmetics: the counters with and
without the bounce and under the depth cut, their sum against d_stats and against the lit frame's stats; a shuffled list with a duplicate; the
heat bytes of every store (packets, 4x AA, tint, tile planes, a pitched frame); slicing under a level budget of one output packet; an opaque set
at two depths; and the lit frames around a heat launch.  What `room` must exercise is asserted without a GPU by tests/test_materials_heat_host.py."""
import numpy as np
import pytest

from snail_amd import materials as P
from tests import materials_heat_ref as MH
from tests import materials_tree_cases as K
from tests import oracle_lib as O
from tests.test_gpu_materials_synth import dev
from tests.test_gpu_materials_tree import TILES, room_set, scattered, shuffled

pytestmark = pytest.mark.gpu
ARITH = [("ieee", O.MODE_IEEE), ("host_sse", O.MODE_SSE)]
REFL, AA = P.RENDER_REFLECTIONS, P.RENDER_AA4
FILL = 0x5A


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def words(t):
    """an int32 device tensor of uint32 counters -> uint64 numpy"""
    return t.cpu().numpy().view(np.uint32).astype(np.uint64)


def same_words(what, got, want):
    bad = np.argwhere(got != want)
    print("%s: %d differing words of %d; sum %s" % (what, len(bad), got.size, got.reshape(-1, 4).sum(axis=0).tolist()))
    assert got.shape == want.shape and len(bad) == 0, (what, bad[:5].tolist(), got.reshape(-1, 4)[:3].tolist(), want.reshape(-1, 4)[:3].tolist())


def same_bytes(what, got, want):
    bad = np.argwhere(got != want)
    print("%s: %d differing bytes of %d, %d distinct colours" % (what, len(bad), got.size, len(np.unique(want.reshape(-1, 3), axis=0))))
    assert got.shape == want.shape and len(bad) == 0 and want.any(), (what, len(bad), bad[:5].tolist())


# ---- 1. counters ----
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("resx,resy", K.FRAMES)
def test_packet_counters_equal_the_restatement(torch_mod, resx, resy, arith, mode):
    """D = 8 with and without the bounce, D = 2 under the cut: every word; their sum is d_stats and the lit frame's stats, the counter the lit frame's"""
    torch = torch_mod
    c, sc, ms = room_set()
    ref = MH.room_ref()
    xy = K.frame_packets(resx, resy)
    dxy = dev(torch, xy)
    cam13 = c["cam"].as_array13()
    sc.set_arith(arith)
    try:
        for refl, depth in ((True, 8), (False, 8), (True, 2)):
            flags = REFL if refl else 0
            want, wtrunc = ref.packet_stats(cam13, resx, resy, xy, c["lights"], flags, mode, depth)
            st, fst = sc.new_stats(), sc.new_stats()
            got, tr = ms.packet_stats(c["cam"], resx, resy, None, c["lights"], reflections=refl, stats=st, max_depth=depth)      # the frame's own grid
            _, ftr = ms.tree_frame_packets(c["cam"], resx, resy, dxy, c["lights"], flags=flags, stats=fst, max_depth=depth)
            got, st, fst = words(got), st.cpu().numpy().astype(np.uint64), fst.cpu().numpy().astype(np.uint64)
            same_words("counters %dx%d %s refl=%d D=%d" % (resx, resy, arith, refl, depth), got, want)
            print("   d_stats %s, the lit frame's %s; truncated %d / %d / %d" % (st.tolist(), fst.tolist(), int(tr[0]), int(ftr[0]), wtrunc))
            assert np.array_equal(got.sum(axis=0), st) and np.array_equal(st, fst)
            assert int(tr.cpu().numpy()[0]) == wtrunc == int(ftr.cpu().numpy()[0]) and (wtrunc > 0) == (depth == 2)
    finally:
        sc.set_arith("ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
def test_a_shuffled_list_with_a_duplicate(torch_mod, arith, mode):
    """every entry carries its own packet's counters, the packet listed twice in both places; eight lights, some culled per packet"""
    torch = torch_mod
    c, sc, ms = room_set()
    resx, resy = K.FRAMES[1]
    xy = shuffled(resx, resy)
    from tests import materials_transparency_cases as TK
    L = TK.lights_of(c, "eight")
    sc.set_arith(arith)
    try:
        st = sc.new_stats()
        got, tr = ms.packet_stats(c["cam"], resx, resy, dev(torch, xy), L, reflections=True, stats=st)
        want, wtrunc = MH.room_ref().packet_stats(c["cam"].as_array13(), resx, resy, xy, L, REFL, mode, 8)
        got = words(got)
        same_words("shuffled %s" % arith, got, want)
        assert len(np.unique(want, axis=0)) >= 3 and np.array_equal(xy[-1], xy[1]) and np.array_equal(got[-1], got[1])
        assert np.array_equal(got.sum(axis=0), st.cpu().numpy().astype(np.uint64)) and int(tr.cpu().numpy()[0]) == wtrunc == 0
    finally:
        sc.set_arith("ieee")


# ---- 2. bytes ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_heat_bytes_of_packets(torch_mod, arith, mode):
    """plain packets, 4x AA with the [n][4][4] counters, and both with a tint"""
    torch = torch_mod
    c, sc, ms = room_set()
    ref = MH.room_ref()
    resx, resy = K.FRAMES[1]
    xy = shuffled(resx, resy)
    dxy = dev(torch, xy)
    cam13 = c["cam"].as_array13()
    sc.set_arith(arith)
    try:
        for flags in (REFL, REFL | AA, AA):
            for tint in (None, K.TINT):
                q = 4 if flags & AA else 1
                ps = torch.full((len(xy), q, 4), -1, dtype=torch.int32, device="cuda:0")
                st = sc.new_stats()
                got, tr = ms.render_heat_packets(c["cam"], resx, resy, dxy, c["lights"], flags=flags, tint=tint, packet_stats=ps, stats=st)
                want, wps, wtrunc = ref.heat_packets(cam13, resx, resy, xy, c["lights"], flags, tint, mode, 8)
                what = "heat packets %s flags=%d tint=%s" % (arith, flags, tint is not None)
                same_words(what, words(ps).reshape(wps.shape), wps)
                same_bytes(what, got.cpu().numpy(), want)
                assert np.array_equal(wps.reshape(-1, 4).sum(axis=0), st.cpu().numpy().astype(np.uint64)) and int(tr.cpu().numpy()[0]) == wtrunc == 0
                if tint is None:
                    assert len(np.unique(want.reshape(-1, 3), axis=0)) >= 3
    finally:
        sc.set_arith("ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
def test_heat_tiles_and_the_pitched_frame(torch_mod, arith, mode):
    c, sc, ms = room_set()
    ref = MH.room_ref()
    resx, resy = K.FRAMES[0]
    cam13 = c["cam"].as_array13()
    off, total, inside = scattered(TILES)
    sc.set_arith(arith)
    try:
        for flags, tint in ((REFL, None), (REFL | AA, K.TINT)):
            data = np.full(total, FILL, dtype=np.uint8)
            _, _, st, tr = ms.render_heat_tiles_host(c["cam"], resx, resy, TILES, off, c["lights"], flags=flags, tint=tint, data=data)
            want, wst, wtrunc = ref.heat_tiles(cam13, resx, resy, TILES, c["lights"], flags, tint, mode, 8)
            for k, (x, y, w, h) in enumerate(TILES.tolist()):
                bad = np.flatnonzero(data[off[k]:off[k] + 3 * w * h] != want[k])
                assert len(bad) == 0, ("tile", k, flags, len(bad), bad[:5].tolist())
            print("heat tiles %s flags=%d: stats %s / %s" % (arith, flags, st.tolist(), wst.tolist()))
            assert np.concatenate(want).any() and (data[~inside] == FILL).all() and np.array_equal(st, wst) and tr[0] == wtrunc == 0
        for resx, resy in K.FRAMES:
            pitch = 3 * resx + 5
            for flags, depth in ((REFL, 8), (REFL | AA, 2)):
                img, st, tr = ms.render_heat_frame_host(c["cam"], resx, resy, c["lights"], flags=flags, pitch=pitch, fill=FILL, max_depth=depth)
                want, wst, wtrunc = ref.heat_frame(cam13, resx, resy, c["lights"], flags, mode, depth)
                assert img.shape == (resy, pitch) and (img[:, 3 * resx:] == FILL).all()
                same_bytes("heat frame %dx%d %s flags=%d D=%d" % (resx, resy, arith, flags, depth), img[:, :3 * resx].reshape(resy, resx, 3), want)
                assert np.array_equal(st, wst) and int(tr[0]) == wtrunc and (wtrunc > 0) == (depth == 2), (st, wst, tr, wtrunc)
    finally:
        sc.set_arith("ieee")


# ---- 3. slicing ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_slices_of_one_output_packet_change_nothing(torch_mod, arith, mode):
    """a level budget of ONE output packet's bytes: 7 slices, each booking at its packets' place in the whole list's array"""
    torch = torch_mod
    c, sc, ms = room_set()
    resx, resy = K.FRAMES[0]
    dxy = dev(torch, shuffled(resx, resy))
    sc.set_arith(arith)
    try:
        for flags in (REFL, REFL | AA):
            q = 4 if flags & AA else 1
            runs = []
            for budget in (1 << 40, P.MaterialSet.level_bytes(len(c["lights"]), flags, 8)):
                ms.set_level_budget(budget)
                ps = torch.full((len(dxy), q, 4), -1, dtype=torch.int32, device="cuda:0")
                st = sc.new_stats()
                got, tr = ms.render_heat_packets(c["cam"], resx, resy, dxy, c["lights"], flags=flags, tint=K.TINT, packet_stats=ps, stats=st)
                runs.append((got.cpu().numpy(), words(ps), st.cpu().numpy(), int(tr.cpu().numpy()[0])))
            a, b = runs
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3] == 0 and a[0].any() and a[1].any()
    finally:
        ms.set_level_budget(1 << 30)
        sc.set_arith("ieee")


# ---- 4. an opaque set ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_an_opaque_set_counts_the_same_at_every_depth(torch_mod, arith, mode):
    torch = torch_mod
    c, sc, ms = room_set(opaque=True)
    assert not ms.can_select_transparent
    resx, resy = K.FRAMES[1]
    xy = K.frame_packets(resx, resy)
    dxy = dev(torch, xy)
    sc.set_arith(arith)
    try:
        got = {}
        for depth in (1, 8):
            ps, tr = ms.packet_stats(c["cam"], resx, resy, dxy, c["lights"], reflections=True, max_depth=depth)
            got[depth] = words(ps)
            assert int(tr.cpu().numpy()[0]) == 0
        want, _ = MH.room_ref(opaque=True).packet_stats(c["cam"].as_array13(), resx, resy, xy, c["lights"], REFL, mode, 8)
        same_words("opaque %s" % arith, got[8], want)
        assert np.array_equal(got[1], got[8]) and got[8].any()
    finally:
        sc.set_arith("ieee")


# ---- 5. the lit frames around a heat launch ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_a_heat_launch_leaves_the_lit_frames_alone(torch_mod, arith, mode):
    """tree_frame_packets before and after a heat launch on the same set: identical bytes and stats (eight launches in between: every group of
    intermediates has served a heat launch)"""
    torch = torch_mod
    c, sc, ms = room_set()
    resx, resy = K.FRAMES[0]
    dxy = dev(torch, shuffled(resx, resy))
    sc.set_arith(arith)
    try:
        s0, s1 = sc.new_stats(), sc.new_stats()
        a, ta = ms.tree_frame_packets(c["cam"], resx, resy, dxy, c["lights"], flags=REFL | AA, tint=K.TINT, stats=s0)
        a = a.cpu().numpy()
        for k in range(8):
            ms.render_heat_packets(c["cam"], resx, resy, dxy, c["lights"], flags=(REFL | AA) if k & 1 else REFL, tint=K.TINT if k & 2 else None)
        b, tb = ms.tree_frame_packets(c["cam"], resx, resy, dxy, c["lights"], flags=REFL | AA, tint=K.TINT, stats=s1)
        assert np.array_equal(a, b.cpu().numpy()) and a.any() and np.array_equal(s0.cpu().numpy(), s1.cpu().numpy())
        assert int(ta.cpu().numpy()[0]) == int(tb.cpu().numpy()[0]) == 0
    finally:
        sc.set_arith("ieee")
