"""The transparency continuation together with the mirrored bounce, tiles, 4x AA and the tint on the MI355X (include/snail_materials_tree.h),
bit for bit against the restatement (tests/materials_tree_ref.py) on `room` (tests/materials_tree_cases.py) in both arithmetics: the new stage
k_mat_mirror_rays on level-1 packets; the packet form for every flag combination, depth, light list and frame size over a shuffled packet list
with a duplicate; tile lists and the image form; the header's equivalences against the older functions, device against device; slicing under a
small level budget; two frames back to back on one stream; and the older entry points' refusal of the set.  What `room` must exercise is
asserted without a GPU by tests/test_materials_tree_host.py."""
import numpy as np
import pytest

from snail_amd import HostBVH, _lib
from snail_amd import materials as P
from snail_amd.scene import Scene
from tests import materials_tree_cases as K
from tests import materials_tree_ref as TR
from tests import materials_transparency_cases as TK
from tests import oracle_lib as O
from tests.test_gpu_materials_synth import dev
from tests.test_gpu_materials_transparency import product_materials

pytestmark = pytest.mark.gpu
ARITH = [("ieee", O.MODE_IEEE), ("host_sse", O.MODE_SSE)]
REFL, DEPTH, AA = P.RENDER_REFLECTIONS, P.RENDER_DEPTH, P.RENDER_AA4
FILL = 0x5A
_sets = {}


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def room_set(opaque=False):
    """(case, Scene, MaterialSet of the new creator) of `room`, or of `room` with opaque stand-ins; built once"""
    if opaque not in _sets:
        c = K.room()
        hb = HostBVH.build(c["tv"])
        assert np.array_equal(hb.perm, c["osc"].perm) and hb.nodes.tobytes() == c["osc"].nodes.tobytes()
        sc = Scene(hb, 0)
        mats = []
        for d in c["descs"]:
            if opaque and d[0] == "transp":
                d = ("tex", d[1], d[3])
            elif opaque and d[0] == "uber" and 0.0 < d[3] < 1.0:
                d = ("uber", d[1], d[2], 0.0)
            mats += product_materials([d])
        ms = P.MaterialSet(sc, c["uv"], c["nrm"], c["mat_index"], c["flat"], c["material_map"], mats, [P.Texture(t) for t in c["textures"]], transparent=True)
        _sets[opaque] = (c, sc, ms)
    return _sets[opaque]


def shuffled(resx, resy):
    """the frame's packets in a shuffled order, one of them twice"""
    xy = K.frame_packets(resx, resy)
    pick = np.random.RandomState(11).permutation(len(xy))
    return np.ascontiguousarray(np.concatenate([xy[pick], xy[pick[1:2]]]))


def check_packets(what, got, want, st, wst, trunc, wtrunc):
    bad = np.argwhere(got != want)
    print("%s: %d differing bytes; stats %s / %s; truncated %d / %d" % (what, len(bad), np.asarray(st).tolist(), np.asarray(wst).tolist(), int(trunc), int(wtrunc)))
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist())
    assert np.array_equal(np.asarray(st).astype(np.uint64), np.asarray(wst).astype(np.uint64)), (what, st, wst)
    assert int(trunc) == int(wtrunc), (what, trunc, wtrunc)


# ---- 1. the stage ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_mirror_rays_stage(torch_mod, arith, mode):
    """k_mat_mirror_rays on the level-1 packets of `room` (96 x 64: 24 packets): every output plane, the zeros and SafeInv(0) of masked lanes, the
    order words under an input order list with skipped packets -- whose outputs keep what they were filled with -- and the stats word"""
    torch = torch_mod
    c, sc, ms = room_set()
    resx, resy = K.STAGE_FRAME
    fr = TR.TreeFrames(K.room_tr())
    lvl, smp = TR.generic_level(fr, c["cam"].as_array13(), resx, resy, K.frame_packets(resx, resy), mode)
    want = TR.mirror_level(fr, smp, mode)
    n = len(lvl["order"])
    part = lvl["order"] >= 0
    assert 4 <= part.sum() < n                                     # packets that are part of level 1, and packets that are not
    sel = want["distance"] == np.float32(np.inf)
    assert sel[part].any() and (~sel[part]).any() and (sel[part].reshape(-1, 256).sum(axis=1) == 0).any()       # hit lanes, masked lanes, an all-miss packet
    sc.set_arith(arith)
    try:
        out = tuple(torch.full(s, FILL, dtype=t, device="cuda:0") for s, t in (((n, 64, 3, 4), torch.float32),) * 3 + (((n, 64), torch.uint8), ((n, 256), torch.float32),
                                                                                                                    ((n, 256), torch.int32), ((n,), torch.int32)))
        st = sc.new_stats()
        ms.mirror_rays(dev(torch, lvl["origin"]), dev(torch, lvl["dir"]), dev(torch, lvl["mask"]), dev(torch, lvl["t"]), dev(torch, lvl["samples"]),
                       dev(torch, lvl["order"]), out=out, stats=st)
        got = [a.cpu().numpy() for a in out]
        st = st.cpu().numpy()
        # without an order list every packet is mirrored
        free = ms.mirror_rays(dev(torch, lvl["origin"]), dev(torch, lvl["dir"]), dev(torch, lvl["mask"]), dev(torch, lvl["t"]), dev(torch, lvl["samples"]))
        free = [a.cpu().numpy() for a in free]
    finally:
        sc.set_arith("ieee")
    keys = ("origin", "dir", "idir", "mask", "distance", "object")
    filled = [np.full_like(g, FILL) for g in got]
    for k, g, f, fr_ in zip(keys, got, filled, free):
        w = want[k]
        bad = int((np.ascontiguousarray(g[part]).view(np.uint8) != np.ascontiguousarray(w[part]).view(np.uint8)).sum())
        kept = int((np.ascontiguousarray(g[~part]).view(np.uint8) != np.ascontiguousarray(f[~part]).view(np.uint8)).sum())
        print("mirror_rays %s %s: %d differing bytes in the level's packets, %d bytes written in skipped packets" % (arith, k, bad, kept))
        assert bad == 0 and kept == 0, (k, bad, kept)
        assert np.ascontiguousarray(fr_).view(np.uint8).tobytes() == np.ascontiguousarray(w).view(np.uint8).tobytes(), k
    assert np.array_equal(got[6], np.where(part, np.arange(n), -1)) and np.array_equal(free[6], np.arange(n))
    assert int(st[2]) == int(sel[part].sum()) and not st[[0, 1, 3]].any(), (st, int(sel[part].sum()))
    # masked lanes: zeros in origin and dir, SafeInv(0) in idir
    off = ~sel[part].reshape(-1, 64, 1, 4).repeat(3, axis=2)
    assert off.any() and not got[0][part][off].any() and not got[1][part][off].any() and len(np.unique(got[2][part][off].view(np.uint32))) == 1


# ---- 2. frames ----
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("lights", ["case", "none", "eight"])
@pytest.mark.parametrize("resx,resy", K.FRAMES)
def test_tree_frame_packets_equal_the_restatement(torch_mod, resx, resy, lights, arith, mode):
    torch = torch_mod
    c, sc, ms = room_set()
    L = TK.lights_of(c, lights)
    xy = shuffled(resx, resy)
    dxy = dev(torch, xy)
    cam13 = c["cam"].as_array13()
    moved = 0
    sc.set_arith(arith)
    try:
        for depth in (1, 2, 8):
            ref = K.tiles_ref(depth)
            for flags in (REFL, REFL | AA, AA, 0):
                for tint in (None, K.TINT):
                    st = sc.new_stats()
                    got, tr = ms.tree_frame_packets(c["cam"], resx, resy, dxy, L, flags=flags, tint=tint, stats=st, max_depth=depth)
                    want, wst = ref.packets(cam13, resx, resy, xy, L, flags, tint, mode=mode)
                    check_packets("room %dx%d lights=%s %s D=%d flags=%d tint=%s" % (resx, resy, lights, arith, depth, flags, tint is not None), got.cpu().numpy(), want,
                                  st.cpu().numpy(), wst, tr.cpu().numpy()[0], ref.truncated)
                    assert want.any()
                    moved += ref.truncated > 0
                    if depth == 8:
                        assert ref.truncated == 0
    finally:
        sc.set_arith("ieee")
    assert moved >= 8                                              # the cut at D = 1 and D = 2 moved the counter under every flag combination


# ---- 3. tiles and the image form ----
TILES = np.array([(0, 0, 16, 64), (16, 0, 16, 64), (32, 0, 16, 64), (5, 3, 21, 13)], dtype=np.int32)      # 16 x 64 tiles cross the 48 x 32 image's lower edge; an odd one


def scattered(tiles):
    size = 3 * tiles[:, 2].astype(np.int64) * tiles[:, 3]
    order = [2, 0, 3, 1]
    off = np.zeros(len(tiles), dtype=np.int64)
    at = 7
    for k in order:
        off[k] = at
        at += int(size[k]) + 13
    inside = np.zeros(at, dtype=bool)
    for k in range(len(tiles)):
        inside[off[k]:off[k] + size[k]] = True
    return off, at, inside


@pytest.mark.parametrize("arith,mode", ARITH)
def test_tree_tiles_and_image_form(torch_mod, arith, mode):
    c, sc, ms = room_set()
    resx, resy = K.FRAMES[0]
    cam13 = c["cam"].as_array13()
    off, total, inside = scattered(TILES)
    ref = K.tiles_ref(8)
    sc.set_arith(arith)
    try:
        for flags, tint in ((REFL, None), (REFL | AA, K.TINT), (DEPTH | AA, None)):
            data = np.full(total, FILL, dtype=np.uint8)
            got, goff, st, tr = ms.render_tree_tiles_host(c["cam"], resx, resy, TILES, off, c["lights"], flags=flags, tint=tint, data=data, max_depth=8)
            want, wst = ref.tiles(cam13, resx, resy, TILES, c["lights"], flags, tint, mode=mode)
            for k, (x, y, w, h) in enumerate(TILES.tolist()):
                g = data[off[k]:off[k] + 3 * w * h]
                bad = np.flatnonzero(g != want[k])
                assert len(bad) == 0, ("tile", k, flags, len(bad), bad[:5].tolist())
            assert np.concatenate(want).any() and (data[~inside] == FILL).all() and np.array_equal(st, wst) and tr[0] == 0, (flags, st, wst, tr)
        pitch = 3 * resx + 5
        for flags in (REFL, REFL | AA):
            img, st, tr = ms.render_tree_frame_host(c["cam"], resx, resy, c["lights"], flags=flags, pitch=pitch, fill=FILL, max_depth=2)
            r2 = K.tiles_ref(2)
            want, wst = r2.frame(cam13, resx, resy, c["lights"], flags, mode=mode)
            assert img.shape == (resy, pitch) and (img[:, 3 * resx:] == FILL).all()
            bad = np.argwhere((img[:, :3 * resx].reshape(resy, resx, 3) != want).any(axis=2))
            assert want.any() and len(bad) == 0, (flags, len(bad), bad[:5].tolist())
            assert np.array_equal(st, wst) and int(tr[0]) == r2.truncated > 0, (flags, st, wst, tr, r2.truncated)
    finally:
        sc.set_arith("ieee")


# ---- 4. the header's equivalences, device against device ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_equivalence_a_flags_0_is_the_transparent_packets(torch_mod, arith, mode):
    torch = torch_mod
    c, sc, ms = room_set()
    resx, resy = K.FRAMES[1]
    dxy = dev(torch, shuffled(resx, resy))
    sc.set_arith(arith)
    try:
        for depth in (1, 2, 8):
            s1, s2 = sc.new_stats(), sc.new_stats()
            a, ta = ms.tree_frame_packets(c["cam"], resx, resy, dxy, c["lights"], stats=s1, max_depth=depth)
            b, tb = ms.render_transparent_packets(c["cam"], resx, resy, dxy, c["lights"], stats=s2, max_depth=depth)
            check_packets("(a) D=%d %s" % (depth, arith), a.cpu().numpy(), b.cpu().numpy(), s1.cpu().numpy(), s2.cpu().numpy(), ta.cpu().numpy()[0], tb.cpu().numpy()[0])
            assert b.cpu().numpy().any()
    finally:
        sc.set_arith("ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
def test_equivalence_b_an_opaque_set_is_the_tile_renderer(torch_mod, arith, mode):
    torch = torch_mod
    c, sc, ms = room_set(opaque=True)
    assert not ms.can_select_transparent
    resx, resy = K.FRAMES[1]
    dxy = dev(torch, shuffled(resx, resy))
    off, total, inside = scattered(TILES)
    sc.set_arith(arith)
    try:
        for depth in (1, 8):
            for flags in (0, REFL, AA, REFL | AA, DEPTH):
                for tint in (None, K.TINT):
                    s1, s2 = sc.new_stats(), sc.new_stats()
                    a, ta = ms.tree_frame_packets(c["cam"], resx, resy, dxy, c["lights"], flags=flags, tint=tint, stats=s1, max_depth=depth)
                    b = ms.frame_packets(c["cam"], resx, resy, dxy, c["lights"], flags=flags, tint=tint, stats=s2)
                    check_packets("(b) packets D=%d flags=%d tint=%s %s" % (depth, flags, tint is not None, arith), a.cpu().numpy(), b.cpu().numpy(), s1.cpu().numpy(),
                                  s2.cpu().numpy(), ta.cpu().numpy()[0], 0)
            for flags, tint in ((REFL, None), (REFL | AA, K.TINT)):
                ga = ms.render_tree_tiles_host(c["cam"], 48, 32, TILES, off, c["lights"], flags=flags, tint=tint, data=np.full(total, FILL, np.uint8), max_depth=depth)
                gb = ms.render_tiles_host(c["cam"], 48, 32, TILES, off, c["lights"], flags=flags, tint=tint, data=np.full(total, FILL, np.uint8))
                assert np.array_equal(ga[0], gb[0]) and np.array_equal(ga[2], gb[2]) and ga[3][0] == 0 and (ga[0] != FILL).any()
            for flags in (REFL, AA):
                ia = ms.render_tree_frame_host(c["cam"], resx, resy, c["lights"], flags=flags, max_depth=depth)
                ib = ms.render_frame_host(c["cam"], resx, resy, c["lights"], flags=flags)
                assert np.array_equal(ia[0], ib[0]) and np.array_equal(ia[1], ib[1]) and ia[2][0] == 0 and ia[0].any()
    finally:
        sc.set_arith("ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
def test_equivalence_c_depth_is_the_scene_s_tile_renderer(torch_mod, arith, mode):
    c, sc, ms = room_set()
    tiles = np.array([(0, 0, 16, 32), (16, 0, 16, 32), (8, 8, 20, 24), (40, 3, 3, 5)], dtype=np.int32)       # (snail_render_tiles does not clip to the image)
    sc.set_arith(arith)
    try:
        for flags in (DEPTH, DEPTH | AA, DEPTH | AA | REFL):
            got, off, st, tr = ms.render_tree_tiles_host(c["cam"], 48, 32, tiles, lights7=c["lights"], flags=flags, max_depth=3)
            want, woff, wst = sc.render_tiles_host(c["cam"], 48, 32, tiles, c["lights"], flags=flags, color=(1.0, 1.0, 1.0))
            assert np.array_equal(off, woff) and want.any() and np.array_equal(got, want) and np.array_equal(st, wst) and tr[0] == 0, (flags, st, wst, tr)
    finally:
        sc.set_arith("ieee")


# ---- 5. slicing ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_slices_change_nothing(torch_mod, arith, mode):
    """a budget of 2 and of 4 output packets' worth on 6 packets + 1 (the last slice partial), with and without AA: bytes, stats and the counter of
    the unsliced run; and after calls at depth 8 on every group of intermediates, calls at depth 2 allocate nothing"""
    torch = torch_mod
    c, sc, ms = room_set()
    resx, resy = K.FRAMES[0]
    dxy = dev(torch, shuffled(resx, resy))
    assert len(dxy) == 7
    sc.set_arith(arith)
    try:
        for flags in (REFL, REFL | AA):
            for depth in (8, 2):
                one = P.MaterialSet.level_bytes(len(c["lights"]), flags, depth)
                ms.set_level_budget(1 << 40)
                s0 = sc.new_stats()
                want, t0 = ms.tree_frame_packets(c["cam"], resx, resy, dxy, c["lights"], flags=flags, tint=K.TINT, stats=s0, max_depth=depth)
                for budget in (2 * one, 4 * one + 1, 1):
                    ms.set_level_budget(budget)
                    s1 = sc.new_stats()
                    got, t1 = ms.tree_frame_packets(c["cam"], resx, resy, dxy, c["lights"], flags=flags, tint=K.TINT, stats=s1, max_depth=depth)
                    check_packets("slices flags=%d D=%d budget=%d %s" % (flags, depth, budget, arith), got.cpu().numpy(), want.cpu().numpy(), s1.cpu().numpy(),
                                  s0.cpu().numpy(), t1.cpu().numpy()[0], t0.cpu().numpy()[0])
                assert want.cpu().numpy().any() and (depth == 8 or int(t0.cpu().numpy()[0]) > 0)
        ms.set_level_budget(1 << 40)
        for _ in range(8):                                         # every one of the set's eight groups of intermediates has run depth 8 with the bounce and AA
            ms.tree_frame_packets(c["cam"], resx, resy, dxy, c["lights"], flags=REFL | AA, max_depth=8)
        torch.cuda.synchronize()
        free = torch.cuda.mem_get_info()[0]
        for _ in range(8):
            ms.tree_frame_packets(c["cam"], resx, resy, dxy, c["lights"], flags=REFL | AA, max_depth=2)
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == free
    finally:
        ms.set_level_budget(1 << 30)
        sc.set_arith("ieee")


# ---- 6. stream order ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_two_frames_back_to_back_on_one_stream(torch_mod, arith, mode):
    torch = torch_mod
    c, sc, ms = room_set()
    resx, resy = K.FRAMES[0]
    xy = K.frame_packets(resx, resy)
    dxy = dev(torch, xy)
    stream = torch.cuda.Stream()
    sc.set_arith(arith)
    try:
        with torch.cuda.stream(stream):
            s8, s2 = sc.new_stats(), sc.new_stats()
            stream.synchronize()
            a, ta = ms.tree_frame_packets(c["cam"], resx, resy, dxy, c["lights"], flags=REFL, stats=s8, stream=stream, max_depth=8)
            b, tb = ms.tree_frame_packets(c["cam"], resx, resy, dxy, c["lights"], flags=REFL, stats=s2, stream=stream, max_depth=2)
        stream.synchronize()
    finally:
        sc.set_arith("ieee")
    for depth, g, st, tr in ((8, a, s8, ta), (2, b, s2, tb)):
        ref = K.tiles_ref(depth)
        want, wst = ref.packets(c["cam"].as_array13(), resx, resy, xy, c["lights"], REFL, None, mode=mode)
        check_packets("back to back D=%d %s" % (depth, arith), g.cpu().numpy(), want, st.cpu().numpy(), wst, tr.cpu().numpy()[0], ref.truncated)


# ---- 7. the older entry points ----
def test_the_older_functions_still_refuse_the_room_set(torch_mod):
    torch = torch_mod
    c, sc, ms = room_set()
    assert ms.can_select_transparent
    dxy = dev(torch, K.frame_packets(48, 32))
    for name, call in (("snail_materials_frame_packets_dev", lambda: ms.frame_packets(c["cam"], 48, 32, dxy, flags=REFL)),
                       ("snail_materials_render_tiles", lambda: ms.render_tiles_host(c["cam"], 48, 32, TILES)),
                       ("snail_materials_render_frame", lambda: ms.render_frame_host(c["cam"], 48, 32, flags=AA)),
                       ("snail_materials_bounce_packets_dev", lambda: ms.render_packets(c["cam"], 48, 32, dxy, reflections=True)),
                       ("snail_render_materials_packets_dev", lambda: ms.render_packets(c["cam"], 48, 32, dxy))):
        with pytest.raises(_lib.SnailError) as e:
            call()
        assert name in str(e.value) and "transparent" in str(e.value), (name, str(e.value))
    with pytest.raises(_lib.SnailError) as e:
        ms.render_transparent_packets(c["cam"], 48, 32, dxy, flags=REFL)
    assert "flags" in str(e.value)
