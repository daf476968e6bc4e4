"""The transparency continuation together with the mirrored bounce, tile lists, 4x antialiasing, depth shading and the tint under full shading
of instanced scenes on the MI355X (include/snail_instances_materials_tree.h; InstancedMaterialSet.mirror_rays / .tree_frame_packets /
.render_tree_tiles_host / .render_tree_frame_host / .set_level_budget / .level_bytes), in both arithmetics.  Every comparison is for equality of
bytes, of the four TreeStats and of the truncated-lane counter; nothing here takes a tolerance.  Against existing device functions, independent
of the new restatement: (a) flags 0 against the transparency frames, (b) an opaque set against the bounce frames, (c) depth shading against the
instanced scene's own tile renderer, (d) the image form against the packet form.  Against the restatement
(tests/instances_materials_tree_ref.py) on the cases of tests/instances_materials_tree_cases.py, which were chosen on the CPU; what they
exercise is asserted without a GPU by tests/test_instances_materials_tree_host.py, whose docstring has the truncated-lane figures: `glasshouse`
and `moved` are cut at maxDepth 2 (counter non-zero, equal to the restatement's) and whole at FULL_DEPTH (counter 0), `deep` is cut at maxDepth 1
alone.  Sets and scenes are built once per module (those of tests/test_gpu_instances_materials_transparency.py, by import).  Nothing here reads
outside the repository."""
import numpy as np
import pytest

from snail_amd import _lib
from tests import dbvh_shade_ref as S
from tests import dbvh_tiles_ref as DT
from tests import instances_materials_transparency_cases as C
from tests import instances_materials_tree_cases as K
from tests import instances_materials_tree_ref as R
from tests import oracle_lib as O
from tests import test_gpu_instances_materials_transparency as G

pytestmark = pytest.mark.gpu
ARITH = [("ieee", O.MODE_IEEE), ("host_sse", O.MODE_SSE)]
REFL, DEPTH, AA4 = R.REFLECTIONS, R.DEPTH, R.AA4
device_set, set_arith, dev = G.device_set, G.set_arith, G.dev


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def word(t):
    return int(t.cpu().numpy()[0]) if hasattr(t, "cpu") else int(t[0])


def np_stats(st):
    return (st.cpu().numpy() if hasattr(st, "cpu") else np.asarray(st)).astype(np.uint64)


def assert_packets(what, got, want, st, wst, trunc, wtrunc):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    bad = (got != np.asarray(want)).any(axis=2)
    print("%s: %d differing pixels of %d; stats %s / %s; truncated %d / %d" % (what, int(bad.sum()), bad.size, np_stats(st).tolist(), np_stats(wst).tolist(), trunc, wtrunc))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    assert np.array_equal(np_stats(st), np_stats(wst)), (what, np_stats(st), np_stats(wst))
    assert trunc == wtrunc, (what, trunc, wtrunc)


def tree_packets(isc, ms, cam, frame, xy, lights, flags, depth, tint=None, torch=None):
    st = isc.new_stats()
    out, trunc = ms.tree_frame_packets(cam, frame[0], frame[1], dev(torch, xy), lights, flags, tint, stats=st, max_depth=depth)
    return out.cpu().numpy(), np_stats(st), word(trunc)


# ---- against existing device functions ----
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("depth", [1, 4])
def test_a_flags_0_equals_the_transparency_frames(torch_mod, depth, arith, mode):
    torch = torch_mod
    isc, ms = device_set("glasshouse")
    cam, (resx, resy) = K.camera("glasshouse"), K.FRAME
    xy = dev(torch, S.frame_packets(resx, resy))
    lights = K.lights_of("glasshouse", 2)
    set_arith(isc, arith)
    try:
        sa, sb = isc.new_stats(), isc.new_stats()
        new, tn = ms.tree_frame_packets(cam, resx, resy, xy, lights, 0, stats=sa, max_depth=depth)
        old, to = ms.render_transparent_packets(cam, resx, resy, xy, lights, stats=sb, max_depth=depth)
        new, old = new.cpu().numpy(), old.cpu().numpy()
    finally:
        set_arith(isc, "ieee")
    assert_packets("(a) depth %d, %s" % (depth, arith), new, old, sa, sb, word(tn), word(to))
    assert old.any() and (depth != 1 or word(to) > 0)


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("depth", [1, 8])
def test_b_an_opaque_set_equals_the_bounce_frames(torch_mod, depth, arith, mode):
    torch = torch_mod
    isc, ms = device_set("glasshouse", True, True, False)
    assert ms.can_select_transparent is False
    cam, (resx, resy) = K.camera("glasshouse"), K.FRAME
    xy = dev(torch, S.frame_packets(resx, resy))
    lights = K.lights_of("glasshouse", 2)
    set_arith(isc, arith)
    try:
        for refl in (False, True):
            sa, sb = isc.new_stats(), isc.new_stats()
            new, tn = ms.tree_frame_packets(cam, resx, resy, xy, lights, REFL if refl else 0, stats=sa, max_depth=depth)
            old = ms.render_packets(cam, resx, resy, xy, lights, stats=sb, reflections=refl)
            assert_packets("(b) depth %d, reflections %d, %s" % (depth, refl, arith), new, old.cpu().numpy(), sa, sb, word(tn), 0)
    finally:
        set_arith(isc, "ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("flags,tint", [(DEPTH, None), (DEPTH | AA4, None), (DEPTH | REFL, K.TINT), (DEPTH | AA4, K.TINT)])
def test_c_depth_shading_equals_the_scene_s_own(torch_mod, flags, tint, arith, mode):
    torch = torch_mod
    isc, ms = device_set("moved")
    cam, (resx, resy) = K.camera("moved"), K.TILE_FRAME
    xy = dev(torch, S.frame_packets(resx, resy))
    tiles = K.TILE_LISTS["shared_packet"] + K.TILE_LISTS["right_edge"]
    set_arith(isc, arith)
    try:
        sa, sb = isc.new_stats(), isc.new_stats()
        trunc = torch.full((1,), 5, dtype=torch.int64, device="cuda:0")
        new, trunc = ms.tree_frame_packets(cam, resx, resy, xy, K.lights_of("moved", 2), flags, tint, stats=sa, max_depth=2, truncated=trunc)
        old = isc.shade_packets(cam, resx, resy, xy, None, flags, tint, stats=sb)
        assert_packets("(c) flags %d tint %s, %s" % (flags, tint, arith), new, old.cpu().numpy(), sa, sb, word(trunc), 5)
        ht = np.full(1, 9, dtype=np.uint64)
        data, off, st, ht = ms.render_tree_tiles_host(cam, resx, resy, tiles, None, K.lights_of("moved", 2), flags, tint, max_depth=2, truncated=ht)
        odata, ooff, ost = isc.render_tiles_host(cam, resx, resy, tiles, None, flags, tint)
    finally:
        set_arith(isc, "ieee")
    assert np.array_equal(data, odata) and np.array_equal(off, ooff) and np.array_equal(st, ost) and int(ht[0]) == 9 and data.any()


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("flags", [REFL, REFL | AA4])
def test_d_the_image_form_equals_the_packet_form(torch_mod, flags, arith, mode):
    torch = torch_mod
    isc, ms = device_set("moved")
    cam, (resx, resy) = K.camera("moved"), (70, 50)
    xy = S.frame_packets(resx, resy)
    lights = K.lights_of("moved", 2)
    set_arith(isc, arith)
    try:
        pk, pst, ptr = tree_packets(isc, ms, cam, (resx, resy), xy, lights, flags, 2, torch=torch)
        img, ist, itr = ms.render_tree_frame_host(cam, resx, resy, lights, flags, pitch=resx * 3 + 20, fill=0x5a, max_depth=2, truncated=np.full(1, 7, dtype=np.uint64))
    finally:
        set_arith(isc, "ieee")
    want = S.packets_to_frame(xy, pk, resx, resy)
    assert np.array_equal(img[:, :resx * 3].reshape(resy, resx, 3), want) and (img[:, resx * 3:] == 0x5a).all() and want.any()
    assert np.array_equal(np_stats(ist), pst) and int(itr[0]) == 7 + ptr


# ---- against the restatement ----
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("n_lights", [0, 2])
@pytest.mark.parametrize("name", ["glasshouse", "moved"])
def test_frames_with_reflections_equal_the_restatement(torch_mod, name, n_lights, arith, mode):
    isc, ms = device_set(name)
    want, wst, wtr, d, xy, _ = K.reference(name, mode, n_lights, K.GPU_DEPTH)
    set_arith(isc, arith)
    try:
        got, st, tr = tree_packets(isc, ms, K.camera(name), K.FRAME, xy, K.lights_of(name, n_lights), REFL, K.GPU_DEPTH, torch=torch_mod)
    finally:
        set_arith(isc, "ieee")
    assert_packets("%s, %d lights, maxDepth %d, %s" % (name, n_lights, K.GPU_DEPTH, arith), got, want, st, wst, tr, wtr)
    assert d.b_selected and d.truncated_b > 0


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("name", ["glasshouse", "moved"])
def test_whole_frames_with_reflections_equal_the_restatement(torch_mod, name, arith, mode):
    """at FULL_DEPTH no lane is cut: counter 0, the frame is the reference's"""
    isc, ms = device_set(name)
    want, wst, wtr, d, xy, _ = K.reference(name, mode, 2, K.FULL_DEPTH)
    set_arith(isc, arith)
    try:
        got, st, tr = tree_packets(isc, ms, K.camera(name), K.FRAME, xy, K.lights_of(name, 2), REFL, K.FULL_DEPTH, torch=torch_mod)
    finally:
        set_arith(isc, "ieee")
    assert_packets("%s, maxDepth %d, %s" % (name, K.FULL_DEPTH, arith), got, want, st, wst, tr, wtr)
    assert wtr == 0


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("name", ["glasshouse", "moved"])
def test_aa4_and_the_tint_equal_the_restatement(torch_mod, name, arith, mode):
    isc, ms = device_set(name)
    tr = K.tiles_ref(name)
    cam, (resx, resy) = K.camera(name), K.AA_FRAME
    xy = S.frame_packets(resx, resy)
    lights = K.lights_of(name, 2)
    set_arith(isc, arith)
    try:
        for tint in (None, K.TINT):
            want, wst = tr.packets(cam.as_array13(), resx, resy, xy, lights, REFL | AA4, tint=tint, mode=mode)
            got, st, trunc = tree_packets(isc, ms, cam, (resx, resy), xy, lights, REFL | AA4, K.GPU_DEPTH, tint, torch=torch_mod)
            assert_packets("%s AA4 tint %s, %s" % (name, tint, arith), got, want, st, wst, trunc, tr.truncated)
    finally:
        set_arith(isc, "ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("depth", [K.CUT_DEPTH, 2, 8])
def test_the_deep_case(torch_mod, depth, arith, mode):
    isc, ms = device_set("deep")
    want, wst, wtr, d, xy, _ = K.reference("deep", mode, 1, depth)
    set_arith(isc, arith)
    try:
        got, st, tr = tree_packets(isc, ms, K.camera("deep"), K.FRAME, xy, K.lights_of("deep", 1), REFL, depth, torch=torch_mod)
    finally:
        set_arith(isc, "ieee")
    assert_packets("deep, maxDepth %d, %s" % (depth, arith), got, want, st, wst, tr, wtr)
    assert (wtr > 0) == (depth == K.CUT_DEPTH) and sum(v for k, v in d.mirrored_all_miss.items() if k >= 1) >= 1


@pytest.mark.parametrize("arith,mode", ARITH)
def test_an_explicit_packet_list_with_a_repeated_and_an_outside_packet(torch_mod, arith, mode):
    name = "moved"
    isc, ms = device_set(name)
    xy = ((32, 16), (80, 48), (32, 16), (96, 0), (0, 64), (16, 32))          # (96, 0) and (0, 64) lie outside the 96x64 frame
    want, wst, wtr, _, pk, _ = K.reference(name, mode, 2, K.GPU_DEPTH, xy=xy)
    set_arith(isc, arith)
    try:
        got, st, tr = tree_packets(isc, ms, K.camera(name), K.FRAME, pk, K.lights_of(name, 2), REFL, K.GPU_DEPTH, torch=torch_mod)
    finally:
        set_arith(isc, "ieee")
    assert_packets("packet list, %s" % arith, got, want, st, wst, tr, wtr)
    assert np.array_equal(got[0], got[2])


@pytest.mark.parametrize("arith,mode", ARITH)
def test_mirror_rays_on_a_level_of_the_restatement(torch_mod, arith, mode):
    torch = torch_mod
    name = "glasshouse"
    isc, ms = device_set(name)
    rec = K.reference(name, mode, 2, K.GPU_DEPTH)[5]
    idx, rows = R.call_records(rec, None, 1)                                  # the calls A_1: generic packets that mirror
    n = len(rows)
    assert n >= 4 and all("mirrored" in r for r in rows)
    stack = lambda f: np.ascontiguousarray(np.stack([f(r) for r in rows]))    # noqa: E731
    origin, dirs, mask = stack(lambda r: r["rays"]["origin"]), stack(lambda r: r["rays"]["dir"]), stack(lambda r: r["rays"]["mask"])
    t, smp = stack(lambda r: r["t"].reshape(256)), stack(lambda r: r["samples"])
    skip = 1
    order_in = np.arange(n, dtype=np.int32); order_in[skip] = -1
    want = {k: stack(lambda r, k=k: r["mirrored"][k]) for k in ("origin", "dir", "idir", "mask", "distance", "object", "element", "bary")}
    set_arith(isc, arith)
    try:
        f = lambda *shape: torch.full(shape, 7.0, dtype=torch.float32, device="cuda:0")      # noqa: E731
        i = lambda *shape: torch.full(shape, 7, dtype=torch.int32, device="cuda:0")          # noqa: E731
        out = (f(n, 64, 3, 4), f(n, 64, 3, 4), f(n, 64, 3, 4), torch.full((n, 64), 7, dtype=torch.uint8, device="cuda:0"), f(n, 256), i(n, 256), i(n, 256), f(n, 64, 2, 4), i(n))
        st = isc.new_stats()
        ms.mirror_rays(dev(torch, origin), dev(torch, dirs), dev(torch, mask), dev(torch, t), dev(torch, smp), dev(torch, order_in), out=out, stats=st)
        got = [o.cpu().numpy() for o in out]
        # ... and without an order list: every packet
        st2 = isc.new_stats()
        all_ = [o.cpu().numpy() for o in ms.mirror_rays(dev(torch, origin), dev(torch, dirs), dev(torch, mask), dev(torch, t), dev(torch, smp), stats=st2)]
    finally:
        set_arith(isc, "ieee")
    keep = np.arange(n) != skip
    lanes = lambda m: int(np.unpackbits(np.ascontiguousarray(m & 15).reshape(-1)).sum())      # noqa: E731
    for k, (g, a) in zip(("origin", "dir", "idir", "mask", "distance", "object", "element", "bary"), zip(got, all_)):
        w = want[k].reshape(g.shape)
        G.assert_bits("mirror_rays %s, %s" % (k, arith), g[keep], w[keep])
        G.assert_bits("mirror_rays %s without an order list, %s" % (k, arith), a, w)
        assert (g[skip] == 7).all(), k                                       # nothing of the skipped packet is written
    assert np.array_equal(got[8], order_in) and np.array_equal(all_[8], np.arange(n))
    assert np_stats(st).tolist() == [0, 0, lanes(want["mask"][keep]), 0] and np_stats(st2).tolist() == [0, 0, lanes(want["mask"]), 0]


# ---- tiles ----
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("key,flags,tint", [("column", REFL, None), ("right_edge", REFL, None), ("rect", REFL | AA4, K.TINT), ("shared_packet", REFL, K.TINT)])
def test_tiles_equal_the_packet_form_through_the_planar_store(torch_mod, key, flags, tint, arith, mode):
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
        pk, pst, ptr = tree_packets(isc, ms, cam, (resx, resy), DT.tile_packets(tiles), lights, flags, K.GPU_DEPTH, tint, torch=torch_mod)
        data, _, st, trunc = ms.render_tree_tiles_host(cam, resx, resy, tiles, offsets, lights, flags, tint, data=data, max_depth=K.GPU_DEPTH, truncated=np.full(1, 3, dtype=np.uint64))
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
    assert np.array_equal(np_stats(st), pst) and int(trunc[0]) == 3 + ptr


# ---- slicing ----
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("frame,flags,tint", [(K.FRAME, REFL, None), (K.AA_FRAME, REFL | AA4, K.TINT)])
def test_slicing_changes_nothing(torch_mod, frame, flags, tint, arith, mode):
    name = "glasshouse"
    isc, ms = device_set(name)
    xy = S.frame_packets(*frame)
    lights = K.lights_of(name, 2)
    one = ms.level_bytes(2, flags, K.GPU_DEPTH)
    assert one > 0 and ms.level_bytes(2, flags | DEPTH, K.GPU_DEPTH) == 0
    set_arith(isc, arith)
    try:
        whole = tree_packets(isc, ms, K.camera(name), frame, xy, lights, flags, K.GPU_DEPTH, tint, torch=torch_mod)
        ms.set_level_budget(one)                          # one output packet per slice
        try:
            single = tree_packets(isc, ms, K.camera(name), frame, xy, lights, flags, K.GPU_DEPTH, tint, torch=torch_mod)
            ms.set_level_budget(3 * one + one // 2)       # three per slice, the last slice shorter
            three = tree_packets(isc, ms, K.camera(name), frame, xy, lights, flags, K.GPU_DEPTH, tint, torch=torch_mod)
        finally:
            ms.set_level_budget(1 << 30)
    finally:
        set_arith(isc, "ieee")
    assert_packets("one packet per slice, %s" % arith, single[0], whole[0], single[1], whole[1], single[2], whole[2])
    assert_packets("three packets per slice, %s" % arith, three[0], whole[0], three[1], whole[1], three[2], whole[2])
    assert whole[0].any()


def test_level_bytes_of_refused_arguments_is_minus_1(torch_mod):
    L = _lib.lib()
    for args in ((0, 8, 1), (0, 0, 0), (0, 0, 9), (9, 0, 1), (-1, 0, 1)):
        assert L.snail_instances_materials_level_bytes(*args) == -1, args
    _, ms = device_set("glasshouse")
    with pytest.raises(_lib.SnailError):
        ms.level_bytes(0, 8, 1)
    with pytest.raises(_lib.SnailError):
        ms.set_level_budget(0)


# ---- ordering against updates ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_a_frame_an_update_and_a_frame_on_one_stream(torch_mod, arith, mode):
    torch = torch_mod
    u = C.case("moved")
    isc, ms = G.new_set("glasshouse")                                 # (a handle of this test's own: the cached one keeps its transforms)
    isc1, ms1 = device_set("moved")
    cam, (resx, resy) = K.camera("glasshouse"), K.FRAME
    xy = dev(torch, S.frame_packets(resx, resy))
    lights = K.lights_of("glasshouse", 2)
    set_arith(isc, arith); set_arith(isc1, arith)
    try:
        sa, sb, sc = isc.new_stats(), isc.new_stats(), isc1.new_stats()
        first, t0 = ms.tree_frame_packets(cam, resx, resy, xy, lights, REFL, stats=sa, max_depth=K.GPU_DEPTH)
        isc.update(u["rot"], u["tr"], u["bi"])
        second, t1 = ms.tree_frame_packets(cam, resx, resy, xy, lights, REFL, stats=sb, max_depth=K.GPU_DEPTH)
        fresh, t2 = ms1.tree_frame_packets(cam, resx, resy, xy, lights, REFL, stats=sc, max_depth=K.GPU_DEPTH)
        first, second, fresh = first.cpu().numpy(), second.cpu().numpy(), fresh.cpu().numpy()
    finally:
        set_arith(isc, "ieee"); set_arith(isc1, "ieee")
        ms.close()
        isc.close()
    assert_packets("after the update, %s" % arith, second, fresh, sb, sc, word(t1), word(t2))
    assert (first != second).any(axis=2).sum() >= 100 and not np.array_equal(np_stats(sa), np_stats(sb))
