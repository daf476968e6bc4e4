"""The one mirrored bounce under full shading on the MI355X (include/snail_materials_bounce.h; MaterialSet.mirror_packets / .shade_rays and
reflections=True): the mirror stage and the sample stage on generic packets bit for bit, frames byte for byte and TreeStats for equality
against the test-side restatement tests/materials_bounce_ref.py, in both arithmetics -- and, independent of that restatement, the
degenerate sets against the simple-shading bounce of Scene.render_whitted.  What the cases (tests/materials_bounce_cases.py) must exercise
is a condition of the cases, asserted on the restatement's diagnostics without a GPU by tests/test_materials_bounce_host.py."""
import numpy as np
import pytest

from snail_amd import HostBVH, _lib
from snail_amd import materials as P
from snail_amd.scene import Scene, _stream_ptr
from tests import dbvh_shade_ref as S
from tests import materials_bounce_cases as BK
from tests import materials_bounce_ref as B
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu
ARITH = [("ieee", O.MODE_IEEE), ("host_sse", O.MODE_SSE)]
FRAMES = BK.FRAMES                    # 24 and 20 packets, the second with partial packets
CASES = ["mirror", "large", "small", "quirk"]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_sets = {}


def device_set(name):
    """(Scene, MaterialSet) of a case, built once; the product builder's tree is the oracle's"""
    if name not in _sets:
        c = BK.case(name)
        hb = HostBVH.build(c["tv"])
        assert np.array_equal(hb.perm, c["osc"].perm) and hb.nodes.tobytes() == c["osc"].nodes.tobytes()
        sc = Scene(hb, 0)
        mats = []
        for d in c["descs"]:
            mats.append(P.Material.simple(d[1], d[2]) if d[0] == "simple" else P.Material.textured(d[1], d[2]) if d[0] == "tex" else P.Material.uber(d[1], d[2], d[3]))
        ms = P.MaterialSet(sc, c["uv"], c["nrm"], c["mat_index"], c["flat"], c["material_map"], mats, [P.Texture(t) for t in c["textures"]])
        _sets[name] = (sc, ms)
    return _sets[name]


def bits_differ(got, want):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (g.shape, w.shape, g.dtype, w.dtype)
    return g.view(np.uint8) != w.view(np.uint8)


# ---- 1. the mirror stage ----
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("resx,resy", FRAMES)
@pytest.mark.parametrize("name", CASES)
def test_mirror_stage(torch_mod, name, resx, resy, arith, mode):
    torch = torch_mod
    sc, ms = device_set(name)
    cam = BK.camera(name, resx)
    _, _, inter, xy, d = BK.reference(name, resx, resy, mode)
    sc.set_arith(arith)
    try:
        dxy = torch.from_numpy(np.array(xy)).to("cuda:0")
        hits = sc.trace_packets(cam, resx, resy, dxy)
        smp = ms.shade_packets(cam, resx, resy, dxy, hits)
        st = sc.new_stats()
        got = [a.cpu().numpy() for a in ms.mirror_packets(cam, resx, resy, dxy, hits[0], smp, stats=st)]
        st = st.cpu().numpy()
    finally:
        sc.set_arith("ieee")
    assert not bits_differ(smp.cpu().numpy(), B.stack(inter, "samples")).any()           # (the device's own primary samples are the restatement's)
    n = len(xy)
    want = [B.stack(inter, "mirrored", k) for k in ("origin", "dir", "idir", "mask", "distance", "object")]
    for k, g, w in zip(("origin", "dir", "idir", "mask", "distance", "object"), got, want):
        ne = bits_differ(g.reshape(w.shape), w)
        print("%s %dx%d %s %s: %d differing bytes of %d" % (name, resx, resy, arith, k, int(ne.sum()), ne.size))
        assert not ne.any(), (k, int(ne.sum()), np.argwhere(ne)[:4].tolist())
    assert got[3].shape == (n, 64) and d.mirrored_lanes >= 256
    assert st.tolist() == [0, 0, d.mirrored_lanes, 0]                                      # TracingRays(CountMaskBits(mask)) of the nested call


# ---- 2. the sample stage on generic packets ----
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("resx,resy", FRAMES)
@pytest.mark.parametrize("name", CASES)
def test_sample_stage_on_generic_packets(torch_mod, name, resx, resy, arith, mode):
    """the restatement's mirrored packets and their hits in, its nested samples out; the list mixes masked and unmasked packets wherever the
    case has both (`mirror` at 96 x 64, `quirk`), and the unmasked ones once more without a mask array"""
    torch = torch_mod
    sc, ms = device_set(name)
    _, _, inter, xy, d = BK.reference(name, resx, resy, mode)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")      # noqa: E731
    dirs, mask = B.stack(inter, "mirrored", "dir"), B.stack(inter, "mirrored", "mask")
    t, u, v, tid = (B.stack(inter, "nested", k).reshape(len(xy), 256) for k in ("t", "u", "v", "tri_id"))
    want = B.stack(inter, "nested", "samples")
    sc.set_arith(arith)
    try:
        got = ms.shade_rays(dev(dirs), dev(mask), dev(t), dev(u), dev(v), dev(tid)).cpu().numpy()
        full = np.flatnonzero((mask == 15).all(axis=1))
        got_full = ms.shade_rays(dev(dirs[full]), None, dev(t[full]), dev(u[full]), dev(v[full]), dev(tid[full])).cpu().numpy() if len(full) else None
    finally:
        sc.set_arith("ieee")
    ne = bits_differ(got, want)
    print("%s %dx%d %s: samples differing %d of %d; nested packets masked / unmasked %d / %d" % (name, resx, resy, arith, int(ne.sum()), ne.size, d.packets_masked, d.packets_unmasked))
    assert not ne.any(), (int(ne.sum()), np.argwhere(ne)[:5].tolist())
    assert want.any() and len(full) == d.packets_unmasked
    if got_full is not None:
        assert not bits_differ(got_full, want[full]).any()
    if name == "mirror" and resx == 96:
        assert d.packets_masked >= 8 and d.packets_unmasked >= 8 and d.a_uber_masked >= 8 and d.a_uber_unmasked >= 8


# ---- 3. frames ----
def check_frames(torch, name, resx, resy, arith, mode, lights_key):
    sc, ms = device_set(name)
    cam = BK.camera(name, resx)
    lights = BK.lights_of(name, lights_key)
    want, wst, _, xy, d = BK.reference(name, resx, resy, mode, lights_key)
    # a shuffled list that leaves packets out, restated on its own
    pick = np.random.default_rng(7).permutation(len(xy))[: (2 * len(xy)) // 3]
    sub = np.ascontiguousarray(np.array(xy)[pick])
    wsub, wsst, _ = B.BounceRef(BK.materials_ref(name)).render_packets(cam.as_array13(), resx, resy, sub, lights, mode=mode)
    sc.set_arith(arith)
    try:
        st, st2 = sc.new_stats(), sc.new_stats()
        frame = ms.render(cam, resx, resy, lights, stats=st, reflections=True).cpu().numpy()
        bgr = ms.render_packets(cam, resx, resy, torch.from_numpy(sub).to("cuda:0"), lights, stats=st2, reflections=True).cpu().numpy()
        img, hst = ms.render_image_host(cam, resx, resy, lights, reflections=True)
        plain = ms.render(cam, resx, resy, lights).cpu().numpy()
    finally:
        sc.set_arith("ieee")
    st, st2 = st.cpu().numpy().astype(np.uint64), st2.cpu().numpy().astype(np.uint64)
    bad = np.argwhere((frame != want).any(axis=2))
    print("%s %dx%d %s lights=%s: %d differing pixels; stats %s / %s; list %d differing bytes, stats %s / %s" %
          (name, resx, resy, arith, lights_key, len(bad), st.tolist(), wst.tolist(), int((bgr != wsub).sum()), st2.tolist(), wsst.tolist()))
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), frame[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())
    assert np.array_equal(st, wst), (st, wst)
    assert np.array_equal(bgr, wsub) and np.array_equal(st2, wsst), (st2, wsst)
    assert np.array_equal(img.reshape(resy, resx, 3), want) and np.array_equal(hst, wst)
    assert (plain != want).any() and d.mirrored_hits >= 8          # the bounce shows
    return d


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("resx,resy", FRAMES)
@pytest.mark.parametrize("name", CASES)
def test_frames_with_the_case_s_lights(torch_mod, name, resx, resy, arith, mode):
    check_frames(torch_mod, name, resx, resy, arith, mode, "case")


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("lights_key", ["none", "eight"])
@pytest.mark.parametrize("name,resx,resy", [("mirror", 96, 64), ("small", 70, 50)])
def test_frames_without_lights_and_with_eight(torch_mod, name, resx, resy, lights_key, arith, mode):
    d = check_frames(torch_mod, name, resx, resy, arith, mode, lights_key)
    if lights_key == "eight":
        assert len(BK.eight_lights(name)) == 8 and len({n for _, n in d.nested.not_culled}) >= 2 and d.nested.lit_pixels >= 8
    else:
        assert d.nested.lit_pixels == 0 and d.primary.lit_pixels == 0


# ---- 4. independent of the restatement ----
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("name", ["degenerate_box", "degenerate_small"])
def test_degenerate_set_equals_the_simple_shading_bounce(torch_mod, name, arith, mode):
    sc, ms = device_set(name)
    c = BK.case(name)
    sc.set_arith(arith)
    try:
        for resx, resy in FRAMES:
            st0, st1 = sc.new_stats(), sc.new_stats()
            want = sc.render_whitted(c["cam"], resx, resy, c["lights"], color=(1.0, 1.0, 1.0), stats=st0, reflections=True).cpu().numpy()
            got = ms.render(c["cam"], resx, resy, c["lights"], stats=st1, reflections=True).cpu().numpy()
            plain = ms.render(c["cam"], resx, resy, c["lights"]).cpu().numpy()
            bad = np.argwhere((got != want).any(axis=2))
            print("%s %dx%d %s: %d differing pixels, stats %s / %s" % (name, resx, resy, arith, len(bad), st1.cpu().numpy().tolist(), st0.cpu().numpy().tolist()))
            assert want.any() and (want != plain).any()
            assert len(bad) == 0, (len(bad), bad[:5].tolist())
            assert np.array_equal(st0.cpu().numpy(), st1.cpu().numpy())
    finally:
        sc.set_arith("ieee")


# ---- 5. flags == 0 through the new functions ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_flags_0_is_the_frame_without_the_bounce(torch_mod, arith, mode):
    torch = torch_mod
    sc, ms = device_set("small")
    c = BK.case("small")
    resx, resy = 70, 50
    cam = BK.camera("small", resx)
    L = _lib.lib()
    cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32)
    lights = np.ascontiguousarray(c["lights"], dtype=np.float32)
    amb = np.array([0.1, 0.1, 0.1], dtype=np.float32)
    sc.set_arith(arith)
    try:
        st0, st1, st2 = sc.new_stats(), sc.new_stats(), sc.new_stats()
        want = ms.render(cam, resx, resy, lights, stats=st0).cpu().numpy()
        out = torch.zeros((resy, resx, 3), dtype=torch.uint8, device="cuda:0")
        _lib.check(L.snail_materials_bounce_dev(ms._h, _lib.ptr(cam13), resx, resy, _lib.ptr(lights), len(lights), _lib.ptr(amb), 0, _lib.ptr(out), resx * 3, _lib.ptr(st1),
                                                _stream_ptr(None)), "snail_materials_bounce_dev")
        xy = torch.from_numpy(S.frame_packets(resx, resy)).to("cuda:0")
        bgr = torch.zeros((len(xy), 256, 3), dtype=torch.uint8, device="cuda:0")
        _lib.check(L.snail_materials_bounce_packets_dev(ms._h, _lib.ptr(cam13), resx, resy, _lib.ptr(xy), len(xy), _lib.ptr(lights), len(lights), _lib.ptr(amb), 0,
                                                        _lib.ptr(bgr), _lib.ptr(st2), _stream_ptr(None)), "snail_materials_bounce_packets_dev")
        img = np.zeros((resy, resx * 3), dtype=np.uint8)
        hst = np.zeros(4, dtype=np.uint64)
        _lib.check(L.snail_materials_bounce_image(ms._h, _lib.ptr(cam13), resx, resy, _lib.ptr(lights), len(lights), _lib.ptr(amb), 0, _lib.ptr(img), resx * 3, _lib.ptr(hst)),
                   "snail_materials_bounce_image")
    finally:
        sc.set_arith("ieee")
    assert want.any() and np.array_equal(out.cpu().numpy(), want) and np.array_equal(st1.cpu().numpy(), st0.cpu().numpy())
    assert np.array_equal(S.packets_to_frame(xy.cpu().numpy(), bgr.cpu().numpy(), resx, resy), want) and np.array_equal(st2.cpu().numpy(), st0.cpu().numpy())
    assert np.array_equal(img.reshape(resy, resx, 3), want) and np.array_equal(hst, st0.cpu().numpy().astype(np.uint64))


# ---- 6. more launches in flight than the set has groups of intermediates ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_nine_launches_on_two_streams_then_a_smaller_and_a_larger_frame(torch_mod, arith, mode):
    """a set of its own, so that the sizes of its eight groups of intermediates are this test's: all eight sized by the smaller frame, then
    grown by the larger one; then nine launches on two streams without a wait in between (the ninth takes the first launch's group, on the
    other stream), a smaller frame and a larger one behind them"""
    torch = torch_mod
    sc, _ = device_set("mirror")
    c = BK.case("mirror")
    cam = c["cam"]
    mats = [P.Material.simple(d[1], d[2]) if d[0] == "simple" else P.Material.textured(d[1], d[2]) if d[0] == "tex" else P.Material.uber(d[1], d[2], d[3]) for d in c["descs"]]
    ms = P.MaterialSet(sc, c["uv"], c["nrm"], c["mat_index"], c["flat"], c["material_map"], mats, [P.Texture(t) for t in c["textures"]])
    small, large = (70, 50), (96, 64)
    want = {f: BK.reference("mirror", f[0], f[1], mode)[0] for f in (small, large)}
    sc.set_arith(arith)
    try:
        for f in (small, large):                 # every group allocated at the smaller frame's size, then grown
            for _ in range(8):
                assert np.array_equal(ms.render(cam, f[0], f[1], c["lights"], reflections=True).cpu().numpy(), want[f]), f
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(device="cuda:0"), torch.cuda.Stream(device="cuda:0")]
        got = []
        for k, f in enumerate([large] * 9 + [small, large]):
            with torch.cuda.stream(streams[k & 1]):
                got.append((f, ms.render(cam, f[0], f[1], c["lights"], stream=streams[k & 1], reflections=True)))
        for s in streams:
            s.synchronize()
    finally:
        sc.set_arith("ieee")
        torch.cuda.synchronize()
        ms.close()
    assert len(got) == 11
    for f, frame in got:
        assert np.array_equal(frame.cpu().numpy(), want[f]), f
