"""Full shading of plain scenes on the MI355X (include/snail_materials.h; snail_amd/materials.py): the sample buffer bit for bit, frames
byte for byte and TreeStats for equality against the test-side restatement tests/materials_ref.py, in both arithmetics -- and, independent
of that restatement, the degenerate set (every material the default, every triangle flat with its plane normal) against the simple-shading
frame of Scene.render_whitted.  The cases (tests/materials_cases.py) were chosen with the restatement alone; what each must exercise is
asserted on the restatement's own diagnostics, so that no comparison passes vacuously."""
import functools
import threading

import numpy as np
import pytest

from snail_amd import HostBVH
from snail_amd import materials as P
from snail_amd.scene import Scene
from tests import dbvh_shade_ref as S
from tests import materials_cases as K
from tests import materials_ref as M
from tests import oracle_lib as O
from tests import util as U

pytestmark = pytest.mark.gpu
ARITH = [("ieee", O.MODE_IEEE), ("host_sse", O.MODE_SSE)]
FRAMES = [(96, 64), (70, 50)]       # 24 and 20 packets, the second with partial packets


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_sets = {}


def device_set(name):
    """(Scene, MaterialSet) of a case, built once; the product builder's tree is the oracle's"""
    if name not in _sets:
        c = K.case(name)
        hb = HostBVH.build(c["tv"])
        assert np.array_equal(hb.perm, c["osc"].perm) and hb.nodes.tobytes() == c["osc"].nodes.tobytes()
        sc = Scene(hb, 0)
        mats = []
        for d in c["descs"]:
            mats.append(P.Material.simple(d[1], d[2]) if d[0] == "simple" else P.Material.textured(d[1], d[2]) if d[0] == "tex" else P.Material.uber(d[1], d[2], d[3]))
        ms = P.MaterialSet(sc, c["uv"], c["nrm"], c["mat_index"], c["flat"], c["material_map"], mats, [P.Texture(t) for t in c["textures"]])
        _sets[name] = (sc, ms)
    return _sets[name]


def camera(name, resx):
    c = K.case(name)
    return c["cam70"] if resx == 70 else c["cam"]


@functools.lru_cache(maxsize=None)
def reference(name, resx, resy, mode, lights_key="case"):
    """the restatement's frame, TreeStats, samples, packet list and diagnostics: computed once, shared, never changed"""
    c = K.case(name)
    lights = lights_of(name, lights_key)
    d = M.Diag()
    frame, st, smp, xy = K.reference(name).render(camera(name, resx).as_array13(), resx, resy, lights, mode=mode, diag=d)
    for a in (frame, st, smp, xy):
        a.setflags(write=False)
    return frame, st, smp, xy, d


def eight_lights(name):
    """eight lights before the small case's sheet, radii large enough that none is culled everywhere"""
    assert name == "small"
    return np.array([[-2.0 + 0.4 * k, -0.8 + 0.3 * k, -1.2 - 0.2 * k, 1.0 - 0.1 * k, 0.5, 0.2 + 0.1 * k, 3.0 + 0.8 * k] for k in range(8)], dtype=np.float32)


def lights_of(name, key):
    return K.case(name)["lights"] if key == "case" else None if key == "none" else eight_lights(name)


def check(torch, name, resx, resy, arith, mode, lights_key="case", samples=True):
    """sample buffer, frame and TreeStats of one frame against the restatement -> its diagnostics"""
    sc, ms = device_set(name)
    c = K.case(name)
    cam = camera(name, resx)
    lights = lights_of(name, lights_key)
    want, wst, wsmp, xy, d = reference(name, resx, resy, mode, lights_key)
    sc.set_arith(arith)
    try:
        if samples:
            dxy = torch.from_numpy(np.array(xy)).to("cuda:0")
            hits = sc.trace_packets(cam, resx, resy, dxy)
            smp = ms.shade_packets(cam, resx, resy, dxy, hits).cpu().numpy()
            ne = smp.view(np.uint32) != wsmp.view(np.uint32)
            print("%s %dx%d %s: samples differing %d of %d" % (name, resx, resy, arith, int(ne.sum()), ne.size))
            assert not ne.any(), (int(ne.sum()), np.argwhere(ne)[:5].tolist(), smp[tuple(np.argwhere(ne)[0])], wsmp[tuple(np.argwhere(ne)[0])])
        st = sc.new_stats()
        frame = ms.render(cam, resx, resy, lights, stats=st).cpu().numpy()
    finally:
        sc.set_arith("ieee")
    bad = np.argwhere((frame != want).any(axis=2))
    print("%s %dx%d %s lights=%s: %d differing pixels; stats %s / %s" % (name, resx, resy, arith, lights_key, len(bad), st.cpu().numpy().tolist(), wst.tolist()))
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), frame[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())
    assert np.array_equal(st.cpu().numpy().astype(np.uint64), wst), (st.cpu().numpy(), wst)
    return d


# ---- 1. the degenerate set: independent of the restatement ----
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("name", ["degenerate_box", "degenerate_small"])
def test_degenerate_set_equals_simple_shading(torch_mod, name, arith, mode):
    sc, ms = device_set(name)
    c = K.case(name)
    sc.set_arith(arith)
    try:
        for resx, resy in FRAMES:
            st0, st1 = sc.new_stats(), sc.new_stats()
            want = sc.render_whitted(c["cam"], resx, resy, c["lights"], color=(1.0, 1.0, 1.0), stats=st0).cpu().numpy()
            got = ms.render(c["cam"], resx, resy, c["lights"], stats=st1).cpu().numpy()
            bad = np.argwhere((got != want).any(axis=2))
            print("%s %dx%d %s: %d differing pixels, stats %s / %s" % (name, resx, resy, arith, len(bad), st1.cpu().numpy().tolist(), st0.cpu().numpy().tolist()))
            assert want.any() and len(np.unique(want.reshape(-1, 3), axis=0)) > 16
            assert len(bad) == 0, (len(bad), bad[:5].tolist())
            assert np.array_equal(st0.cpu().numpy(), st1.cpu().numpy())
    finally:
        sc.set_arith("ieee")


# ---- 2. large triangles ----
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("resx,resy", FRAMES)
def test_large_triangles(torch_mod, resx, resy, arith, mode):
    d = check(torch_mod, "large", resx, resy, arith, mode)
    lv = sorted(l for (t, l) in d.mips if t == 0)
    print("blocks a/b/c", d.blocks_a, d.blocks_b, d.blocks_c, "mips", dict(d.mips), "normals", d.normals_right, d.normals_left_a, d.normals_flat)
    assert d.blocks_a >= 100
    assert len(lv) >= 3 and lv[0] == 0 and lv[-1] == 6              # the 64 x 64 texture: level 0, its last level and at least one between
    assert any(t == 1 for (t, _) in d.mips)                          # the 32 x 8 texture is sampled
    assert d.normals_right > 0 and d.normals_left_a > 0 and d.normals_flat > 0
    assert d.lit_pixels >= 100


# ---- 3. small triangles ----
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("resx,resy", FRAMES)
def test_small_triangles(torch_mod, resx, resy, arith, mode):
    d = check(torch_mod, "small", resx, resy, arith, mode)
    print("blocks a/b/c", d.blocks_a, d.blocks_b, d.blocks_c, "default meets others", d.default_meets_others, "uber", d.uber_unmasked, d.uber_masked,
          "lit/occluded", d.lit_pixels, d.occluded_pixels, "culled/traced", len(d.culled), len(d.not_culled))
    assert d.blocks_a >= 100 and d.blocks_b >= 100 and d.blocks_c >= 100
    assert d.default_meets_others >= 1
    assert d.uber_unmasked >= 1 and d.uber_masked >= 1
    assert len(K.case("small")["lights"]) == 2 and d.lit_pixels >= 100 and d.occluded_pixels >= 100
    assert len(d.culled) >= 1 and len(d.not_culled) >= 1


# ---- 4. the quirk ----
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("resx,resy", FRAMES)
def test_lane_0_missed_beside_a_hit_of_triangle_0(torch_mod, resx, resy, arith, mode):
    d = check(torch_mod, "quirk", resx, resy, arith, mode)
    print("quirk lanes", d.quirk_lanes, "blocks with misses and one material", d.blocks_masked_one)
    assert d.quirk_lanes >= 1


# ---- 5. 0 and 8 lights, a DEEP scene ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_zero_and_eight_lights(torch_mod, arith, mode):
    d = check(torch_mod, "small", 64, 48, arith, mode, "none", samples=False)
    assert d.hit_pixels >= 1000 and d.lit_pixels == 0
    d = check(torch_mod, "small", 64, 48, arith, mode, "eight", samples=False)
    assert d.lit_pixels >= 100 and len({n for _, n in d.not_culled}) == 8


@pytest.mark.parametrize("arith,mode", ARITH)
def test_deep_scene(torch_mod, arith, mode):
    assert K.case("deep")["osc"].depth > 62
    d = check(torch_mod, "deep", 64, 48, arith, mode)
    assert d.hit_pixels >= 100 and d.lit_pixels >= 100


# ---- 6. the other two render calls ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_packet_list_and_host_image_equal_the_frame(torch_mod, arith, mode):
    torch = torch_mod
    sc, ms = device_set("small")
    c = K.case("small")
    resx, resy = 70, 50
    cam = camera("small", resx)
    sc.set_arith(arith)
    try:
        st = sc.new_stats()
        whole = ms.render(cam, resx, resy, c["lights"], stats=st).cpu().numpy()
        assert np.array_equal(whole, reference("small", resx, resy, mode)[0])
        xy = S.frame_packets(resx, resy)
        pick = np.random.default_rng(5).permutation(len(xy))[: len(xy) // 2]
        sub = np.ascontiguousarray(xy[pick])
        bgr = ms.render_packets(cam, resx, resy, torch.from_numpy(sub).to("cuda:0"), c["lights"]).cpu().numpy()
        part = S.packets_to_frame(sub, bgr, resx, resy)
        covered = S.packets_to_frame(sub, np.ones_like(bgr), resx, resy).astype(bool)
        assert covered.any() and np.array_equal(part[covered], whole[covered])
        img, hst = ms.render_image_host(cam, resx, resy, c["lights"])
        assert np.array_equal(img.reshape(resy, resx, 3), whole) and np.array_equal(hst, st.cpu().numpy().astype(np.uint64))
        # rows wider than the pixels: the padding stays as it was, on the host and on the device
        pitch = resx * 3 + 10
        img, _ = ms.render_image_host(cam, resx, resy, c["lights"], pitch=pitch, fill=0xAB)
        assert np.array_equal(img[:, :resx * 3].reshape(resy, resx, 3), whole) and (img[:, resx * 3:] == 0xAB).all()
        out = torch.full((resy, pitch), 0xCD, dtype=torch.uint8, device="cuda:0")
        ms.render(cam, resx, resy, c["lights"], out=out)
        o = out.cpu().numpy()
        assert np.array_equal(o[:, :resx * 3].reshape(resy, resx, 3), whole) and (o[:, resx * 3:] == 0xCD).all()
    finally:
        sc.set_arith("ieee")


# ---- 7. two host threads, one set ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_two_threads_render_from_one_set(torch_mod, arith, mode):
    torch = torch_mod
    sc, ms = device_set("small")
    c = K.case("small")
    jobs = [(96, 64), (70, 50)]
    want = [reference("small", rx, ry, mode)[0] for rx, ry in jobs]
    sc.set_arith(arith)
    got, errors = [[], []], []

    def work(k):
        try:
            rx, ry = jobs[k]
            stream = torch.cuda.Stream(device="cuda:0")
            for _ in range(12):        # more launches than the set has intermediates: the sets are recycled across the two streams
                with torch.cuda.stream(stream):
                    got[k].append(ms.render(camera("small", rx), rx, ry, c["lights"], stream=stream))
            stream.synchronize()
        except Exception as e:      # pragma: no cover
            errors.append(e)
    try:
        threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for k in range(2):
            assert len(got[k]) == 12
            for f in got[k]:
                assert np.array_equal(f.cpu().numpy(), want[k])
    finally:
        sc.set_arith("ieee")
