"""Full shading of instanced scenes on the MI355X (include/snail_instances_materials.h; snail_amd/instances_materials.py): the sample buffer
bit for bit, frames byte for byte and TreeStats for equality against the test-side restatement tests/instances_materials_ref.py, in both
arithmetics -- and, independent of that restatement, the degenerate set (every material the default, every record flat with its plane
normal) against the simple-shading frame of InstancedScene.render_whitted.  The cases (tests/instances_materials_cases.py) were chosen
with the restatement alone; what each must exercise is asserted on the restatement's own diagnostics, so that no comparison passes
vacuously."""
import functools
import threading

import numpy as np
import pytest

from snail_amd import HostBVH, _lib
from snail_amd import instances_materials as IP
from snail_amd import materials as P
from snail_amd.instances import InstancedScene
from snail_amd.scene import Scene
from tests import instances_materials_cases as K
from tests import instances_materials_ref as IM
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu
ARITH = [("ieee", O.MODE_IEEE), ("host_sse", O.MODE_SSE)]
FRAMES = [(96, 64), (70, 50)]       # 24 and 20 packets, the second with partial packets and rows that are no multiple of 4 bytes


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_blas, _sets = {}, {}


def blas_scene(key, tv, osc):
    """the device Scene of a BLAS, built once; the product builder's tree is the oracle's"""
    if key not in _blas:
        hb = HostBVH.build(tv)
        assert np.array_equal(hb.perm, osc.perm) and hb.nodes.tobytes() == osc.nodes.tobytes()
        _blas[key] = Scene(hb, 0)
    return _blas[key]


def product_materials():
    mats = []
    for d in K.DESCS:
        mats.append(P.Material.simple(d[1], d[2]) if d[0] == "simple" else P.Material.textured(d[1], d[2]) if d[0] == "tex" else P.Material.uber(d[1], d[2], d[3]))
    return mats, [P.Texture(t) for t in K.TEXTURES()]


def device_set(name):
    """(InstancedScene, InstancedMaterialSet) of a case, built once; the handle's tree and records are the case's own (built without a GPU)"""
    if name not in _sets:
        c = K.case(name)
        keys = ["chain"] if name == "deep" else ["sheet", "box"][:len(c["tvs"])]
        scs = [blas_scene(k, tv, osc) for k, tv, osc in zip(keys, c["tvs"], c["oscs"])]
        isc = InstancedScene(scs, c["rot"], c["tr"], c["bi"])
        check_tree(isc, c["ref"])
        mats, texs = product_materials()
        _sets[name] = (isc, IP.InstancedMaterialSet(isc, c["per_blas"], mats, texs))
    return _sets[name]


def check_tree(isc, ref):
    xs, bs = isc.slot_transforms()
    assert isc.nodes().tobytes() == ref.nodes.tobytes() and np.array_equal(xs, ref.xf) and np.array_equal(bs, ref.bi)


def set_arith(isc, arith):
    for s in isc.blas:
        s.set_arith(arith)


@functools.lru_cache(maxsize=None)
def reference(name, resx, resy, mode, lights_key="case"):
    """the restatement's frame, TreeStats, samples, packet list and diagnostics: computed once per (case, size, mode), shared, never changed"""
    c = K.case(name)
    d = IM.Diag()
    frame, st, smp, xy = K.reference(name).render(c["cams"][resx].as_array13(), resx, resy, lights_of(name, lights_key), mode=mode, diag=d)
    for a in (frame, st, smp, xy):
        a.setflags(write=False)
    return frame, st, smp, xy, d


def eight_lights():
    """eight lights before the main case's sheets, radii large enough that none is culled everywhere"""
    return np.array([[-2.0 + 0.6 * k, -0.8 + 0.3 * k, -1.6 - 0.2 * k, 1.0 - 0.1 * k, 0.5, 0.2 + 0.1 * k, 3.0 + 0.8 * k] for k in range(8)], dtype=np.float32)


def lights_of(name, key):
    return K.case(name)["lights"] if key == "case" else None if key == "none" else eight_lights()


def assert_frame(frame, want, st, wst, what):
    bad = np.argwhere((frame != want).any(axis=2))
    print("%s: %d differing pixels; stats %s / %s" % (what, len(bad), np.asarray(st).tolist(), wst.tolist()))
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), frame[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())
    assert np.array_equal(np.asarray(st).astype(np.uint64), wst), (what, st, wst)


# ---- 1. the sample buffer ----
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("name,resx,resy", [("main", 96, 64), ("quirk", 48, 32)])
def test_samples_equal_the_restatement(torch_mod, name, resx, resy, arith, mode):
    torch = torch_mod
    isc, ms = device_set(name)
    cam = K.case(name)["cams"][resx]
    _, _, wsmp, xy, d = reference(name, resx, resy, mode)
    set_arith(isc, arith)
    try:
        dxy = torch.from_numpy(np.array(xy)).to("cuda:0")
        hits = isc.trace_packets(cam, resx, resy, dxy)
        smp = ms.shade_packets(cam, resx, resy, dxy, hits).cpu().numpy()
    finally:
        set_arith(isc, "ieee")
    ne = smp.view(np.uint32) != wsmp.view(np.uint32)
    print("%s %dx%d %s: samples differing %d of %d" % (name, resx, resy, arith, int(ne.sum()), ne.size))
    assert not ne.any(), (int(ne.sum()), np.argwhere(ne)[:5].tolist(), smp[tuple(np.argwhere(ne)[0])], wsmp[tuple(np.argwhere(ne)[0])])
    if name == "quirk":
        assert d.quirk_lanes >= 1
        return
    assert min(d.blocks_a, d.blocks_b, d.blocks_c, d.normals_flat, d.normals_right, d.normals_left_a) >= 1, vars(d)
    assert any(mip > 0 for (_t, mip) in d.mips)
    assert d.uber_unmasked >= 1 and d.uber_masked >= 1
    assert d.cross_instance_same_tri >= 1 and d.shared_material_unmasked >= 1 and d.rotated_lanes >= 100


# ---- 2. lit frames: the three forms ----
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("resx,resy", FRAMES)
def test_lit_frames_equal_the_restatement(torch_mod, resx, resy, arith, mode):
    torch = torch_mod
    isc, ms = device_set("main")
    c = K.case("main")
    cam = c["cams"][resx]
    want, wst, _, xy, d = reference("main", resx, resy, mode)
    set_arith(isc, arith)
    try:
        st = isc.new_stats()
        frame = ms.render(cam, resx, resy, c["lights"], stats=st).cpu().numpy()
        assert_frame(frame, want, st.cpu().numpy(), wst, "_dev %dx%d %s" % (resx, resy, arith))
        # the packet list: every other packet, packet-major bytes
        sub = np.ascontiguousarray(np.array(xy)[::2])
        st = isc.new_stats()
        got = ms.render_packets(cam, resx, resy, torch.from_numpy(sub).to("cuda:0"), c["lights"], stats=st).cpu().numpy()
        pw, pst, _ = K.reference("main").render_packets(cam.as_array13(), resx, resy, sub, c["lights"], mode=mode)
        assert np.array_equal(got, pw) and np.array_equal(st.cpu().numpy().astype(np.uint64), pst)
        # the host image, with a pitch of its own: the bytes past a row's pixels stay
        img, ist = ms.render_image_host(cam, resx, resy, c["lights"], pitch=resx * 3 + 5, fill=0xCD)
        assert_frame(img[:, :resx * 3].reshape(resy, resx, 3), want, ist, wst, "_image %dx%d %s" % (resx, resy, arith))
        assert (img[:, resx * 3:] == 0xCD).all()
    finally:
        set_arith(isc, "ieee")
    assert d.hit_pixels >= resx * resy // 5 and d.lit_pixels >= 100 and d.occluded_pixels >= 100
    assert d.culled and d.not_culled


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("lights_key", ["none", "eight"])
def test_zero_and_eight_lights(torch_mod, lights_key, arith, mode):
    isc, ms = device_set("main")
    resx, resy = 70, 50
    want, wst, _, _, d = reference("main", resx, resy, mode, lights_key)
    set_arith(isc, arith)
    try:
        st = isc.new_stats()
        frame = ms.render(K.case("main")["cams"][resx], resx, resy, lights_of("main", lights_key), stats=st).cpu().numpy()
    finally:
        set_arith(isc, "ieee")
    assert_frame(frame, want, st.cpu().numpy(), wst, "%s lights %s" % (lights_key, arith))
    if lights_key == "none":
        assert d.lit_pixels == 0 and d.hit_pixels >= resx * resy // 5
    else:
        assert d.lit_pixels >= 100 and len({n for _, n in d.not_culled}) == 8


# ---- 3. independent of the restatement ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_degenerate_set_equals_simple_shading(torch_mod, arith, mode):
    isc, ms = device_set("degenerate")
    c = K.case("degenerate")
    set_arith(isc, arith)
    try:
        for resx, resy in FRAMES:
            st0, st1 = isc.new_stats(), isc.new_stats()
            want = isc.render_whitted(c["cams"][resx], resx, resy, c["lights"], color=(1.0, 1.0, 1.0), stats=st0).cpu().numpy()
            got = ms.render(c["cams"][resx], resx, resy, c["lights"], stats=st1).cpu().numpy()
            assert want.any() and len(np.unique(want.reshape(-1, 3), axis=0)) > 16
            assert_frame(got, want, st1.cpu().numpy(), st0.cpu().numpy().astype(np.uint64), "degenerate %dx%d %s" % (resx, resy, arith))
    finally:
        set_arith(isc, "ieee")


# ---- 4. updates: the kernels read the instance records at launch ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_the_same_set_follows_updates(torch_mod, arith, mode):
    torch = torch_mod
    c, u = K.case("main"), K.case("updated")
    mats, texs = product_materials()
    scs = [blas_scene(k, tv, osc) for k, tv, osc in zip(["sheet", "box"], c["tvs"], c["oscs"])]
    isc = InstancedScene(scs, c["rot"], c["tr"], c["bi"])          # (a scene of this test's own: the cached one keeps its transforms)
    ms = IP.InstancedMaterialSet(isc, c["per_blas"], mats, texs)
    resx, resy = 96, 64
    cam = c["cams"][resx]
    old, ost = reference("main", resx, resy, mode)[:2]
    new, nst = reference("updated", resx, resy, mode)[:2]
    assert int((old != new).any(axis=2).sum()) >= 500
    set_arith(isc, arith)
    try:
        st = isc.new_stats()
        assert_frame(ms.render(cam, resx, resy, c["lights"], stats=st).cpu().numpy(), old, st.cpu().numpy(), ost, "before the update")
        isc.update(u["rot"], u["tr"], u["bi"])
        check_tree(isc, u["ref"])
        st = isc.new_stats()
        assert_frame(ms.render(cam, resx, resy, c["lights"], stats=st).cpu().numpy(), new, st.cpu().numpy(), nst, "after update")
        # ... and back again on the device
        xf = np.concatenate([c["rot"].reshape(-1, 9), c["tr"]], axis=1).astype(np.float32)
        isc.update_dev(torch.from_numpy(xf).to("cuda:0"), torch.from_numpy(np.ascontiguousarray(c["bi"], dtype=np.int32)).to("cuda:0"))
        st = isc.new_stats()
        frame = ms.render(cam, resx, resy, c["lights"], stats=st).cpu().numpy()
        check_tree(isc, c["ref"])
        assert_frame(frame, old, st.cpu().numpy(), ost, "after update_dev")
    finally:
        set_arith(isc, "ieee")
        ms.close()
        isc.close()


# ---- 5. two host threads, one set ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_two_threads_render_from_one_set(torch_mod, arith, mode):
    torch = torch_mod
    isc, ms = device_set("main")
    c = K.case("main")
    want = [reference("main", rx, ry, mode)[0] for rx, ry in FRAMES]
    set_arith(isc, arith)
    got, errors = [[], []], []

    def work(k):
        try:
            rx, ry = FRAMES[k]
            stream = torch.cuda.Stream(device="cuda:0")
            for _ in range(4):
                with torch.cuda.stream(stream):
                    got[k].append(ms.render(c["cams"][rx], rx, ry, c["lights"], stream=stream))
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
            assert len(got[k]) == 4
            for f in got[k]:
                assert np.array_equal(f.cpu().numpy(), want[k])
    finally:
        set_arith(isc, "ieee")


# ---- 6. a DEEP BLAS ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_deep_blas_under_one_light(torch_mod, arith, mode):
    isc, ms = device_set("deep")
    c = K.case("deep")
    assert c["oscs"][0].depth > 62 and len(c["lights"]) == 1
    resx, resy = 64, 48
    want, wst, _, _, d = reference("deep", resx, resy, mode)
    set_arith(isc, arith)
    try:
        st = isc.new_stats()
        frame = ms.render(c["cams"][64], resx, resy, c["lights"], stats=st).cpu().numpy()
    finally:
        set_arith(isc, "ieee")
    assert_frame(frame, want, st.cpu().numpy(), wst, "deep %s" % arith)
    assert d.hit_pixels >= resx * resy // 5 and d.lit_pixels >= 100 and d.rotated_lanes >= 100


# ---- 7. what is refused against the handle ----
def test_a_set_that_does_not_fit_the_handle_is_refused(torch_mod):
    isc, _ = device_set("main")
    c = K.case("main")
    sh = [P.pack_shtris(*pb[:4], perm=osc.perm) for pb, osc in zip(c["per_blas"], c["oscs"])]
    maps = [pb[4] for pb in c["per_blas"]]
    mats, texs = product_materials()
    with pytest.raises(_lib.SnailError, match="nBlas"):
        IP.create_instanced_set(isc._h, sh[:1], maps[:1], mats, texs)
    with pytest.raises(_lib.SnailError, match="nTris"):
        IP.create_instanced_set(isc._h, [sh[0][:-1], sh[1]], maps, mats, texs)
    with pytest.raises(_lib.SnailError, match="nTris"):
        IP.create_instanced_set(isc._h, [sh[1], sh[0]], [maps[1], maps[0]], mats, texs)
