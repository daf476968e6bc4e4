"""Lit frames of instanced scenes on the MI355X (snail_instances_render_whitted_dev / _packets_dev / snail_instances_render_image):
frames byte for byte and TreeStats for equality against the test-side restatement tests/dbvh_shade_ref.py, in both arithmetics.  The
cases (tests/instances_shade_cases.py) were chosen with the restatement alone; what each must exercise is asserted on the restatement's
own output, so that no comparison passes vacuously."""
import threading

import numpy as np
import pytest

from snail_amd import scenes
from snail_amd.instances import InstancedScene
from tests import dbvh_ref as R
from tests import dbvh_shade_ref as S
from tests import instances_shade_cases as K
from tests import oracle_lib as O
from tests import util as U
from tests.test_gpu_instances import ARITH, blas, set_arith

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def device_scene(names, rot, tr, bi, ref=None):
    """The InstancedScene of a case and the restatement's scene over the tree the handle holds (the case's own, built without a GPU, is the same)"""
    isc = InstancedScene([blas(nm)[0] for nm in names], rot, tr, bi)
    xs, bs = isc.slot_transforms()
    if ref is not None:
        assert isc.nodes().tobytes() == ref.nodes.tobytes() and np.array_equal(xs, ref.xf) and np.array_equal(bs, ref.bi)
    return isc, R.Ref([blas(nm)[1] for nm in names], isc.nodes(), xs, bs)


def check_lit(isc, ref, cam, resx, resy, lights, reflections, arith, mode, diag=None, want_cross=False):
    set_arith(isc, arith)
    st = isc.new_stats()
    frame = isc.render_whitted(cam, resx, resy, lights, stats=st, reflections=reflections).cpu().numpy()
    want, wst = S.ShadeRef(ref, want_cross=want_cross).render(cam.as_array13(), resx, resy, lights, reflections=reflections, mode=mode, diag=diag)
    bad = np.argwhere((frame != want).any(axis=2))
    print("lit frame %dx%d %s refl=%d: %d differing pixels; stats %s / %s" % (resx, resy, arith, reflections, len(bad), st.cpu().numpy().tolist(), wst.tolist()))
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), frame[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())
    assert np.array_equal(st.cpu().numpy().astype(np.uint64), wst), (st.cpu().numpy(), wst)
    return want


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("reflections", [False, True], ids=["plain", "reflections"])
def test_field_frames_equal_the_restatement(torch_mod, reflections, arith, mode):
    """24 instances over box + lancia, 128x96, two lights inside the field's box, the second with a radius that the packet-level cull removes
    for some packets"""
    names, rot, tr, bi, resx, resy, cam, lights, cref = K.case("field")
    lo, hi = cref.nodes[0]["bmin"], cref.nodes[0]["bmax"]
    assert ((lights[:, :3] >= lo) & (lights[:, :3] <= hi)).all()
    isc, ref = device_scene(names, rot, tr, bi, cref)
    d = S.Diag()
    check_lit(isc, ref, cam, resx, resy, lights, reflections, arith, mode, d, want_cross=True)
    assert d.hit_pixels >= resx * resy // 5
    assert d.lit_pixels >= 100 and d.occluded_pixels >= 100 and d.cross_instance_occluders >= 1
    assert any(n == 1 for _, n in d.culled) and any(n == 1 for _, n in d.not_culled)
    if reflections:
        assert d.mirrored_hits >= 100
    set_arith(isc, "ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("name", ["overlap", "inside"])
def test_overlapping_instances_and_a_camera_inside(torch_mod, name, arith, mode):
    names, rot, tr, bi, resx, resy, cam, lights, cref = K.case(name)
    isc, ref = device_scene(names, rot, tr, bi, cref)
    for reflections in (False, True):
        d = S.Diag()
        check_lit(isc, ref, cam, resx, resy, lights, reflections, arith, mode, d, want_cross=True)
        assert d.hit_pixels >= resx * resy // 5 and d.lit_pixels >= 100 and d.occluded_pixels >= 100
        assert d.cross_instance_occluders >= 1 or name == "inside"      # (inside: the camera's own instance fills the view and shadows itself)
        if reflections:
            assert d.mirrored_hits >= 100
    set_arith(isc, "ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
def test_deep_blas_field(torch_mod, arith, mode):
    """chain + box: the DEEP inner walk under the shadow and mirrored packets (lights outside the field, so that instances shadow each other)"""
    assert blas("chain")[1].depth > 62
    names, rot, tr, bi, resx, resy, cam, lights, cref = K.case("deep")
    isc, ref = device_scene(names, rot, tr, bi, cref)
    for reflections in (False, True):
        d = S.Diag()
        check_lit(isc, ref, cam, resx, resy, lights, reflections, arith, mode, d, want_cross=True)
        assert d.hit_pixels >= resx * resy // 5 and d.lit_pixels >= 100 and d.occluded_pixels >= 100 and d.cross_instance_occluders >= 1
        if reflections:
            assert d.mirrored_hits >= 100
    set_arith(isc, "ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
def test_zero_and_eight_lights(torch_mod, arith, mode):
    names, rot, tr, bi, resx, resy, cam, lights, cref = K.case("field")
    isc, ref = device_scene(names, rot, tr, bi, cref)
    resx, resy = 64, 48
    d = S.Diag()
    check_lit(isc, ref, cam, resx, resy, None, True, arith, mode, d)          # colour = diffuse only (blended with the mirrored colour)
    assert d.hit_pixels >= resx * resy // 5 and d.lit_pixels == 0
    spec = [(0.1 + 0.1 * k, 0.3 + 0.08 * k, 0.9 - 0.1 * k, (1.0 - 0.1 * k, 0.5, 0.2 + 0.1 * k), 0.15 + 0.12 * k) for k in range(8)]
    eight = K.field_lights(cref.nodes, spec)
    d = S.Diag()
    check_lit(isc, ref, cam, resx, resy, eight, False, arith, mode, d)
    assert d.lit_pixels >= 100 and d.occluded_pixels >= 100 and len({n for _, n in d.not_culled}) == 8
    # a frame whose size is no multiple of 16 or of 4, rows of 3 * resx bytes (no multiple of 4): the byte-wise tail of the store; every pixel
    # inside resx x resy is compared
    d = S.Diag()
    check_lit(isc, ref, cam, 90, 53, lights, True, arith, mode, d)
    assert d.hit_pixels >= 90 * 53 // 5 and d.lit_pixels >= 100
    set_arith(isc, "ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
def test_packet_list_and_host_image(torch_mod, arith, mode):
    torch = torch_mod
    names, rot, tr, bi, resx, resy, cam, lights, cref = K.case("field")
    isc, ref = device_scene(names, rot, tr, bi, cref)
    set_arith(isc, arith)
    whole = isc.render_whitted(cam, resx, resy, lights, reflections=True).cpu().numpy()
    xy = S.frame_packets(resx, resy)
    pick = np.random.default_rng(5).permutation(len(xy))[: len(xy) // 2]
    sub = np.ascontiguousarray(xy[pick])
    st = isc.new_stats()
    got = isc.render_whitted_packets(cam, resx, resy, torch.from_numpy(sub).cuda(), lights, stats=st, reflections=True).cpu().numpy()
    for k, (px, py) in enumerate(sub.tolist()):
        assert np.array_equal(got[k].reshape(16, 16, 3), whole[py:py + 16, px:px + 16]), (k, px, py)
    want, wst = S.ShadeRef(ref).render_packets(cam.as_array13(), resx, resy, sub, lights, reflections=True, mode=mode)
    assert np.array_equal(got, want) and np.array_equal(st.cpu().numpy().astype(np.uint64), wst)
    # the host-pointer image call: lit, and SNAIL_RENDER_DEPTH = snail_instances_render_depth; 4x antialiasing is refused with nothing written
    img, ist = isc.render_image_host(cam, resx, resy, lights, flags=InstancedScene.RENDER_REFLECTIONS)
    wf, wfs = S.ShadeRef(ref).render(cam.as_array13(), resx, resy, lights, reflections=True, mode=mode)
    assert np.array_equal(img, whole) and np.array_equal(img, wf) and np.array_equal(ist, wfs)
    dimg, dst = isc.render_image_host(cam, resx, resy, flags=InstancedScene.RENDER_DEPTH)
    assert np.array_equal(dimg, isc.render_depth(cam, resx, resy).cpu().numpy()) and dimg.any()
    rt, _, _, _, _, rst = ref.render_primary(cam.as_array13(), resx, resy, mode=mode)
    assert np.array_equal(dimg, O.shade_depth(rt, mode=mode).reshape(resy, resx, 3)) and np.array_equal(dst, rst)
    from snail_amd import _lib
    with pytest.raises(_lib.SnailError, match="AA4"):
        isc.render_image_host(cam, resx, resy, lights, flags=InstancedScene.RENDER_AA4)
    set_arith(isc, "ieee")


@pytest.mark.parametrize("arith", ["ieee", "host_sse"])
@pytest.mark.parametrize("reflections", [False, True], ids=["plain", "reflections"])
def test_identity_instance_of_the_atrium_equals_the_plain_scene(torch_mod, reflections, arith):
    sc = blas("atrium")[0]
    isc = InstancedScene([sc], np.eye(3, dtype=np.float32)[None], np.zeros((1, 3), np.float32))
    set_arith(isc, arith)
    cam = U.camera_for("atrium", blas("atrium")[2])
    lights = K.field_lights(isc.nodes(), [(0.5, 0.7, 0.5, K.WHITE, 1.0), (0.3, 0.4, 0.6, K.WARM, 0.2)])
    got = isc.render_whitted(cam, 256, 256, lights, reflections=reflections).cpu().numpy()
    want = sc.render_whitted(cam, 256, 256, lights, reflections=reflections).cpu().numpy()
    assert np.array_equal(got, want), int((got != want).any(axis=2).sum())
    assert (want.reshape(-1, 3).max(axis=1) > 0).sum() > 256 * 256 // 5
    set_arith(isc, "ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
def test_update_between_two_lit_frames_on_one_stream(torch_mod, arith, mode):
    torch = torch_mod
    names, rot, tr, bi, resx, resy, cam, lights, cref = K.case("field")
    resx, resy = 64, 48
    isc, ref1 = device_scene(names, rot, tr, bi, cref)
    set_arith(isc, arith)
    rot2, tr2, bi2 = K.layout(names, 40, 77, 0.1)          # instances moved, count grown past the handle's buffers
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        f1 = isc.render_whitted(cam, resx, resy, lights, stream=s, reflections=True)
        isc.update(rot2, tr2, bi2, stream=s)
        f2 = isc.render_whitted(cam, resx, resy, lights, stream=s, reflections=True)
    s.synchronize()
    xs, bs = isc.slot_transforms()
    assert len(xs) == 40
    ref2 = R.Ref([blas(nm)[1] for nm in names], isc.nodes(), xs, bs)
    w1 = S.ShadeRef(ref1).render(cam.as_array13(), resx, resy, lights, reflections=True, mode=mode)[0]
    w2 = S.ShadeRef(ref2).render(cam.as_array13(), resx, resy, lights, reflections=True, mode=mode)[0]
    assert np.array_equal(f1.cpu().numpy(), w1) and np.array_equal(f2.cpu().numpy(), w2)
    assert not np.array_equal(w1, w2)
    set_arith(isc, "ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
def test_eight_threads_render_lit_frames_on_one_handle(torch_mod, arith, mode):
    torch = torch_mod
    names, rot, tr, bi, resx, resy, cam, lights, cref = K.case("field")
    resx, resy = 64, 48
    isc, ref = device_scene(names, rot, tr, bi, cref)
    set_arith(isc, arith)
    want = isc.render_whitted(cam, resx, resy, lights, reflections=True).cpu().numpy()
    assert np.array_equal(want, S.ShadeRef(ref).render(cam.as_array13(), resx, resy, lights, reflections=True, mode=mode)[0])
    errors = []

    def work(k):
        try:
            s = torch.cuda.Stream()
            for _ in range(3):
                with torch.cuda.stream(s):
                    f = isc.render_whitted(cam, resx, resy, lights, stream=s, reflections=True)
                s.synchronize()
                if not np.array_equal(f.cpu().numpy(), want):
                    errors.append(k)
        except Exception as e:   # pragma: no cover
            errors.append(repr(e))

    th = [threading.Thread(target=work, args=(k,)) for k in range(8)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    set_arith(isc, "ieee")
    assert not errors, errors


def build_shade_mock(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "instances_shade_mock")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", os.path.join(root, "tests", "cpp", "instances_shade_mock.cpp"), "-o", exe,
                           "-L" + os.path.join(root, "snail_amd"), "-lsnailhip", "-Wl,-rpath," + os.path.join(root, "snail_amd")])
    return exe


@pytest.mark.parametrize("arith,mode", ARITH)
def test_cpp_adapter_lit_image(torch_mod, tmp_path, arith, mode):
    """A C++ host in the reference's shape (tests/cpp/instances_shade_mock.cpp over snail::HipDBVH): the image Render(...) with gVals[1] = 0, then
    with gVals[7] = 1, is made on the device from the scene's lights and ambient -- the images and TreeStats equal the restatement -- and the
    mock's host Render stubs (which exit with status 3) are not reached.  The image is 90 x 53 with rows of 3 * 90 + 1 bytes."""
    import subprocess
    names, rot, tr, bi, _, _, cam, lights, cref = K.case("field")
    resx, resy = 90, 53
    isc, ref = device_scene(names, rot, tr, bi, cref)
    d = tmp_path
    for k, nm in enumerate(names):
        hb = blas(nm)[0].bvh
        hb.nodes.tofile(str(d / ("blas%d_nodes.bin" % k))); hb.tris.tofile(str(d / ("blas%d_tris.bin" % k)))
    xs, bs = isc.slot_transforms()
    isc.nodes().tofile(str(d / "top_nodes.bin")); xs.tofile(str(d / "xf12.bin")); bs.astype(np.int32).tofile(str(d / "blas_index.bin"))
    np.ascontiguousarray(cam.as_array13(), dtype=np.float32).tofile(str(d / "cam.bin"))
    np.ascontiguousarray(lights, dtype=np.float32).tofile(str(d / "lights7.bin"))
    depths = [blas(nm)[0].bvh.depth for nm in names]
    np.array([resx, resy, int(arith == "host_sse"), len(names)] + depths, dtype=np.int32).tofile(str(d / "meta.bin"))
    r = subprocess.run([build_shade_mock(tmp_path), str(d)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "instances shade adapter ok" in r.stdout, r.stdout + r.stderr
    assert "Render called" not in r.stdout
    stats = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in open(str(d / "stats.txt")).read().splitlines()}
    pitch = resx * 3 + 1
    for key, fname, refl in (("lit", "out_lit.bin", False), ("refl", "out_refl.bin", True)):
        dg = S.Diag()
        want, wst = S.ShadeRef(ref).render(cam.as_array13(), resx, resy, lights, reflections=refl, mode=mode, diag=dg)
        assert dg.hit_pixels >= resx * resy // 5 and dg.lit_pixels >= 100 and dg.occluded_pixels >= 100
        raw = np.fromfile(str(d / fname), dtype=np.uint8).reshape(resy, pitch)
        assert np.array_equal(raw[:, :resx * 3].reshape(resy, resx, 3), want), key
        assert (raw[:, resx * 3:] == 0xAB).all()            # nothing written past a row's pixels
        assert stats[key] == [int(wst[0]), int(wst[1]), int(wst[2]), int(wst[3])], (key, stats[key], wst)
