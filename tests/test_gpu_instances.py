"""Two-level instanced scenes on the MI355X (snail_amd.instances, include/snail_instances.h): the device top-level
walk against the existing BVH path (identity instance) and against the test-side restatement tests/dbvh_ref.py (top level restated,
inner level through the oracle's pinned BVH walks), in both arithmetics."""
import os
import threading
import types

import numpy as np
import pytest

from snail_amd import HostBVH, scenes, survey_camera
from snail_amd.instances import InstancedScene
from snail_amd.scene import Context, Scene, ShadowContext
from tests import dbvh_ref as R
from tests import instances_edges as E
from tests import oracle_lib as O
from tests import util as U

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
ARITH = [("ieee", O.MODE_IEEE), ("host_sse", O.MODE_SSE)]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_blas_cache = {}


def blas(name):
    """(HostBVH-built device Scene, OracleScene) of a BLAS: box, lancia (the reference's own mesh), chain (depth 63: the DEEP walk)"""
    if name not in _blas_cache:
        tv = E.blas_tris(name)     # (the triangles and the oracle scene live in tests/instances_edges.py, which the host tests share)
        _blas_cache[name] = (Scene(HostBVH.build(tv), 0), E.oracle(name), tv)
    return _blas_cache[name]


def make(names, n, seed, spread=1.0):
    """An InstancedScene over the BLASes `names` (instances cycle over them) and its restatement."""
    pairs = [blas(nm) for nm in names]
    lo = np.min([p[1].nodes[0]["bmin"] for p in pairs], axis=0)
    hi = np.max([p[1].nodes[0]["bmax"] for p in pairs], axis=0)
    rot, tr, bi = scenes.instance_field(lo, hi, n, seed=seed, n_blas=len(names))
    tr = (tr * np.float32(spread)).astype(np.float32)
    isc = InstancedScene([p[0] for p in pairs], rot, tr, bi)
    xs, bs = isc.slot_transforms()
    ref = R.Ref([p[1] for p in pairs], isc.nodes(), xs, bs)
    return isc, ref


def field_camera(isc):
    nd = isc.nodes()[0]
    return survey_camera(np.concatenate([nd["bmin"], nd["bmax"], nd["bmin"]]).reshape(1, 9))


def set_arith(isc, arith):
    for s in isc.blas:
        s.set_arith(arith)


def check_frame(isc, ref, cam, resx, resy, arith, mode):
    set_arith(isc, arith)
    st = isc.new_stats()
    t, u, v, inst, tri = isc.trace_primary(cam, resx, resy, stats=st)
    rt, ru, rv, rinst, rtri, rst = ref.render_primary(cam.as_array13(), resx, resy, mode=mode)
    U.assert_bit_equal(t.cpu().numpy(), rt, "t")
    U.assert_bit_equal(u.cpu().numpy(), ru, "u")
    U.assert_bit_equal(v.cpu().numpy(), rv, "v")
    assert np.array_equal(inst.cpu().numpy(), rinst), "instance"
    assert np.array_equal(tri.cpu().numpy(), rtri), "triId"
    assert np.array_equal(st.cpu().numpy().astype(np.uint64), rst), (st.cpu().numpy(), rst)
    return rt


@pytest.mark.parametrize("arith", ["ieee", "host_sse"])
@pytest.mark.parametrize("name", ["box", "atrium"])
def test_identity_instance_equals_the_bvh_path(torch_mod, name, arith):
    sc = blas(name)[0]
    isc = InstancedScene([sc], np.eye(3, dtype=np.float32)[None], np.zeros((1, 3), np.float32))
    set_arith(isc, arith)
    cam = U.camera_for(name, blas(name)[2])
    t, u, v, inst, tri = isc.trace_primary(cam, 256, 256)
    fr = sc.trace_primary(cam, 256, 256)
    for a, b, what in ((t, fr.t, "t"), (u, fr.u, "u"), (v, fr.v, "v"), (tri, fr.tri_id, "triId")):
        U.assert_bit_equal(a.cpu().numpy(), b.cpu().numpy(), what)
    assert not inst.cpu().numpy().any()
    assert np.isfinite(t.cpu().numpy()).sum() > 1000
    set_arith(isc, "ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
def test_fields_equal_the_restatement(torch_mod, arith, mode):
    # two BLASes mixed in one field
    isc, ref = make(["box", "lancia"], 24, seed=3, spread=0.1)
    rt = check_frame(isc, ref, field_camera(isc), 128, 96, arith, mode)
    rinst = ref.render_primary(field_camera(isc).as_array13(), 32, 32, mode=mode)[3]
    assert np.isfinite(rt).sum() > 20 and len(np.unique(rinst)) >= 2
    # overlapping instances: translations squeezed, so instances cross and closest-hit ties across instances happen
    isc2, ref2 = make(["box"], 16, seed=8, spread=0.002)
    check_frame(isc2, ref2, field_camera(isc2), 96, 64, arith, mode)
    # a camera inside an instance's box (the identity instance, last, sits at the origin)
    isc3, ref3 = make(["lancia"], 8, seed=5)
    from snail_amd import FPSCamera
    c = blas("lancia")[1].nodes[0]
    inside = ((c["bmin"] + c["bmax"]) * 0.5).astype(np.float32)
    check_frame(isc3, ref3, FPSCamera(inside, 0.3, 0.1).camera(), 96, 64, arith, mode)
    set_arith(isc, "ieee"); set_arith(isc2, "ieee"); set_arith(isc3, "ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
def test_leaves_of_several_instances(torch_mod, arith, mode):
    """a caller's tree whose leaves hold several instances (the binned SAH never builds one): every instance of a leaf is walked and
    counted (Intersection per instance)"""
    isc0, _ = make(["box", "lancia"], 7, seed=13, spread=0.3)
    xs, bs = isc0.slot_transforms()
    nodes = isc0.nodes()[:3].copy()
    nodes[0]["sub"], nodes[0]["aux"] = 1, 0
    nodes[1]["sub"], nodes[1]["aux"] = 0x80000000 | 0, 3
    nodes[2]["sub"], nodes[2]["aux"] = 0x80000000 | 3, 4
    for k, (a, b) in ((1, (0, 3)), (2, (3, 7))):
        lo = np.min(isc0.nodes()["bmin"], axis=0); hi = np.max(isc0.nodes()["bmax"], axis=0)
        nodes[k]["bmin"], nodes[k]["bmax"] = lo, hi
    isc = InstancedScene.from_tree(isc0.blas, nodes, xs, bs)
    ref = R.Ref([blas("box")[1], blas("lancia")[1]], nodes, xs, bs)
    check_frame(isc, ref, field_camera(isc0), 64, 64, arith, mode)
    set_arith(isc, "ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
def test_deep_blas_field(torch_mod, arith, mode):
    assert blas("chain")[1].depth > 62
    isc, ref = make(["chain", "box"], 6, seed=4, spread=0.05)
    check_frame(isc, ref, field_camera(isc), 64, 64, arith, mode)
    set_arith(isc, "ieee")


def _world(isc):
    return types.SimpleNamespace(nodes=isc.nodes())


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("shared,masked", [(True, False), (True, True), (False, False), (False, True)])
def test_generic_packets_equal_the_restatement(torch_mod, shared, masked, arith, mode):
    torch = torch_mod
    isc, ref = make(["box", "lancia"], 12, seed=21, spread=0.05)
    set_arith(isc, arith)
    for size, n_packets, coherent in ((1, 3, False), (3, 3, False), (16, 2, True), (64, 3, False)):
        org, d, idir, mask, dist, obj, bary = U.secondary_packets(_world(isc), None, 0, 0, n_packets, seed=size + 7 * shared + 3 * masked,
                                                                  shared=shared, masked=masked, size=size, coherent=coherent)
        if mode != O.MODE_IEEE:
            idir = R.inv(d + np.float32(0.00000001), mode)
        elem = np.full_like(obj, 5)
        dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
        ctx = Context(dev(org), dev(d), dev(idir), dev(dist), dev(obj), dev(bary), size=size, shared_origin=shared, mask=dev(mask))
        de = dev(elem)
        st = isc.new_stats()
        isc.traverse_primary(ctx, de, stats=st)
        rst = np.zeros(4, dtype=np.uint64)
        for p in range(n_packets):
            sl = slice(p * size, (p + 1) * size)
            po = org[p:p + 1].reshape(1, 3, 4) if shared else org[sl].reshape(size, 3, 4)
            rst += ref.traverse(po, d[sl].reshape(size, 3, 4), idir[sl].reshape(size, 3, 4), None if mask is None else mask[sl],
                                dist[sl], obj[sl], elem[sl], bary[sl], shared, False, mode)
        U.assert_bit_equal(ctx.distance.cpu().numpy(), dist, "distance %d" % size)
        assert np.array_equal(ctx.object.cpu().numpy(), obj), size
        assert np.array_equal(de.cpu().numpy(), elem), size
        U.assert_bit_equal(ctx.barycentric.cpu().numpy(), bary, "bary %d" % size)
        assert np.array_equal(st.cpu().numpy().astype(np.uint64), rst), (size, st.cpu().numpy(), rst)
    set_arith(isc, "ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
def test_shadow_packets_equal_the_restatement(torch_mod, arith, mode):
    torch = torch_mod
    isc, ref = make(["box", "lancia"], 12, seed=31, spread=0.05)
    set_arith(isc, arith)
    for size, n_packets in ((1, 3), (3, 3), (16, 3), (64, 3)):
        org, d, idir, dist = U.shadow_packets(_world(isc), n_packets, seed=size, size=size)
        if mode != O.MODE_IEEE:
            idir = R.inv(d + np.float32(0.00000001), mode)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        ctx = ShadowContext(dev(org), dev(d), dev(idir), dev(dist), size=size)
        st = isc.new_stats()
        isc.traverse_shadow(ctx, stats=st)
        rst = np.zeros(4, dtype=np.uint64)
        for p in range(n_packets):
            sl = slice(p * size, (p + 1) * size)
            po = np.repeat(org[p].reshape(1, 3, 1), 4, axis=2).astype(np.float32)
            rst += ref.traverse(po, d[sl].reshape(size, 3, 4), idir[sl].reshape(size, 3, 4), None, dist[sl], None, None, None, True, True, mode)
        U.assert_bit_equal(ctx.distance.cpu().numpy(), dist, "shadow distance %d" % size)
        assert (dist == -np.inf).sum() > 0
        assert np.array_equal(st.cpu().numpy().astype(np.uint64), rst), (size, st.cpu().numpy(), rst)
    set_arith(isc, "ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
def test_depth_frame_equals_shade_depth_of_the_restatement(torch_mod, arith, mode):
    isc, ref = make(["box"], 10, seed=12)
    set_arith(isc, arith)
    cam = field_camera(isc)
    frame = isc.render_depth(cam, 96, 64).cpu().numpy()
    rt = ref.render_primary(cam.as_array13(), 96, 64, mode=mode)[0]
    want = O.shade_depth(rt, mode=mode).reshape(64, 96, 3)
    assert np.array_equal(frame, want)
    set_arith(isc, "ieee")


def test_update_between_launches_on_one_stream(torch_mod):
    torch = torch_mod
    isc, ref = make(["box"], 12, seed=40)
    cam = field_camera(isc)
    s = torch.cuda.Stream()
    pairs = [blas("box")]
    lo, hi = pairs[0][1].nodes[0]["bmin"], pairs[0][1].nodes[0]["bmax"]
    rot2, tr2, bi2 = scenes.instance_field(lo, hi, 12, seed=41)
    with torch.cuda.stream(s):
        f1 = isc.trace_primary(cam, 64, 64, stream=s)
        isc.update(rot2, tr2, bi2, stream=s)
        f2 = isc.trace_primary(cam, 64, 64, stream=s)
    s.synchronize()
    xs, bs = isc.slot_transforms()
    ref2 = R.Ref([pairs[0][1]], isc.nodes(), xs, bs)
    # ... and an update to more instances than the handle's buffers hold (they are reallocated once the launches before it are done)
    rot3, tr3, bi3 = scenes.instance_field(lo, hi, 300, seed=42)
    with torch.cuda.stream(s):
        isc.update(rot3, tr3, bi3, stream=s)
        f3 = isc.trace_primary(cam, 64, 64, stream=s)
    s.synchronize()
    xs3, bs3 = isc.slot_transforms()
    ref3 = R.Ref([pairs[0][1]], isc.nodes(), xs3, bs3)
    assert len(xs3) == 300
    for f, r in ((f1, ref), (f2, ref2), (f3, ref3)):
        rt, ru, rv, rinst, rtri, _ = r.render_primary(cam.as_array13(), 64, 64)
        U.assert_bit_equal(f[0].cpu().numpy(), rt, "t")
        assert np.array_equal(f[3].cpu().numpy(), rinst) and np.array_equal(f[4].cpu().numpy(), rtri)


def test_threads_share_one_handle(torch_mod):
    torch = torch_mod
    isc, ref = make(["box", "lancia"], 16, seed=50)
    cam = field_camera(isc)
    want = ref.render_primary(cam.as_array13(), 64, 64)
    errors = []

    def work(k):
        try:
            s = torch.cuda.Stream()
            for _ in range(3):
                with torch.cuda.stream(s):
                    t, u, v, inst, tri = isc.trace_primary(cam, 64, 64, stream=s)
                s.synchronize()
                if not (np.array_equal(t.cpu().numpy().view(np.uint32), want[0].view(np.uint32)) and np.array_equal(tri.cpu().numpy(), want[4])
                        and np.array_equal(inst.cpu().numpy(), want[3])):
                    errors.append(k)
        except Exception as e:   # pragma: no cover
            errors.append(repr(e))

    th = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors


@pytest.mark.parametrize("arith,mode", ARITH)
def test_cpp_adapter_instanced(torch_mod, tmp_path, arith, mode):
    """A C++ host in the reference's shape (tests/cpp/instances_mock.cpp over snail::HipDBVH, mock DBVH / ObjectInstance / BVH types): the
    prefetched frame (BeginFrame + per-packet TraversePrimary(Context<1,0>) copies, frame TreeStats), Render(scene, camera, image, ...) with
    gVals[1] on the device, and the immediate TraversePrimary(Context<0,1>) / TraverseShadow paths all equal tests/dbvh_ref.py."""
    import subprocess
    from tests.test_instances_abi import build_instances_mock
    isc, ref = make(["box", "lancia"], 10, seed=61, spread=0.2)
    d = tmp_path
    resx, resy = 96, 64
    cam = field_camera(isc)
    names = ["box", "lancia"]
    for k, nm in enumerate(names):
        hb = blas(nm)[0].bvh
        hb.nodes.tofile(str(d / ("blas%d_nodes.bin" % k))); hb.tris.tofile(str(d / ("blas%d_tris.bin" % k)))
    xs, bs = isc.slot_transforms()
    isc.nodes().tofile(str(d / "top_nodes.bin")); xs.tofile(str(d / "xf12.bin")); bs.astype(np.int32).tofile(str(d / "blas_index.bin"))
    np.ascontiguousarray(cam.as_array13(), dtype=np.float32).tofile(str(d / "cam.bin"))
    n_ry, n_sh = 3, 3
    ro, rd, ri, rmask, rdist, robj, rbary = U.secondary_packets(_world(isc), None, 0, 0, n_ry, seed=62, shared=False, masked=True)
    for nm, a in (("ry_origin", ro), ("ry_dir", rd), ("ry_idir", ri), ("ry_mask", rmask), ("ry_dist", rdist)):
        a.tofile(str(d / (nm + ".bin")))
    so, sd, si, sdist = U.shadow_packets(_world(isc), n_sh, 63)
    for nm, a in (("sh_origin", so), ("sh_dir", sd), ("sh_idir", si), ("sh_dist", sdist)):
        a.tofile(str(d / (nm + ".bin")))
    depths = [blas(nm)[0].bvh.depth for nm in names]
    np.array([resx, resy, int(arith == "host_sse"), len(names), n_ry, n_sh] + depths, dtype=np.int32).tofile(str(d / "meta.bin"))
    r = subprocess.run([build_instances_mock(tmp_path), str(d)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "instances adapter ok" in r.stdout, r.stdout + r.stderr
    assert "host tile Render: prefetched %d x %d 1" % (resx, resy) in r.stdout
    stats = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in open(str(d / "stats.txt")).read().splitlines()}
    # prefetched frame
    rt, ru, rv, rinst, rtri, rst = ref.render_primary(cam.as_array13(), resx, resy, mode=mode)
    n = resx * resy
    raw = np.fromfile(str(d / "out_primary.bin"), dtype=np.uint8)
    planes = [raw[k * n * 4:(k + 1) * n * 4] for k in range(5)]
    U.assert_bit_equal(planes[0].view(np.float32).reshape(resy, resx), rt, "adapter t")
    U.assert_bit_equal(planes[1].view(np.float32).reshape(resy, resx), ru, "adapter u")
    U.assert_bit_equal(planes[2].view(np.float32).reshape(resy, resx), rv, "adapter v")
    assert np.array_equal(planes[3].view(np.int32).reshape(resy, resx), rinst)
    assert np.array_equal(planes[4].view(np.int32).reshape(resy, resx), rtri)
    assert stats["primary"] == [int(rst[0]), int(rst[1]), int(rst[3])]
    # the depth image on the device
    img = np.fromfile(str(d / "out_image.bin"), dtype=np.uint8).reshape(resy, resx, 3)
    assert np.array_equal(img, O.shade_depth(rt, mode=mode).reshape(resy, resx, 3))
    assert stats["image"] == [int(rst[0]), int(rst[1]), int(rst[2]), int(rst[3])]
    # immediate generic packets <0,1>
    wst = np.zeros(4, dtype=np.uint64)
    welem = np.zeros_like(robj)
    for p in range(n_ry):
        sl = slice(p * 64, (p + 1) * 64)
        wst += ref.traverse(ro[sl].reshape(64, 3, 4), rd[sl].reshape(64, 3, 4), ri[sl].reshape(64, 3, 4), rmask[sl], rdist[sl], robj[sl], welem[sl],
                            rbary[sl], False, False, mode)
    raw = np.fromfile(str(d / "out_ry.bin"), dtype=np.uint8)
    nq = n_ry * 64
    U.assert_bit_equal(raw[:nq * 16].view(np.float32).reshape(-1, 4), rdist, "rays dist")
    assert np.array_equal(raw[nq * 16:nq * 32].view(np.int32).reshape(-1, 4), robj)
    assert np.array_equal(raw[nq * 32:nq * 48].view(np.int32).reshape(-1, 4), welem)
    U.assert_bit_equal(raw[nq * 48:].view(np.float32).reshape(-1, 8), rbary, "rays bary")
    assert stats["rays"] == [int(wst[0]), int(wst[1]), int(wst[3])]
    # immediate shadow packets
    wst = np.zeros(4, dtype=np.uint64)
    for p in range(n_sh):
        sl = slice(p * 64, (p + 1) * 64)
        po = np.repeat(so[p].reshape(1, 3, 1), 4, axis=2).astype(np.float32)
        wst += ref.traverse(po, sd[sl].reshape(64, 3, 4), si[sl].reshape(64, 3, 4), None, sdist[sl], None, None, None, True, True, mode)
    U.assert_bit_equal(np.fromfile(str(d / "out_sh.bin"), dtype=np.float32).reshape(-1, 4), sdist, "shadow dist")
    assert stats["shadow"] == [int(wst[0]), int(wst[1]), int(wst[3])]
    set_arith(isc, "ieee")
