"""The instanced walk on the MI355X at its edges (snail_amd/csrc/instances.inc: k_inst_frame, k_inst_trace, k_inst_occl, instWalk,
instCollide; instancesPrimary of instances_host.inc) against the restatement tests/dbvh_ref.py, bit for bit in both arithmetics: partial
packets with guarded planes, rects, packet lists and NULL planes, top-level trees at the depth limit, every sign octant, exact
rotations, far translations, exact duplicates and singular directions.  The cases are those of tests/instances_edges.py;
tests/test_instances_edges_host.py proves on the host that each reaches the edge it is named for."""
import numpy as np
import pytest

from snail_amd import HostBVH, _lib, scenes
from snail_amd.instances import InstancedScene
from snail_amd.scene import Context, Scene, ShadowContext
from tests import dbvh_ref as R
from tests import instances_edges as E
from tests import oracle_lib as O
from tests import util as U
from tests.test_gpu_instances import ARITH, blas, set_arith
from tests.test_gpu_instances_rebuild import check_rebuild

pytestmark = pytest.mark.gpu
SENTINEL = -7
FN_PRIMARY = "snail_instances_trace_primary_dev"
FN_PACKETS = "snail_instances_trace_packets_dev"


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_scenes, _devices = {}, {}


def scene_of(name):
    """the device Scene of a BLAS: tests/test_gpu_instances.py::blas's where it has one, the unit box otherwise"""
    if name in ("box", "lancia", "chain"):
        return blas(name)[0]
    if name not in _scenes:
        _scenes[name] = Scene(HostBVH.build(E.blas_tris(name)), 0)
    return _scenes[name]


def device(case):
    """The case on the device (host build, or the caller's tree), holding exactly the tree and records the host tests looked at."""
    if case.key not in _devices:
        sc = [scene_of(nm) for nm in case.names]
        isc = InstancedScene.from_tree(sc, case.nodes, case.xs, case.bs) if case.tree else InstancedScene(sc, case.rot, case.tr, case.bi)
        assert isc.nodes().tobytes() == case.nodes.tobytes()
        xs, bs = isc.slot_transforms()
        assert xs.tobytes() == case.xs.tobytes() and bs.tobytes() == case.bs.tobytes()
        _devices[case.key] = isc
    return _devices[case.key]


def equal_planes(got, want, what=""):
    """(t, u, v, inst, tri): t, u, v as bits, ids exactly"""
    for a, b, nm in zip(got[:3], want[:3], "tuv"):
        U.assert_bit_equal(np.asarray(a), np.asarray(b), "%s %s" % (what, nm))
    assert np.array_equal(got[3], want[3]), what + " instance"
    assert np.array_equal(got[4], want[4]), what + " triId"


def check_frame(isc, case, cam, resx, resy, mode, what=""):
    st = isc.new_stats()
    got = [x.cpu().numpy() for x in isc.trace_primary(cam, resx, resy, stats=st)]
    want = E.expected_frame(case, cam, resx, resy, mode)
    equal_planes(got, want, what)
    assert np.array_equal(st.cpu().numpy().astype(np.uint64), want[5]), (what, st.cpu().numpy(), want[5])
    return want


class Planes:
    """Five output planes of n + 4096 elements each and a stats word, prefilled: what a store out of bounds would disturb."""

    def __init__(self, torch, n, stats_fill=0):
        d = torch.device("cuda", 0)
        self.n = n
        self.f = [torch.full((n + 4096,), float(SENTINEL), dtype=torch.float32, device=d) for _ in range(3)]
        self.i = [torch.full((n + 4096,), SENTINEL, dtype=torch.int32, device=d) for _ in range(2)]
        self.stats = torch.full((4,), stats_fill, dtype=torch.int64, device=d)
        self.stats_fill = stats_fill

    def all(self):
        return self.f + self.i

    def numpy(self):
        return [x.cpu().numpy() for x in self.all()]

    def assert_untouched(self, start=0):
        for k, x in enumerate(self.numpy()):
            assert (x[start:] == SENTINEL).all(), "plane %d written at or after element %d" % (k, start)

    def assert_stats_untouched(self):
        assert (self.stats.cpu().numpy() == self.stats_fill).all()


def primary_raw(isc, cam, resx, resy, rect, pl, use=(1, 1, 1, 1, 1)):
    cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32)
    p = [_lib.ptr(x) if u else None for x, u in zip(pl.all(), use)]
    return _lib.lib().snail_instances_trace_primary_dev(isc._h, _lib.ptr(cam13), resx, resy, rect[0], rect[1], rect[2], rect[3], p[0], p[1], p[2], p[3], p[4],
                                                        _lib.ptr(pl.stats), None)


def packets_raw(isc, cam, resx, resy, xy, n, pl, use=(1, 1, 1, 1, 1)):
    cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32)
    p = [_lib.ptr(x) if u else None for x, u in zip(pl.all(), use)]
    return _lib.lib().snail_instances_trace_packets_dev(isc._h, _lib.ptr(cam13), resx, resy, _lib.ptr(xy), n, p[0], p[1], p[2], p[3], p[4], _lib.ptr(pl.stats), None)


def last_error():
    return _lib.lib().snail_last_error().decode()


# ---- partial frames ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("size", E.PARTIAL_SIZES)
def test_partial_frames_with_guarded_planes(torch_mod, size, arith, mode):
    resx, resy = size
    case, cam = E.blob(), E.blob_camera()
    isc = device(case)
    set_arith(isc, arith)
    pl = Planes(torch_mod, resx * resy)
    assert primary_raw(isc, cam, resx, resy, (0, 0, resx, resy), pl) == 0, last_error()
    torch_mod.cuda.synchronize()
    want = E.expected_frame(case, cam, resx, resy, mode)
    got = pl.numpy()
    equal_planes([g[:resx * resy].reshape(resy, resx) for g in got], want, "%dx%d" % size)       # a store past a row's end shows in the next row
    pl.assert_untouched(resx * resy)                                                             # ... past the last row, in the tail
    assert np.array_equal(pl.stats.cpu().numpy().astype(np.uint64), want[5])
    set_arith(isc, "ieee")


# ---- rects ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("rect", E.RECTS)
def test_rects(torch_mod, rect, arith, mode):
    resx, resy = E.RECT_FRAME
    case, cam = E.blob(), E.blob_camera()
    isc = device(case)
    set_arith(isc, arith)
    pl = Planes(torch_mod, resx * resy)
    assert primary_raw(isc, cam, resx, resy, rect, pl) == 0, last_error()
    torch_mod.cuda.synchronize()
    want = E.expected_frame(case, cam, resx, resy, mode, rect=rect)
    x0, y0, w, h = rect
    inside = np.zeros((resy, resx), dtype=bool)
    inside[y0:min(resy, y0 + h), x0:min(resx, x0 + w)] = True
    assert inside.any()
    got = pl.numpy()
    frames = [g[:resx * resy].reshape(resy, resx) for g in got]
    equal_planes([f[inside] for f in frames], [wv[inside] for wv in want[:5]], "rect %s" % (rect,))
    for k, f in enumerate(frames):
        assert (f[~inside] == SENTINEL).all(), "plane %d written outside the clipped rect %s" % (k, rect)
    pl.assert_untouched(resx * resy)
    assert np.array_equal(pl.stats.cpu().numpy().astype(np.uint64), want[5])
    set_arith(isc, "ieee")


@pytest.mark.parametrize("bad", [dict(x0=8), dict(y0=24), dict(w=0), dict(h=-1), dict(x0=-16), dict(y0=-16), dict(x0=-16, y0=-16), dict(resx=0)])
def test_rect_refusals(torch_mod, bad):
    resx, resy = E.RECT_FRAME
    isc = device(E.blob())
    a = dict(resx=resx, resy=resy, x0=16, y0=16, w=40, h=30)
    a.update(bad)
    pl = Planes(torch_mod, resx * resy, stats_fill=5)
    rc = primary_raw(isc, E.blob_camera(), a["resx"], a["resy"], (a["x0"], a["y0"], a["w"], a["h"]), pl)
    torch_mod.cuda.synchronize()
    assert rc != 0 and FN_PRIMARY in last_error(), (rc, last_error())
    pl.assert_untouched()
    pl.assert_stats_untouched()


# ---- packet lists ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith,mode", ARITH)
def test_packet_lists_and_null_planes(torch_mod, arith, mode):
    torch = torch_mod
    resx, resy = E.RECT_FRAME
    case, cam = E.blob(), E.blob_camera()
    isc = device(case)
    set_arith(isc, arith)
    xy = E.packet_list(resx, resy)
    n = len(xy)
    dxy = torch.from_numpy(xy).cuda()
    want = E.expected_packets(case, cam, resx, resy, xy, mode)
    pl = Planes(torch, n * 256)
    assert packets_raw(isc, cam, resx, resy, dxy, n, pl) == 0, last_error()
    torch.cuda.synchronize()
    equal_planes([g[:n * 256].reshape(n, 256) for g in pl.numpy()], want, "packet list")
    pl.assert_untouched(n * 256)
    assert np.array_equal(pl.stats.cpu().numpy().astype(np.uint64), want[5])
    # the wrapper (InstancedScene.trace_packets) is the same call
    st = isc.new_stats()
    got = [x.cpu().numpy() for x in isc.trace_packets(cam, resx, resy, dxy, stats=st)]
    equal_planes(got, want, "trace_packets")
    assert np.array_equal(st.cpu().numpy().astype(np.uint64), want[5])
    # NULL planes: the planes given are the reference's, the others' memory is not touched, the stats are those of the full call
    for use in ((0, 0, 0, 0, 1), (1, 0, 0, 1, 0)):
        p2 = Planes(torch, n * 256)
        assert packets_raw(isc, cam, resx, resy, dxy, n, p2, use) == 0, last_error()
        torch.cuda.synchronize()
        for k, g in enumerate(p2.numpy()):
            if use[k]:
                assert np.array_equal(g[:n * 256].reshape(n, 256).view(np.uint32), np.ascontiguousarray(want[k]).view(np.uint32)), (use, k)
                assert (g[n * 256:] == SENTINEL).all()
            else:
                assert (g == SENTINEL).all(), (use, k)
        assert np.array_equal(p2.stats.cpu().numpy().astype(np.uint64), want[5]), use
    # ... and of the frame form
    wantf = E.expected_frame(case, cam, resx, resy, mode)
    for use in ((0, 0, 0, 0, 1), (1, 0, 0, 1, 0)):
        p3 = Planes(torch, resx * resy)
        assert primary_raw(isc, cam, resx, resy, (0, 0, resx, resy), p3, use) == 0, last_error()
        torch.cuda.synchronize()
        for k, g in enumerate(p3.numpy()):
            if use[k]:
                assert np.array_equal(g[:resx * resy].reshape(resy, resx).view(np.uint32), np.ascontiguousarray(wantf[k]).view(np.uint32)), (use, k)
                assert (g[resx * resy:] == SENTINEL).all()
            else:
                assert (g == SENTINEL).all(), (use, k)
        assert np.array_equal(p3.stats.cpu().numpy().astype(np.uint64), wantf[5]), use
    set_arith(isc, "ieee")


def test_packet_list_empty_and_null(torch_mod):
    torch = torch_mod
    resx, resy = E.RECT_FRAME
    isc, cam = device(E.blob()), E.blob_camera()
    dxy = torch.from_numpy(E.packet_list(resx, resy)).cuda()
    pl = Planes(torch, 256, stats_fill=5)
    assert packets_raw(isc, cam, resx, resy, dxy, 0, pl) == 0          # nothing to do: no error, nothing written
    torch.cuda.synchronize()
    pl.assert_untouched()
    pl.assert_stats_untouched()
    rc = packets_raw(isc, cam, resx, resy, None, 4, pl)
    torch.cuda.synchronize()
    assert rc != 0 and FN_PACKETS in last_error() and "null" in last_error()
    pl.assert_untouched()
    pl.assert_stats_untouched()


# ---- generic and shadow packets over a case ---------------------------------------------------------------------------------------------------
def check_generic(torch, isc, ref, arrays, size, shared, mode, what):
    org, d, idir, mask, dist, obj, bary = [None if a is None else a.copy() for a in arrays]
    elem = np.full_like(obj, 5)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ctx = Context(dev(org), dev(d), dev(idir), dev(dist), dev(obj), dev(bary), size=size, shared_origin=shared, mask=dev(mask))
    de = dev(elem)
    st = isc.new_stats()
    isc.traverse_primary(ctx, de, stats=st)
    rst = E.ref_generic(ref, org, d, idir, mask, dist, obj, elem, bary, size, shared, mode)
    U.assert_bit_equal(ctx.distance.cpu().numpy(), dist, what + " distance")
    assert np.array_equal(ctx.object.cpu().numpy(), obj), what + " object"
    assert np.array_equal(de.cpu().numpy(), elem), what + " element"
    if bary is not None:
        U.assert_bit_equal(ctx.barycentric.cpu().numpy(), bary, what + " bary")
    assert np.array_equal(st.cpu().numpy().astype(np.uint64), rst), (what, st.cpu().numpy(), rst)
    return dist


def check_shadow(torch, isc, ref, arrays, size, mode, what):
    org, d, idir, dist = [a.copy() for a in arrays]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ctx = ShadowContext(dev(org), dev(d), dev(idir), dev(dist), size=size)
    st = isc.new_stats()
    isc.traverse_shadow(ctx, stats=st)
    rst = E.ref_shadow(ref, org, d, idir, dist, size, mode)
    U.assert_bit_equal(ctx.distance.cpu().numpy(), dist, what + " shadow distance")
    assert np.array_equal(st.cpu().numpy().astype(np.uint64), rst), (what, st.cpu().numpy(), rst)
    return dist


def packets_over(case, size, shared, masked, mode, seed, n_packets=3, coherent=False):
    org, d, idir, mask, dist, obj, bary = U.secondary_packets(case.world(), None, 0, 0, n_packets, seed=seed, shared=shared, masked=masked, size=size,
                                                              coherent=coherent)
    if mode != O.MODE_IEEE:
        idir = R.inv(d + E.EPS, mode)
    return org, d, idir, mask, dist, obj, bary


def shadows_over(case, size, mode, seed, n_packets=3):
    org, d, idir, dist = U.shadow_packets(case.world(), n_packets, seed=seed, size=size)
    if mode != O.MODE_IEEE:
        idir = R.inv(d + E.EPS, mode)
    return org, d, idir, dist


# ---- depth ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("far_first", [False, True])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_comb_64_frames(torch_mod, axis, far_first, arith, mode):
    case = E.comb(64, axis, far_first)
    isc = device(case)
    set_arith(isc, arith)
    for which, cam in E.comb_cameras(case, axis).items():
        R.Ref.max_stack = 0
        want = check_frame(isc, case, cam, 32, 32, mode, "comb %s" % which)
        assert np.isfinite(want[0]).sum() > 20
    set_arith(isc, "ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
def test_comb_63_frames(torch_mod, arith, mode):
    case = E.comb(63, 2, True)
    isc = device(case)
    set_arith(isc, arith)
    for which, cam in E.comb_cameras(case, 2).items():
        check_frame(isc, case, cam, 32, 32, mode, "comb 63 %s" % which)
    set_arith(isc, "ieee")


def test_comb_65_is_refused_before_any_launch(torch_mod):
    case = E.comb(65, 0, True)
    with pytest.raises(_lib.SnailError):
        InstancedScene.from_tree([scene_of("box")], case.nodes, case.xs, case.bs)
    assert "depth" in last_error() and "snail_instances_create" in last_error(), last_error()


@pytest.mark.parametrize("arith,mode", ARITH)
def test_comb_64_packets(torch_mod, arith, mode):
    case = E.comb(64, 1, True)
    isc = device(case)
    set_arith(isc, arith)
    for size in (1, 3, 64):
        for shared, masked in ((True, False), (True, True), (False, False), (False, True)):
            arrays = packets_over(case, size, shared, masked, mode, seed=size + 7 * shared + 3 * masked)
            check_generic(torch_mod, isc, case.ref(), arrays, size, shared, mode, "comb %d %s %s" % (size, shared, masked))
        check_shadow(torch_mod, isc, case.ref(), shadows_over(case, size, mode, seed=size), size, mode, "comb %d" % size)
    set_arith(isc, "ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
def test_comb_64_over_the_deep_blas(torch_mod, arith, mode):
    """the top level at its depth limit over a BLAS whose own depth takes the DEEP kernels"""
    assert E.oracle("chain").depth > 62
    case, cams = E.chain_comb()
    isc = device(case)
    set_arith(isc, arith)
    for which in ("low", "side"):
        check_frame(isc, case, cams[which], 32, 16, mode, "chain comb %s" % which)
    set_arith(isc, "ieee")


# ---- octants --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith,mode", ARITH)
def test_every_sign_octant_of_the_top_level(torch_mod, arith, mode):
    case = E.octant_field()
    isc = device(case)
    set_arith(isc, arith)
    for k, cam in enumerate(E.octant_cameras(case)):
        check_frame(isc, case, cam, 32, 32, mode, "octant %d" % k)
    set_arith(isc, "ieee")


# ---- exact rotations ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith,mode", ARITH)
def test_exact_rotations(torch_mod, arith, mode):
    case, cam = E.rotation_field(), E.rotation_camera()
    isc = device(case)
    set_arith(isc, arith)
    check_frame(isc, case, cam, 96, 64, mode, "rotations 96x64")
    check_frame(isc, case, cam, 33, 17, mode, "rotations 33x17")
    for size in (1, 16, 64):
        for shared, masked in ((True, False), (False, True)):
            arrays = packets_over(case, size, shared, masked, mode, seed=40 + size, coherent=size == 16)
            check_generic(torch_mod, isc, case.ref(), arrays, size, shared, mode, "rotations %d %s" % (size, shared))
        check_shadow(torch_mod, isc, case.ref(), shadows_over(case, size, mode, seed=50 + size), size, mode, "rotations %d" % size)
    set_arith(isc, "ieee")


# ---- far field ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("k", E.FAR_K)
def test_far_field(torch_mod, k, arith, mode):
    for axes in E.FAR_AXES:
        case, cam, _, _ = E.far_field(k, axes)
        isc = device(case)
        set_arith(isc, arith)
        check_frame(isc, case, cam, 64, 48, mode, "far %d %s" % (k, axes))
        check_shadow(torch_mod, isc, case.ref(), shadows_over(case, 64, mode, seed=k), 64, mode, "far %d %s" % (k, axes))
        check_shadow(torch_mod, isc, case.ref(), shadows_over(case, 3, mode, seed=k + 1), 3, mode, "far %d %s" % (k, axes))
        set_arith(isc, "ieee")


# ---- duplicates -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith,mode", ARITH)
def test_duplicates_host_built_and_rebuilt_on_the_device(torch_mod, arith, mode):
    rot, tr, bi = scenes.instance_field((-1, -1, -1), (1, 1, 1), 5, seed=77)
    rebuilt = InstancedScene([scene_of("box")], rot, tr, bi)
    for case, m in E.duplicates():
        cam = E.duplicates_camera(case)
        isc = device(case)
        set_arith(isc, arith)
        check_frame(isc, case, cam, 64, 48, mode, case.key)
        # the same tree from update_dev: byte-equal to the host builder's, and the same frame
        nodes, depth, perm = check_rebuild(torch_mod, rebuilt, case.xf, case.bi)
        assert nodes.tobytes() == case.nodes.tobytes() and np.array_equal(perm, case.perm)
        check_frame(rebuilt, case, cam, 64, 48, mode, case.key + " rebuilt")
    set_arith(rebuilt, "ieee")
    rebuilt.close()


# ---- singular packets -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("size", [64, 16])
def test_singular_packets(torch_mod, size, arith, mode):
    case = E.singular_field()
    isc = device(case)
    set_arith(isc, arith)
    for shared, masked in ((True, False), (True, True), (False, False), (False, True)):
        arrays = E.singular_packets(case, size, shared, masked, mode)[:7]
        dist = check_generic(torch_mod, isc, case.ref(), arrays, size, shared, mode, "singular %d %s %s" % (size, shared, masked))
        assert np.isfinite(dist).sum() > 0       # (tests/test_instances_edges_host.py holds what the singular lanes reach)
    # without barycentrics: the kernels' other instantiation
    arrays = list(E.singular_packets(case, size, True, False, mode)[:7])
    arrays[6] = None
    check_generic(torch_mod, isc, case.ref(), arrays, size, True, mode, "singular %d no bary" % size)
    dist = check_shadow(torch_mod, isc, case.ref(), E.singular_shadow_packets(case, size, mode)[:4], size, mode, "singular %d" % size)
    assert (dist == -np.inf).sum() > 0
    set_arith(isc, "ieee")
