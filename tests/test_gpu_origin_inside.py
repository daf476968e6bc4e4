"""Primary packets skip the box test at nodes that CONTAIN the camera (snail_dev.inc: SNAIL_OIN_*, dev::relAux): the origin-relative node records
carry a "contains the origin" bit on such inner nodes, and the record-prefetching loop of dev::primaryPacket -- the octant statements of sign-coherent
packets and the plain statement -- does only the visit's scalar work there.

Everything is held against tests.oracle_lib, which tests every box: t, u, v, triId bit for bit and TreeStats for equality, in both arithmetics.  The
number of flagged records is computed here from the oracle's nodes by the rule of the fill kernel (inner node, relative near words <= 0, far words
>= 0, as float32) and compared with the workbench library's count over the very array the product library filled.

Scene atrium:0.05 (15 794 triangles, 9261 nodes, depth 17) at 328x200 = 21 x 13 packets, the last column cut.  Camera positions: the bench's (8 inner
nodes contain it); x moved onto node 1's bmin.x and y onto node 3's bmax.y (a relative word that is +0: the comparison's boundary; a LEAF contains
these points too and must not be flagged); the root's min corner (three zero words); a point one extent outside the root, looking at it (nothing flagged: the
ordinary visit); jittered positions."""
import ctypes as C

import numpy as np
import pytest

from snail_amd import FPSCamera, scenes
from snail_amd.camera import Camera
from tests import oracle_lib as O
from tests import util as U

pytestmark = pytest.mark.gpu

F = np.float32
NAME = "atrium:0.05"
RESX, RESY = 328, 200
ARITHS = [("ieee", O.MODE_IEEE), ("host_sse", O.MODE_SSE)]
# name -> (inner nodes, leaves) that contain the position, counted on the CPU for this tree (None: jittered, 8..11 inner)
CONTAINING = {"bench": (8, 0), "on_bmin_x_of_node_1": (11, 1), "on_bmax_y_of_node_3": (10, 1), "root_min_corner": (3, 0), "outside": (0, 0),
              "jitter0": None, "jitter1": None, "jitter2": None}
INSIDE = [k for k in CONTAINING if k != "outside"]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def pair():
    import torch      # before the library is loaded: both bring a HIP runtime, and torch's has to be the process's
    return U.scene_pair(NAME)


def position(case):
    tv, hb, osc = pair()
    n = osc.nodes
    base = np.asarray(scenes.atrium_camera()[0], dtype=F)
    if case == "bench":
        return base
    if case == "on_bmin_x_of_node_1":
        return np.array([n[1]["bmin"][0], base[1], base[2]], dtype=F)
    if case == "on_bmax_y_of_node_3":
        return np.array([base[0], n[3]["bmax"][1], base[2]], dtype=F)
    if case == "root_min_corner":
        return n[0]["bmin"].astype(F)
    if case == "outside":      # one extent in front of the root's z-min face, looking at the scene down +z
        c = (n[0]["bmin"] + n[0]["bmax"]) * F(0.5)
        return np.array([c[0], c[1], n[0]["bmin"][2] - (n[0]["bmax"][2] - n[0]["bmin"][2])], dtype=F)
    k = int(case[len("jitter"):])
    return (base + np.random.RandomState(50 + k).uniform(-0.4, 0.4, 3)).astype(F)


def camera_at(pos, axis_view=False):
    """the bench camera's orientation at `pos`; axis_view: looking down +z (ang = pitch = 0: right, up, front = the scene's axes)"""
    _, ang, pitch = scenes.atrium_camera()
    return FPSCamera(np.asarray(pos, dtype=F), 0.0 if axis_view else ang, 0.0 if axis_view else pitch).camera()


def camera_of(case):
    return camera_at(position(case), axis_view=case == "outside")


def containing(nodes, pos):
    """-> (inner, leaf) masks of the nodes whose box contains `pos` by the fill kernel's rule: bmin - o <= 0 and bmax - o >= 0 in float32"""
    o = np.asarray(pos, dtype=F)
    near, far = (nodes["bmin"] - o).astype(F), (nodes["bmax"] - o).astype(F)
    inside = (near <= 0).all(axis=1) & (far >= 0).all(axis=1)
    leaf = (nodes["sub"] & np.uint32(0x80000000)) != 0
    return inside & ~leaf, inside & leaf


def flag_count(sc, pos):
    """snail_debug_rel_flag_count of the workbench library on the product library's handle: the two are one set of sources, and the handle's
    cache already holds the array of `pos` when a frame from there was traced"""
    from snail_amd import _lib
    L = _lib.debug_lib()
    o = np.ascontiguousarray(pos, dtype=F)
    n = C.c_int(-1)
    rc = L.snail_debug_rel_flag_count(sc._h, _lib.ptr(o), C.addressof(n))
    assert rc == 0, L.snail_last_error().decode()
    return n.value


_scenes = {}


def gpu_scene(arith):
    from snail_amd.scene import Scene
    if arith not in _scenes:
        sc = Scene(pair()[1], 0)
        sc.set_arith(arith)
        _scenes[arith] = sc
    return _scenes[arith]


_refs = {}


def oracle_frame(cam, mode, rect=None):
    key = (cam.as_array13().tobytes(), mode, rect)
    if key not in _refs:
        _refs[key] = pair()[2].render_primary(cam.as_array13(), RESX, RESY, rect=rect, mode=mode, threads=8)
    return _refs[key]


def assert_frame(torch_mod, f, stats, ref, what, rect=None):
    torch_mod.cuda.synchronize()
    x0, y0, w, h = rect if rect else (0, 0, RESX, RESY)
    cut = lambda a: np.ascontiguousarray(a[y0:y0 + h, x0:x0 + w])
    for a, b, n in ((f.t, ref[0], "t"), (f.u, ref[1], "u"), (f.v, ref[2], "v"), (f.tri_id, ref[3], "triId")):
        U.assert_bit_equal(cut(a.cpu().numpy()), cut(b), "%s %s" % (what, n))
    if stats is not None:
        assert np.array_equal(stats.cpu().numpy().astype(np.uint64), ref[4]), (what, stats.cpu().numpy(), ref[4])
    assert np.isfinite(cut(ref[0])).sum() > 100, what


def test_the_tree_is_the_one_the_counts_were_made_for(torch_mod):
    tv, hb, osc = pair()
    assert len(tv) == 15794 and len(osc.nodes) == 9261 and osc.depth == 17
    assert hb.nodes.tobytes() == osc.nodes.tobytes()
    for case, want in CONTAINING.items():
        inner, leaf = containing(osc.nodes, position(case))
        got = (int(inner.sum()), int(leaf.sum()))
        if want is None:
            assert 8 <= got[0] <= 11, (case, got)
        else:
            assert got == want, (case, got)
        # the containing set is closed under "parent of": every containing node but the root is a child of a containing inner node
        kids = set()
        for i in np.flatnonzero(inner):
            kids |= {int(osc.nodes["sub"][i]), int(osc.nodes["sub"][i]) + 1}
        assert all(int(i) in kids for i in np.flatnonzero(inner | leaf) if i != 0), case


@pytest.mark.parametrize("arith,mode", ARITHS)
@pytest.mark.parametrize("case", list(CONTAINING))
def test_frames_from_inside_on_the_faces_and_outside_equal_the_oracle(torch_mod, case, arith, mode):
    tv, hb, osc = pair()
    sc = gpu_scene(arith)
    pos = position(case)
    cam = camera_of(case)
    stats = sc.new_stats()
    f = sc.trace_primary(cam, RESX, RESY, stats=stats)
    assert_frame(torch_mod, f, stats, oracle_frame(cam, mode), case)
    inner, leaf = containing(osc.nodes, pos)
    want = int(inner.sum())
    assert flag_count(sc, pos) == want, case                      # leaves are never flagged
    assert (want > 0) == (case in INSIDE), (case, want)           # no "inside" case passes with nothing flagged; outside takes the ordinary visit


def packet_kinds(cam):
    """per packet of the frame: do all its rays agree in the sign of idir on every axis (the octant statements) or not (the plain statement)"""
    cam13 = cam.as_array13()
    coh = []
    for y in range(0, RESY, 16):
        for x in range(0, RESX, 16):
            d, di = O.gen_packet(cam13, RESX, RESY, x, y, O.MODE_IEEE)
            assert np.isfinite(di).all()
            neg = np.signbit(di.reshape(64, 3, 4))
            coh.append(all(neg[:, k, :].all() or not neg[:, k, :].any() for k in range(3)))
    return np.array(coh)


@pytest.mark.parametrize("arith,mode", ARITHS)
def test_a_view_along_a_scene_axis_takes_the_path_in_both_statements(torch_mod, arith, mode):
    """front = +z, right = +x, up = +y: the frame's middle column and row of packets straddle x = 0 / y = 0 of the direction (not sign-coherent),
    the others lie in one octant each"""
    tv, hb, osc = pair()
    sc = gpu_scene(arith)
    pos = position("bench")
    cam = camera_at(pos, axis_view=True)
    assert np.array_equal(cam.right, [1, 0, 0]) and np.array_equal(cam.up, [0, 1, 0]) and np.array_equal(cam.front, [0, 0, 1])
    coh = packet_kinds(cam)
    assert coh.sum() >= 100 and (~coh).sum() >= 20, (int(coh.sum()), int((~coh).sum()))
    assert flag_count(sc, pos) == 8
    stats = sc.new_stats()
    f = sc.trace_primary(cam, RESX, RESY, stats=stats)
    assert_frame(torch_mod, f, stats, oracle_frame(cam, mode), "axis view")


@pytest.mark.parametrize("arith,mode", ARITHS)
def test_one_launch_of_four_frames_inside_outside_on_a_face_inside(torch_mod, arith, mode):
    sc = gpu_scene(arith)
    cams = [camera_of(c) for c in ("bench", "outside", "on_bmin_x_of_node_1", "jitter1")]
    outs = [sc.alloc_frame(RESX, RESY) for _ in cams]
    stats = sc.new_stats()
    sc.trace_primary_batch(cams, RESX, RESY, outs, stats=stats)
    refs = [oracle_frame(c, mode) for c in cams]
    for k, (f, ref) in enumerate(zip(outs, refs)):
        assert_frame(torch_mod, f, None, ref, "frame %d of the launch" % k)
    assert np.array_equal(stats.cpu().numpy().astype(np.uint64), sum(r[4] for r in refs))


@pytest.mark.parametrize("arith,mode", ARITHS)
def test_a_rect_a_packet_list_and_the_heat_map_kernel_from_inside(torch_mod, arith, mode):
    from tests.test_gpu_heatmap import dev_packet_stats, frame_xy, oracle_primary_packets
    tv, hb, osc = pair()
    sc = gpu_scene(arith)
    pos = position("on_bmax_y_of_node_3")
    cam = camera_at(pos)
    assert flag_count(sc, pos) == 10
    # a rect (packet-aligned, cut at the frame's right edge)
    rect = (160, 48, 168, 96)
    stats = sc.new_stats()
    f = sc.trace_primary(cam, RESX, RESY, rect=rect, stats=stats)
    assert_frame(torch_mod, f, stats, oracle_frame(cam, mode, rect), "rect", rect)
    # every packet of the frame as a shuffled list
    xy = frame_xy(RESX, RESY)
    np.random.RandomState(4).shuffle(xy)
    dxy = torch_mod.from_numpy(xy).cuda()
    stats = sc.new_stats()
    planes = sc.trace_packets(cam, RESX, RESY, dxy, stats=stats)
    fr = sc.alloc_frame(RESX, RESY)
    sc.packets_to_frame(dxy, planes, fr)
    assert_frame(torch_mod, fr, stats, oracle_frame(cam, mode), "packet list")
    # the per-packet counters of the heat-map instantiation (PSTATS) against the oracle's, packet by packet: 48x32 = six packets
    want, deferred = oracle_primary_packets(osc, cam.as_array13(), 48, 32, frame_xy(48, 32), mode)
    assert not deferred.any()
    got, tot = dev_packet_stats(torch_mod, sc, cam, 48, 32)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    assert np.array_equal(tot, want.sum(axis=0))


@pytest.mark.parametrize("arith,mode", ARITHS)
def test_a_light_at_the_cameras_position_shares_the_flagged_array(torch_mod, arith, mode):
    """the shadow walk towards a light AT the camera reads the camera's origin-relative array -- the one that carries the bits -- and must ignore them
    (its masked lanes fail every box)"""
    tv, hb, osc = pair()
    sc = gpu_scene(arith)
    pos = position("bench")
    cam = camera_at(pos)
    ext = float((osc.nodes[0]["bmax"] - osc.nodes[0]["bmin"]).max())
    lights = np.array([[pos[0], pos[1], pos[2], 1.0, 0.9, 0.8, 2.0 * ext]], dtype=F)
    want, wst = osc.render_whitted(cam.as_array13(), RESX, RESY, lights, mode=mode, threads=8)
    stats = sc.new_stats()
    got = sc.render_whitted(cam, RESX, RESY, lights, stats=stats).cpu().numpy()
    torch_mod.cuda.synchronize()
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(stats.cpu().numpy().astype(np.uint64), wst), (stats.cpu().numpy(), wst)
    assert want.max() > 40 and flag_count(sc, pos) == 8


@pytest.mark.parametrize("arith,mode", ARITHS)
def test_a_rebuilt_tree_is_flagged_and_traced_anew(torch_mod, arith, mode):
    from snail_amd.scene import Scene
    tv = pair()[0]
    tv2 = (tv * F(1.25)).astype(F)[::-1].copy()      # another tree: the boxes scale away from under the camera, the triangles come in another order
    sc = Scene.from_fast_dev(torch_mod.from_numpy(np.ascontiguousarray(tv)).cuda())
    sc.set_arith(arith)
    pos = position("bench")
    cam = camera_at(pos)
    trees, flagged = [], []
    try:
        for k, verts in enumerate((tv, tv2)):
            if k:
                info = sc.rebuild_fast_dev(torch_mod.from_numpy(verts).cuda())
                torch_mod.cuda.synchronize()
                assert info.cpu().numpy()[0] == 0
            hb = sc.bvh
            osc = O.OracleScene.from_arrays(hb.tris, hb.nodes, hb.depth, hb.perm)
            stats = sc.new_stats()
            f = sc.trace_primary(cam, RESX, RESY, stats=stats)
            ref = osc.render_primary(cam.as_array13(), RESX, RESY, mode=mode, threads=8)
            assert_frame(torch_mod, f, stats, ref, "tree %d" % k)
            inner, leaf = containing(osc.nodes, pos)
            assert flag_count(sc, pos) == int(inner.sum()) and inner.sum() > 0, k
            trees.append(hb.nodes.tobytes())
            flagged.append([np.concatenate([n["bmin"], n["bmax"]]).tobytes() for n in osc.nodes[inner]])
        assert trees[0] != trees[1]
        assert not set(flagged[0]) & set(flagged[1])      # no box that contains the camera is common to the two trees: a stale array could not pass
    finally:
        sc.close()
