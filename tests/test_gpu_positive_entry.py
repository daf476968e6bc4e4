"""Primary packets drop the clamp max(tn, 0) at nodes whose origin-relative record proves tn >= 0 (snail_dev.inc: SNAIL_POSENTRY_*, dev::relAux): word 7 of
every inner and leaf record carries bit 25 + c when its relative near word c is > 0 and bit 28 + c when its far word c is < 0, and each of the eight
octant statements of sign-coherent packets tests its own three bits: set -> the visit without the four v_max_f32; none set -> an out-of-line copy
that tests the "contains the origin" bit and otherwise runs the full visit.  A leaf's triangle count shares the word and is masked where it is handed
to the leaf code, in every walk of the loop (the shadow walk reads the same arrays and must ignore the bits).

Everything is held against tests.oracle_lib, which clamps at every box: t, u, v, triId bit for bit and TreeStats for equality, in both arithmetics.
The six per-bit record counts come from numpy over the oracle's nodes (float32(bmin - o) > 0, float32(bmax - o) < 0, leaves included) and are
compared with the workbench library's counts over the very array the product library filled.

Scene, size, positions and helpers are those of tests/test_gpu_origin_inside.py (atrium:0.05, 328x200).  Views: the bench view (octants 0, 2, 4, 6);
the bench position looking down +z (octants 0..3) and down -z (4..7).  A numpy walk of this file (no distance culling: a superset of the kernel's
visits, the same node set the counts of the octants were made with) sorts each coherent packet's visits into fast (an octant bit set), flagged-inside
and slow (neither), and the test asserts that every one of the eight octants sees all three kinds before any frame is compared."""
import ctypes as C
import math

import numpy as np
import pytest

from snail_amd import FPSCamera
from tests import oracle_lib as O
from tests import util as U
from tests.test_gpu_origin_inside import (ARITHS, RESX, RESY, assert_frame, camera_at, camera_of, containing, flag_count, gpu_scene, oracle_frame, pair,
                                          position)

pytestmark = pytest.mark.gpu

F = np.float32
VIEWS = ["bench", "plus_z", "minus_z", "on_bmin_x_of_node_1", "on_bmax_y_of_node_3", "root_min_corner", "outside"]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def view(case):
    """-> (position, camera)"""
    if case == "plus_z":
        return position("bench"), camera_at(position("bench"), axis_view=True)
    if case == "minus_z":
        return position("bench"), FPSCamera(position("bench"), math.pi, 0.0).camera()
    return position(case), camera_of(case)


def axis_bits(nodes, pos):
    """-> bool [n, 6]: near x, y, z > 0, far x, y, z < 0 of float32(box - pos): bits 25..30 of a relative record's word 7"""
    o = np.asarray(pos, dtype=F)
    return np.concatenate([(nodes["bmin"] - o).astype(F) > 0, (nodes["bmax"] - o).astype(F) < 0], axis=1)


def axis_flag_count(sc, pos):
    from snail_amd import _lib
    L = _lib.debug_lib()
    o = np.ascontiguousarray(pos, dtype=F)
    out = (C.c_int * 6)(*([-1] * 6))
    rc = L.snail_debug_rel_axis_flag_count(sc._h, _lib.ptr(o), C.addressof(out))
    assert rc == 0, L.snail_last_error().decode()
    return list(out)


def check_bits(sc, nodes, pos, what):
    bits = axis_bits(nodes, pos)
    inner, leaf = containing(nodes, pos)
    assert not bits[inner | leaf].any(), what                      # a box that contains the origin has none of the six
    assert axis_flag_count(sc, pos) == [int(x) for x in bits.sum(axis=0)], what
    assert flag_count(sc, pos) == int(inner.sum()), what           # the "contains the origin" bit keeps its meaning
    return bits


_kinds = {}


def visit_kinds(case):
    """The frame's packets walked in numpy with the kernel's products (float32, near / far plane by the packet's octant; every box tested with the
    clamp, distance = inf) -> ({octant: [packets, fast visits, slow visits, flagged-inside visits]}, non-coherent packets)"""
    if case in _kinds:
        return _kinds[case]
    nodes = pair()[2].nodes
    pos, cam = view(case)
    o = np.asarray(pos, dtype=F)
    near, far = (nodes["bmin"] - o).astype(F), (nodes["bmax"] - o).astype(F)
    bits = axis_bits(nodes, pos)
    inside = containing(nodes, pos)[0]
    isleaf = (nodes["sub"] & np.uint32(0x80000000)) != 0
    cam13 = cam.as_array13()
    per, plain = {}, 0
    for y in range(0, RESY, 16):
        for x in range(0, RESX, 16):
            d, di = O.gen_packet(cam13, RESX, RESY, x, y, O.MODE_IEEE)
            di = di.reshape(64, 3, 4).transpose(0, 2, 1).reshape(256, 3)
            neg = np.signbit(di)
            if not all(neg[:, k].all() or not neg[:, k].any() for k in range(3)):
                plain += 1
                continue
            s = neg[0]
            row = per.setdefault(int(s[0]) | int(s[1]) << 1 | int(s[2]) << 2, [0, 0, 0, 0])
            row[0] += 1
            pick = [3 + k if s[k] else k for k in range(3)]        # the octant's bit per axis
            stack = [0]
            while stack:
                i = stack.pop()
                row[3 if inside[i] else 1 if bits[i][pick].any() else 2] += 1
                pn, pf = np.where(s, far[i], near[i]), np.where(s, near[i], far[i])
                with np.errstate(invalid="ignore", over="ignore"):
                    tn, tf = (di * pn).max(axis=1), (di * pf).min(axis=1)
                    hit = (tf - np.maximum(tn, F(0))) >= 0
                if bits[i][pick].any():
                    assert (tn >= 0).all()                           # what the fast visit rests on
                if hit.any() and not isleaf[i]:
                    stack += [int(nodes["sub"][i]), int(nodes["sub"][i]) + 1]
    _kinds[case] = (per, plain)
    return _kinds[case]


def test_every_octant_statement_sees_fast_slow_and_flagged_inside_visits(torch_mod):
    assert len(pair()[2].nodes) == 9261
    per, plain = visit_kinds("bench")
    assert sorted(per) == [0, 2, 4, 6] and plain == 33, (per, plain)
    seen = {}
    for case, octs in (("plus_z", [0, 1, 2, 3]), ("minus_z", [4, 5, 6, 7])):
        per, plain = visit_kinds(case)
        assert sorted(per) == octs and plain == 33, (case, per, plain)
        seen.update(per)
    for o, (packets, fast, slow, ins) in seen.items():
        assert packets == 60 and fast >= 1000 and slow >= 100 and ins == 8 * packets, (o, packets, fast, slow, ins)
    per, plain = visit_kinds("outside")
    assert all(r[3] == 0 and r[1] > 20 * r[2] for r in per.values()), per    # nothing flagged inside, almost everything fast


@pytest.mark.parametrize("arith,mode", ARITHS)
@pytest.mark.parametrize("case", VIEWS)
def test_frames_and_bit_counts_equal_the_oracle(torch_mod, case, arith, mode):
    osc = pair()[2]
    sc = gpu_scene(arith)
    pos, cam = view(case)
    stats = sc.new_stats()
    f = sc.trace_primary(cam, RESX, RESY, stats=stats)
    assert_frame(torch_mod, f, stats, oracle_frame(cam, mode), case)
    bits = check_bits(sc, osc.nodes, pos, case)
    isleaf = (osc.nodes["sub"] & np.uint32(0x80000000)) != 0
    assert bits[isleaf].any() and bits[~isleaf].any(), case         # leaves carry the bits too
    if case.startswith("on_"):
        # a relative word that is exactly 0 sets no bit, and a leaf contains the point: its visit takes the slow path with its count intact
        k = 0 if "bmin_x" in case else 4
        i = 1 if "bmin_x" in case else 3
        rel = (np.concatenate([osc.nodes["bmin"][i], osc.nodes["bmax"][i]]) - np.tile(pos, 2)).astype(F)
        assert rel[k] == 0 and not bits[i][k], case
        assert containing(osc.nodes, pos)[1].sum() == 1, case


@pytest.mark.parametrize("arith,mode", ARITHS)
def test_one_launch_of_four_frames_with_different_cameras(torch_mod, arith, mode):
    sc = gpu_scene(arith)
    cams = [view(c)[1] for c in ("minus_z", "outside", "on_bmin_x_of_node_1", "plus_z")]
    outs = [sc.alloc_frame(RESX, RESY) for _ in cams]
    stats = sc.new_stats()
    sc.trace_primary_batch(cams, RESX, RESY, outs, stats=stats)
    refs = [oracle_frame(c, mode) for c in cams]
    for k, (f, ref) in enumerate(zip(outs, refs)):
        assert_frame(torch_mod, f, None, ref, "frame %d of the launch" % k)
    assert np.array_equal(stats.cpu().numpy().astype(np.uint64), sum(r[4] for r in refs))


@pytest.mark.parametrize("arith,mode", ARITHS)
def test_a_rect_a_packet_list_and_the_heat_map_kernel(torch_mod, arith, mode):
    from tests.test_gpu_heatmap import dev_packet_stats, frame_xy, oracle_primary_packets
    osc = pair()[2]
    sc = gpu_scene(arith)
    pos, cam = view("minus_z")
    rect = (160, 48, 168, 96)      # packet-aligned, cut at the frame's right edge
    stats = sc.new_stats()
    f = sc.trace_primary(cam, RESX, RESY, rect=rect, stats=stats)
    assert_frame(torch_mod, f, stats, oracle_frame(cam, mode, rect), "rect", rect)
    xy = frame_xy(RESX, RESY)
    np.random.RandomState(11).shuffle(xy)
    dxy = torch_mod.from_numpy(xy).cuda()
    stats = sc.new_stats()
    planes = sc.trace_packets(cam, RESX, RESY, dxy, stats=stats)
    fr = sc.alloc_frame(RESX, RESY)
    sc.packets_to_frame(dxy, planes, fr)
    assert_frame(torch_mod, fr, stats, oracle_frame(cam, mode), "packet list")
    # the heat-map instantiation (PSTATS) packet by packet, in both axis views: 48x32 = six packets each
    for case in ("plus_z", "minus_z"):
        c = view(case)[1]
        want, deferred = oracle_primary_packets(osc, c.as_array13(), 48, 32, frame_xy(48, 32), mode)
        assert not deferred.any()
        got, tot = dev_packet_stats(torch_mod, sc, c, 48, 32)
        assert np.array_equal(got, want), (case, got.tolist(), want.tolist())
        assert np.array_equal(tot, want.sum(axis=0))


@pytest.mark.parametrize("arith,mode", ARITHS)
def test_the_shadow_walk_ignores_the_bits_of_the_cameras_array(torch_mod, arith, mode):
    """a light AT the camera: the shadow packets walk the camera's origin-relative array, leaves with flagged count words included"""
    osc = pair()[2]
    sc = gpu_scene(arith)
    pos, cam = view("minus_z")
    ext = float((osc.nodes[0]["bmax"] - osc.nodes[0]["bmin"]).max())
    lights = np.array([[pos[0], pos[1], pos[2], 1.0, 0.9, 0.8, 2.0 * ext]], dtype=F)
    want, wst = osc.render_whitted(cam.as_array13(), RESX, RESY, lights, mode=mode, threads=8)
    stats = sc.new_stats()
    got = sc.render_whitted(cam, RESX, RESY, lights, stats=stats).cpu().numpy()
    torch_mod.cuda.synchronize()
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(stats.cpu().numpy().astype(np.uint64), wst), (stats.cpu().numpy(), wst)
    assert want.max() > 40
    check_bits(sc, osc.nodes, pos, "light at the camera")


@pytest.mark.parametrize("arith,mode", ARITHS)
def test_a_rebuilt_tree_is_flagged_and_traced_anew(torch_mod, arith, mode):
    from snail_amd.scene import Scene
    tv = pair()[0]
    tv2 = (tv * F(1.25)).astype(F)[::-1].copy()
    sc = Scene.from_fast_dev(torch_mod.from_numpy(np.ascontiguousarray(tv)).cuda())
    sc.set_arith(arith)
    pos, cam = view("plus_z")
    counts, slots = [], None
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
            # the slots past the first tree are empty (no bits); a shorter second tree leaves the first one's records in the slots past it,
            # which nobody refers to but which the count runs over
            slots = osc.nodes if slots is None or len(slots) <= len(osc.nodes) else np.concatenate([osc.nodes, slots[len(osc.nodes):]])
            counts.append(axis_flag_count(sc, pos))
            written = ((slots["sub"] & np.uint32(0x80000000)) == 0) | (slots["aux"] > 0)      # (a slot no node was committed to is an empty leaf)
            assert counts[-1] == [int(x) for x in axis_bits(slots[written], pos).sum(axis=0)], k
        assert counts[0] != counts[1]          # a stale array could not pass
    finally:
        sc.close()


@pytest.mark.parametrize("arith,mode", ARITHS)
def test_leaves_of_more_than_16_triangles_keep_their_count(torch_mod, arith, mode):
    """the product tree with subtrees of up to 40 triangles collapsed into one leaf: counts above 16 (bit 4 and up of the word that carries the bits)"""
    from snail_amd.scene import Scene
    hb = U.collapsed_tree(pair()[1], 40)
    isleaf = (hb.nodes["sub"] & np.uint32(0x80000000)) != 0
    assert int(hb.nodes["aux"][isleaf].max()) > 16
    osc = O.OracleScene.from_arrays(hb.tris, hb.nodes, hb.depth, hb.perm)
    sc = Scene(hb, 0)
    sc.set_arith(arith)
    try:
        for case in ("plus_z", "minus_z"):
            pos, cam = view(case)
            stats = sc.new_stats()
            f = sc.trace_primary(cam, RESX, RESY, stats=stats)
            ref = osc.render_primary(cam.as_array13(), RESX, RESY, mode=mode, threads=8)
            assert_frame(torch_mod, f, stats, ref, "collapsed tree, " + case)
            check_bits(sc, osc.nodes, pos, "collapsed tree, " + case)
    finally:
        sc.close()
