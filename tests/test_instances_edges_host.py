"""The edge cases of tests/instances_edges.py on the host: the restatement's three primary forms (frame, rects, packet list) against each
other and against the plain oracle, and -- case group by case group -- the proof that a case reaches the edge it is named for (a
clipped packet with hits on both sides of the clip, a top-level stack of 60 and more entries, both child orders on every axis, exact-t
ties, Inv(0) inside an instance and inf * 0 at the top-level box test, a rounded org - T).  tests/test_gpu_instances_edges.py runs the
device over the same cases."""
import ctypes as C

import numpy as np
import pytest

from snail_amd import _lib, survey_camera
from snail_amd.instances import build_instances
from tests import dbvh_ref as R
from tests import instances_edges as E
from tests import oracle_lib as O
from tests import util as U


def _same(a, b):
    for x, y, what in zip(a[:3], b[:3], "tuv"):
        U.assert_bit_equal(x, y, what)
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])


# ---- the three primary forms -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,mode", [((17, 33), O.MODE_IEEE), ((100, 7), O.MODE_SSE)])
def test_frame_rects_and_packet_list_agree(size, mode):
    resx, resy = size
    case, cam = E.blob(), E.blob_camera()
    full = E.expected_frame(case, cam, resx, resy, mode)
    # rects that tile the frame: a left block of whole packets, the rest in two pieces (one past the frame's edge on purpose)
    xs = 16 * ((resx - 1) // 16)
    ys = 16 * ((resy - 1) // 32) if resy > 16 else 0
    rects = [(0, 0, xs, resy)] if xs else []
    rects += [(xs, 0, resx - xs, ys)] if ys else []
    rects += [(xs, ys, 16, resy - ys)]
    miss = (np.float32(np.inf), np.float32(0), np.float32(0), 0, 0)
    acc = [np.full((resy, resx), m, dtype=p.dtype) for p, m in zip(full[:5], miss)]
    covered = np.zeros((resy, resx), dtype=np.int32)
    stats = np.zeros(4, dtype=np.uint64)
    for r in rects:
        got = case.ref().render_primary(cam.as_array13(), resx, resy, mode=mode, rect=r)
        x0, y0, w, h = r
        inside = np.zeros((resy, resx), dtype=bool)
        inside[y0:min(resy, y0 + h), x0:min(resx, x0 + w)] = True
        for k in range(5):      # outside its clipped rect a rect frame keeps the miss
            assert np.array_equal(got[k][~inside].view(np.uint32), np.full((~inside).sum(), miss[k], dtype=got[k].dtype).view(np.uint32))
            acc[k][inside] = got[k][inside]
        covered += inside
        stats += got[5]
    assert (covered == 1).all()
    _same(acc, full)
    assert np.array_equal(stats, full[5])
    xy = E.grid_packets(resx, resy)
    pk = E.expected_packets(case, cam, resx, resy, xy, mode)
    _same(E.scatter_packets(pk[:5], xy, resx, resy), full)
    assert np.array_equal(pk[5], full[5])


@pytest.mark.parametrize("mode", [O.MODE_IEEE, O.MODE_SSE])
def test_identity_instance_equals_the_plain_oracle_at_a_partial_size(mode):
    """tests/test_gpu_instances.py::test_identity_instance_equals_the_bvh_path, CPU against CPU, at 37 x 21"""
    osc = E.oracle("box")
    cam = survey_camera(E.blas_tris("box"))
    case = E.Case("identity", ["box"], np.eye(3, dtype=np.float32)[None], np.zeros((1, 3), np.float32))
    t, u, v, inst, tri, st = case.ref().render_primary(cam.as_array13(), 37, 21, mode=mode)
    ot, ou, ov, otid, ost = osc.render_primary(cam.as_array13(), 37, 21, mode=mode, threads=2)
    for a, b, what in ((t, ot, "t"), (u, ou, "u"), (v, ov, "v")):
        U.assert_bit_equal(a, b, what)
    assert np.array_equal(tri, otid) and not inst.any()
    assert np.isfinite(t).sum() > 50 and st[2] == ost[2] == 6 * 256


# ---- non-vacuity ---------------------------------------------------------------------------------------------------------------------------
def _clip_counts(case, cam, resx, resy, mode=O.MODE_IEEE):
    """hit pixels in the kept part of clipped packets, hit rays in their clipped-away part"""
    fr = E.expected_frame(case, cam, resx, resy, mode)
    xy = E.grid_packets(resx, resy)
    pk = E.expected_packets(case, cam, resx, resy, xy, mode)
    hit = np.isfinite(fr[0])
    kept = away = 0
    for i, (px, py) in enumerate(xy.tolist()):
        if px + 16 > resx or py + 16 > resy:
            inside = np.zeros((16, 16), dtype=bool)
            inside[:min(16, resy - py), :min(16, resx - px)] = True
            kept += int(hit[py:py + 16, px:px + 16].sum())
            away += int((np.isfinite(pk[0][i]).reshape(16, 16) & ~inside).sum())
    return kept, away


@pytest.mark.parametrize("size", [s for s in E.PARTIAL_SIZES if s[0] % 16 or s[1] % 16])
def test_partial_frames_hit_on_both_sides_of_the_clip(size):
    kept, away = _clip_counts(E.blob(), E.blob_camera(), *size)
    assert kept >= 1 and away >= 1, (size, kept, away)


def test_rects_and_packet_list_hit_on_both_sides_of_the_clip():
    resx, resy = E.RECT_FRAME
    kept, away = _clip_counts(E.blob(), E.blob_camera(), resx, resy)
    assert kept >= 1 and away >= 1
    for r in E.RECTS:
        t = E.expected_frame(E.blob(), E.blob_camera(), resx, resy, O.MODE_IEEE, rect=r)[0]
        assert np.isfinite(t).sum() >= 1, r
    xy = E.packet_list(resx, resy)
    n_grid = len(E.grid_packets(resx, resy))
    assert len(xy) > n_grid + 1 and len(np.unique(xy, axis=0)) == n_grid


@pytest.mark.parametrize("far_first", [False, True])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_comb_64_fills_the_top_level_stack(axis, far_first):
    case = E.comb(64, axis, far_first)
    cams = E.comb_cameras(case, axis)
    reached = {}
    for which in ("low", "high"):
        R.Ref.max_stack = 0
        fr = E.expected_frame(case, cams[which], 32, 32, O.MODE_IEEE)
        reached[which] = R.Ref.max_stack
        assert np.isfinite(fr[0]).sum() > 20
    deep = E.deep_camera(far_first)
    assert reached[deep] >= 60, reached
    assert reached["high" if deep == "low" else "low"] < 60, reached      # (the other end takes the leaf first: nothing piles up)
    # every box is the exact union of its children's
    nd = case.nodes
    for i in np.nonzero((nd["sub"] & 0x80000000) == 0)[0]:
        a, b = nd[int(nd["sub"][i])], nd[int(nd["sub"][i]) + 1]
        assert np.array_equal(nd["bmin"][i], np.minimum(a["bmin"], b["bmin"])) and np.array_equal(nd["bmax"][i], np.maximum(a["bmax"], b["bmax"]))


def test_comb_64_over_the_deep_blas_fills_the_stack_too():
    case, cams = E.chain_comb()
    assert E.oracle("chain").depth > 62
    R.Ref.max_stack = 0
    low = E.expected_frame(case, cams["low"], 32, 16, O.MODE_IEEE)
    assert R.Ref.max_stack >= 60 and np.isfinite(low[0]).sum() >= 5
    assert np.isfinite(E.expected_frame(case, cams["side"], 32, 16, O.MODE_IEEE)[0]).sum() >= 5


def _create_error(nodes, xf, bi):
    """snail_instances_create without a BLAS scene: the tree is validated first, which needs no device (tests/test_instances_host.py)"""
    L = _lib.lib()
    h = L.snail_instances_create((C.c_void_p * 1)(None), 1, _lib.ptr(nodes), len(nodes), _lib.ptr(xf), _lib.ptr(bi), len(xf), 0)
    assert not h
    return L.snail_last_error().decode()


def test_comb_depth_limit():
    """64 levels pass the tree validation (and stop at the missing BLAS handle), 65 are refused for their depth"""
    for depth, want in ((63, "invalid scene handle"), (64, "invalid scene handle"), (65, "deeper than 64")):
        c = E.comb(depth, 0, True)
        msg = _create_error(c.nodes, c.xs, c.bs)
        assert want in msg and (depth < 65 or "depth" in msg), (depth, msg)


def test_octant_cameras_take_both_child_orders_on_every_axis():
    case = E.octant_field()
    cams = E.octant_cameras(case)
    octants = set()
    R.Ref.orders_seen = set()
    for cam in cams:
        fr = E.expected_frame(case, cam, 32, 32, O.MODE_IEEE)
        assert np.isfinite(fr[0]).sum() > 20
        octants.add(tuple(bool(x < 0) for x in np.asarray(cam.front)))
    assert len(octants) == 8
    seen = R.Ref.orders_seen
    for axis in range(3):
        assert {fn ^ s for a, fn, s in seen if a == axis} == {0, 1}, (axis, seen)
        assert {s for a, fn, s in seen if a == axis} == {0, 1}, (axis, seen)


def test_exact_rotations_are_exact():
    rot = E.exact_rotations()
    assert rot.shape == (28, 3, 3) and len({m.tobytes() for m in rot}) == 28
    for m in rot:
        assert np.array_equal(m.astype(np.float64) @ m.astype(np.float64).T, np.eye(3)) and set(np.abs(m).reshape(-1).tolist()) == {0.0, 1.0}
    det = np.round(np.linalg.det(rot.astype(np.float64)))
    assert (det[:24] == 1).all() and (det[24:] == -1).all()
    case, cam = E.rotation_field(), E.rotation_camera()
    org = np.asarray(cam.pos, dtype=np.float32)
    for T in case.tr:       # org - T is exact
        assert np.array_equal((org - T).astype(np.float64), org.astype(np.float64) - T.astype(np.float64))
    # a ray of column resx / 2 has an outer direction component of exactly 0; in an instance that permutes the axes it arrives on another
    # inner axis, where SafeInv gives 1 / 1e-8
    dd, _ = O.gen_packet(np.asarray(cam.as_array13()), 96, 64, 48, 16, O.MODE_IEEE)
    d = dd.reshape(64, 3, 4)
    assert (d[:, 0, 0][::4] == 0).all() and (d[:, 2, :] > 0).all()
    big = R.inv(np.float32(0.0) + E.EPS, O.MODE_IEEE)
    axes_with_zero = set()
    for slot in range(len(case.xs)):
        Rm = case.xs[slot][:9].reshape(3, 3)
        nd = np.stack([(d[:, 0, :] * Rm[0, c] + d[:, 1, :] * Rm[1, c]) + d[:, 2, :] * Rm[2, c] for c in range(3)], axis=1)
        nid = R.inv(nd + E.EPS, O.MODE_IEEE)
        for c in range(3):
            if (nid[:, c, :] == big).any():
                axes_with_zero.add(c)
    assert axes_with_zero == {0, 1, 2}
    for resx, resy in ((96, 64), (33, 17)):
        fr = E.expected_frame(case, cam, resx, resy, O.MODE_IEEE)
        assert len(np.unique(fr[3][np.isfinite(fr[0])])) >= (20 if resx == 96 else 8)


@pytest.mark.parametrize("k", E.FAR_K)
def test_far_field_rounds_and_still_hits(k):
    for axes in E.FAR_AXES:
        case, cam, t64, org64 = E.far_field(k, axes)
        org = np.asarray(cam.pos, dtype=np.float32)
        fr = E.expected_frame(case, cam, 64, 48, O.MODE_IEEE)
        assert np.isfinite(fr[0]).sum() > 20, (k, axes, int(np.isfinite(fr[0]).sum()))
        if k == 24:
            diff32 = (org[None, :] - case.tr).astype(np.float64)
            assert (diff32 != org64[None, :] - t64).any(), axes
            ext = E.bbox6(["unit"])[0]
            assert (ext[3:] - ext[:3]).max() < np.spacing(np.float32(2.0 ** 24))


def test_duplicates_tie_exactly_and_take_median_splits():
    ties = 0
    for case, m in E.duplicates():
        cam = E.duplicates_camera(case)
        r0, t0 = E._dup_transform()
        dup_slots = [s for s in range(len(case.xs)) if case.xs[s].tobytes() == np.concatenate([r0.reshape(-1), t0]).astype(np.float32).tobytes()]
        assert len(dup_slots) == m
        alone = []
        for s in dup_slots[:3]:         # each duplicate alone, through a one-instance Ref (the inputs are bit-equal, so the later ones add nothing)
            one = E.Case("%s-alone-%d" % (case.key, s), ["box"], case.xs[s][:9].reshape(1, 3, 3), case.xs[s][9:].reshape(1, 3))
            alone.append(E.expected_frame(one, cam, 64, 48, O.MODE_IEEE)[0])
        hit = np.isfinite(alone[0])
        for other in alone[1:]:
            assert np.array_equal(alone[0].view(np.uint32), other.view(np.uint32))
        ties += int(hit.sum())
        # ... and in the whole case a duplicate is what the camera sees (which of them a pixel reports is the walk order's business: the
        # packet's child order decides whose equal t comes first)
        fr = E.expected_frame(case, cam, 64, 48, O.MODE_IEEE)
        won = np.isin(fr[3], dup_slots) & np.isfinite(fr[0])
        assert won.sum() > 20
        U.assert_bit_equal(fr[0][won], alone[0][won], "the tie's t")
    assert ties >= 100, ties
    nine = [c for c, m in E.duplicates() if c.key == "dup-9"][0]
    assert np.array_equal(nine.perm, np.arange(9))
    rn, rd, rp = R.build(nine.xf, nine.bi, E.bbox6(nine.names))
    assert rn.tobytes() == nine.nodes.tobytes() and np.array_equal(rp, np.arange(9))
    for c, _ in E.duplicates():     # the library's builder and the restatement's agree on every duplicate case
        rn, rd, rp = R.build(c.xf, c.bi, E.bbox6(c.names))
        assert rn.tobytes() == c.nodes.tobytes() and np.array_equal(rp, c.perm)


def _inner_idir(case, slot, d, mode):
    Rm = case.xs[slot][:9].reshape(3, 3)
    nd = np.stack([(d[:, 0, :] * Rm[0, c] + d[:, 1, :] * Rm[1, c]) + d[:, 2, :] * Rm[2, c] for c in range(3)], axis=1)
    with np.errstate(all="ignore"):
        return R.inv((nd + E.EPS).astype(np.float32), mode)


@pytest.mark.parametrize("shared,masked", [(True, False), (True, True), (False, False), (False, True)])
@pytest.mark.parametrize("size", [64, 16])
def test_singular_packets_reach_inv_of_zero(size, shared, masked):
    case = E.singular_field()
    mode = O.MODE_IEEE
    org, d, idir, mask, dist, obj, bary, edited = E.singular_packets(case, size, shared, masked, mode)
    root = case.nodes[0]
    n_packets = len(d) // size
    nan_products = 0
    for p in range(n_packets):
        iq = idir[p * size:(p + 1) * size].reshape(size, 3, 4)
        c = p % 3
        for q in edited[p]:
            assert mask is None or int(mask[p * size + q]) == 15                     # every lane of a singular quad is active
            assert np.isinf(iq[q, c]).all()                                          # the outer idir is inf ...
            o = org[p].reshape(3, 4)[c] if shared else org[p * size + q].reshape(3, 4)[c]
            with np.errstate(all="ignore"):
                nan_products += int(np.isnan(iq[q, c] * (root["bmin"][c] - o)).sum())   # ... and meets 0 at the root box: inf * 0
    assert nan_products >= 4 * n_packets
    # the singular lanes are walked: some hit an instance, in which (as in every instance: all are axis permutations) the component arrives
    # on an inner axis whose SafeInv is Inv(0)
    elem = np.zeros_like(obj)
    st = E.ref_generic(case.ref(), org, d, idir, mask, dist, obj, elem, bary, size, shared, mode)
    assert st[0] > 0 and np.isfinite(dist).sum() > 10
    inner_hits = 0
    for p in range(n_packets):
        for q in edited[p]:
            for l in np.nonzero(np.isfinite(dist[p * size + q]))[0]:
                nid = _inner_idir(case, int(obj[p * size + q, l]), d[p * size + q].reshape(1, 3, 4), mode)
                inner_hits += int(np.isinf(nid[0, :, l]).any())
    assert inner_hits >= 1
    inner_axes = set()
    for slot in range(len(case.xs)):
        nid = _inner_idir(case, slot, d[:size].reshape(size, 3, 4)[edited[0]], mode)
        inner_axes |= {ax for ax in range(3) if np.isinf(nid[:, ax]).any()}
    assert inner_axes == {0, 1, 2}
    # in the SSE arithmetic rcpps(0) = inf goes through the Newton step: inf + inf - (0 * inf) * inf = NaN
    idir_sse = E.singular_packets(case, size, shared, masked, O.MODE_SSE)[2]
    assert np.isnan(idir_sse[edited[0][0], 0:4]).all()


@pytest.mark.parametrize("size", [64, 16])
def test_singular_shadow_packets_reach_inv_of_zero(size):
    case = E.singular_field()
    org, d, idir, dist, edited = E.singular_shadow_packets(case, size, O.MODE_IEEE)
    root = case.nodes[0]
    nan_products = 0
    for p in range(len(d) // size):
        c = p % 3
        for q in edited[p]:
            iq = idir[p * size + q].reshape(3, 4)
            assert np.isinf(iq[c]).all() and (dist[p * size + q] > 0).all()
            with np.errstate(all="ignore"):
                nan_products += int(np.isnan(iq[c] * (root["bmin"][c] - org[p, c])).sum())
    assert nan_products >= 12
    before = dist.copy()
    st = E.ref_shadow(case.ref(), org, d, idir, dist, size, O.MODE_IEEE)
    assert st[0] > 0 and (dist[before > 0] == -np.inf).sum() > 10
    assert sum(int((dist[p * size + q] == -np.inf).sum()) for p in range(len(d) // size) for q in edited[p]) >= 1      # a singular lane is occluded
