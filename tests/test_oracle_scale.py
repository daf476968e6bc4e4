"""The oracle under exact scaling: triangles, camera position, ray origins, light positions / radii and shadow distances times 2^k
(directions unchanged).  Every multiplication is exact while nothing under- or overflows, and the oracle's arithmetic is then
scale-equivariant: the same tree, the same hits, t times 2^k.  These tests pin where that holds and where it breaks (denormal
intermediates below, overflow above, the absolute constants of the Whitted frame), and where snail_scene_create's fastOK flag flips,
so that tests/test_gpu_extremes.py, which sweeps the kernels across those boundaries, stands on checked ground."""
import numpy as np
import pytest

from tests import extremes as X
from tests import oracle_lib as O
from tests import util

KS = [-40, -32, -30, -25, -21, -20, -19, -10, 0, 10, 15, 18, 19, 20, 25, 29, 30, 31, 40]
EXACT_KS = [-20, -10, 10, 25, 29]           # inside the exact-scaling range for both scenes
RES = (160, 96)


def _primary(name, k, mode):
    tv, hb, osc = X.scaled_pair(name, k)
    return osc.render_primary(X.scaled_camera(name, k).as_array13(), RES[0], RES[1], mode=mode, threads=4)


def _scaled_equal(base, got, k):
    """t == 2^k * t0 bit for bit, u, v, triId and the TreeStats identical"""
    t0, u0, v0, tid0, st0 = base
    t, u, v, tid, st = got
    return (np.array_equal(tid, tid0) and np.array_equal(st, st0) and util.bits(u).tobytes() == util.bits(u0).tobytes()
            and util.bits(v).tobytes() == util.bits(v0).tobytes() and util.bits((t0 * X.pow2(k)).astype(np.float32)).tobytes() == util.bits(t).tobytes())


@pytest.mark.parametrize("name", ["atrium:0.02", "box"])
def test_builders_agree_and_tree_scales(name):
    """HostBVH.build (the product's host builder) and the oracle's builder give the same bytes at every scale, and the tree at 2^k is the
    k = 0 tree with its bounds times 2^k: same child / leaf structure, same triangle order."""
    tv0, hb0, osc0 = X.scaled_pair(name, 0)
    for k in KS:
        tv, hb, osc = X.scaled_pair(name, k)
        assert hb.nodes.tobytes() == osc.nodes.tobytes(), k
        assert hb.tris.tobytes() == osc.tris.tobytes(), k
        assert np.array_equal(hb.perm, osc.perm) and np.array_equal(osc.perm, osc0.perm), k
        assert hb.depth == osc.depth == osc0.depth, k
        assert X.scaled_tree_equals(osc0.nodes, osc.nodes, k), k


@pytest.mark.parametrize("name,ok_ks,bad_ks", [
    ("atrium:0.02", [-10, 0, 10, 15, 18, 19, 20, 25], [-40, -30, -25, -21, -20, -19, 29, 30]),
    ("box", [-20, -19, -10, 0, 10, 15, 18, 19, 20, 25], [-40, -30, -25, -21, 29, 30]),
    ("stress:0.05", [-10, 0, 10, 15, 18, 19, 20], [-40, -30, -25, -21, -20, -19, 25, 29, 30]),
])
def test_fast_ok_flips_across_the_sweep(name, ok_ks, bad_ks):
    """The numpy restatement of snail_scene_create's fastOK rule over the records: the sweep crosses the boundary on both sides."""
    for k in ok_ks:
        assert X.fast_ok(X.scaled_pair(name, k)[2].tris, X.scaled_pair(name, k)[2].nodes), (name, k)
    for k in bad_ks:
        assert not X.fast_ok(X.scaled_pair(name, k)[2].tris, X.scaled_pair(name, k)[2].nodes), (name, k)


def test_fast_ok_rule_restatement_on_hand_made_records():
    """Each clause of the rule on its own: one record pushed just past its bound flips the flag."""
    tv, hb, osc = X.scaled_pair("box", 0)
    assert X.fast_ok(osc.tris, osc.nodes)
    for field, idx, val in [("a", (3, 1), 1.5e9), ("ba", (0, 2), -1.5e9), ("ca", (5, 0), 2e9), ("t0", 4, 0.0), ("it0", 2, 2e12),
                            ("it0", 2, np.inf), ("plane", (1, 3), 2e18), ("plane", (1, 0), np.nan)]:
        t = osc.tris.copy()
        t[field][idx] = val
        assert not X.fast_ok(t, osc.nodes), (field, val)
    for field, idx, val in [("bmin", (2, 0), -2e9), ("bmax", (0, 1), np.inf), ("bmin", (1, 2), 1e8)]:
        n = osc.nodes.copy()
        n[field][idx] = val
        assert not X.fast_ok(osc.tris, n), (field, val)
    assert X.origin_sane([1e9, -1e9, 0]) and not X.origin_sane([0, 1.0000001e9, 0]) and not X.origin_sane([np.nan, 0, 0])


@pytest.mark.parametrize("mode", [O.MODE_IEEE, O.MODE_SSE])
@pytest.mark.parametrize("name", ["atrium:0.02", "box"])
def test_primary_frames_scale_exactly_inside_the_range(name, mode):
    base = _primary(name, 0, mode)
    assert np.isfinite(base[0]).sum() > 1000
    for k in EXACT_KS + [-19, -21, 18, 19, 20, 30]:
        assert _scaled_equal(base, _primary(name, k, mode), k), (name, k)


@pytest.mark.parametrize("mode", [O.MODE_IEEE, O.MODE_SSE])
def test_primary_frames_stop_scaling_where_stated(mode):
    """Below: denormal intermediates change t / u / v of atrium at k = -30 (not which triangle is hit, nor the walk); at k = -40 the
    triangle records degenerate (no hit).  Above: products overflow at k = 31 (hits are lost) and nothing is hit at k = 40."""
    name = "atrium:0.02"
    base = _primary(name, 0, mode)
    n0 = int(np.isfinite(base[0]).sum())
    m30 = _primary(name, -30, mode)
    assert not _scaled_equal(base, m30, -30)
    assert np.array_equal(m30[3], base[3]) and np.array_equal(m30[4], base[4])
    assert int(np.isfinite(_primary(name, -40, mode)[0]).sum()) == 0
    p31 = int(np.isfinite(_primary(name, 31, mode)[0]).sum())
    assert 0 < p31 < n0 * 0.8, (p31, n0)
    assert int(np.isfinite(_primary(name, 40, mode)[0]).sum()) == 0
    if mode == O.MODE_IEEE:
        assert (n0, p31) == (15359, 9246)
    for nm in ("box",):
        b = _primary(nm, 0, mode)
        assert 0 < int(np.isfinite(_primary(nm, 31, mode)[0]).sum()) < int(np.isfinite(b[0]).sum())


@pytest.mark.parametrize("mode", [O.MODE_IEEE, O.MODE_SSE])
@pytest.mark.parametrize("shared,masked,size", [(True, True, 64), (False, True, 64), (True, False, 23), (False, False, 23)])
def test_generic_packets_scale_exactly(mode, shared, masked, size):
    name = "atrium:0.02"
    npk = 4
    base = X.run_rays(X.scaled_pair(name, 0)[2], X.generic_packets(name, 0, shared, masked, size, npk), npk, size, shared, mode)
    assert (base[1] != 0).any()
    for k in EXACT_KS:
        d, o, b, st = X.run_rays(X.scaled_pair(name, k)[2], X.generic_packets(name, k, shared, masked, size, npk), npk, size, shared, mode)
        util.assert_bit_equal(d, (base[0] * X.pow2(k)).astype(np.float32), "distance k=%d" % k)
        util.assert_bit_equal(o, base[1], "object k=%d" % k)
        util.assert_bit_equal(b, base[2], "barycentric k=%d" % k)
        assert np.array_equal(st, base[3]), k


@pytest.mark.parametrize("mode", [O.MODE_IEEE, O.MODE_SSE])
def test_shadow_packets_scale_exactly(mode):
    name = "atrium:0.02"
    npk = 4
    base = X.run_shadow(X.scaled_pair(name, 0)[2], X.shadow_packets_scaled(name, 0, npk), npk, 64, mode)
    assert np.isneginf(base[0]).sum() > np.isneginf(X.shadow_packets_scaled(name, 0, npk)[3]).sum()     # something was occluded
    for k in EXACT_KS:
        d, st = X.run_shadow(X.scaled_pair(name, k)[2], X.shadow_packets_scaled(name, k, npk), npk, 64, mode)
        util.assert_bit_equal(d, (base[0] * X.pow2(k)).astype(np.float32), "shadow distance k=%d" % k)
        assert np.array_equal(st, base[1]), k


def _whitted(name, k, refl, mode=O.MODE_IEEE):
    tv, hb, osc = X.scaled_pair(name, k)
    return osc.render_whitted(X.scaled_camera(name, k).as_array13(), RES[0], RES[1], X.scaled_lights(name, k), mode=mode, reflections=refl, threads=4)


@pytest.mark.parametrize("mode", [O.MODE_IEEE, O.MODE_SSE])
def test_whitted_lights_only_scales_down_to_k_minus_3(mode):
    """Lights only: the frame and TreeStats are scale-invariant for k >= -3 when the light's position and radius scale too.  Lower, the
    absolute `dot(lv, lv) < 0.0001f` of Scene::TraceLight (src/scene_trace.cpp:546) changes pixels; with reflections the absolute 0.001f
    origin offset of the mirrored rays (src/scene_trace.cpp:611) breaks the scaling at every k != 0 (the walk's counters change; the
    rgb8 frame hides it for small |k|)."""
    name = "atrium:0.02"
    f0, s0 = _whitted(name, 0, False, mode)
    assert f0.max() > 0
    for k in (-3, -1, 5, 20, 25):
        f, s = _whitted(name, k, False, mode)
        assert np.array_equal(f, f0) and np.array_equal(s, s0), k
    broke = [k for k in (-8, -10, -20) if not np.array_equal(_whitted(name, k, False, mode)[0], f0)]
    assert broke, "lights-only frames scaled exactly below k = -3"
    r0, rs0 = _whitted(name, 0, True, mode)
    for k in (-2, -1, 1, 5, 20):
        assert not np.array_equal(_whitted(name, k, True, mode)[1], rs0), k
    assert not np.array_equal(_whitted(name, 10, True, mode)[0], r0)
