"""The kernels against the oracle outside the near-origin regime of the other GPU tests: scenes scaled by 2^k across both edges of the
fastOK rule and into the denormal and overflow regimes (with the GPU's own k = 0 result as a second reference where scaling is exact),
scenes and cameras far from the origin (the origin-relative subtractions round), and constructed rays through the generic entry points
(huge finite origins, unnormalised directions, caller idir near FLT_MAX, det == 0 and denormal det, origins on slab planes and edges).
tests/test_oracle_scale.py pins what the oracle does in these regimes."""
import math

import numpy as np
import pytest

from snail_amd import FPSCamera
from tests import extremes as X
from tests import oracle_lib as O
from tests import util
from tests.test_oracle_semantics import brute_force

pytestmark = pytest.mark.gpu

ARITHS = [("ieee", O.MODE_IEEE), ("host_sse", O.MODE_SSE)]
SWEEP_KS = [-30, -20, -10, 0, 10, 20, 25, 29, 31, 40]
EXACT_KS = {-20, -10, 10, 20, 25, 29}          # the oracle scales exactly there (tests/test_oracle_scale.py)
RES = (160, 96)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _scene(hb, arith):
    from snail_amd.scene import Scene
    sc = Scene(hb, 0)
    sc.set_arith(arith)
    return sc


def _primary(torch_mod, sc, osc, cam, mode, what):
    stats = sc.new_stats()
    f = sc.trace_primary(cam, RES[0], RES[1], stats=stats)
    torch_mod.cuda.synchronize()
    ref = osc.render_primary(cam.as_array13(), RES[0], RES[1], mode=mode, threads=4)
    got = tuple(x.cpu().numpy() for x in (f.t, f.u, f.v, f.tri_id)) + (stats.cpu().numpy().astype(np.uint64),)
    for g, r, n in zip(got[:4], ref[:4], ("t", "u", "v", "triId")):
        util.assert_bit_equal(g, r, "%s primary %s" % (what, n))
    assert np.array_equal(got[4], ref[4]), (what, got[4], ref[4])
    return got


def _rays(torch_mod, sc, osc, pk, npk, size, shared, mode, what):
    """device and host-pointer entry points against osc.trace_rays; returns the device's (distance, object, barycentric)"""
    from snail_amd.scene import Context
    origin, dirs, idir, mask, dist, obj, bary = pk
    d2, o2, b2, ost = X.run_rays(osc, pk, npk, size, shared, mode)
    tt = lambda a: torch_mod.from_numpy(np.ascontiguousarray(a)).cuda()
    ctx = Context(tt(origin), tt(dirs), tt(idir), tt(dist.copy()), tt(obj.copy()), tt(bary.copy()), size=size, shared_origin=shared,
                  mask=None if mask is None else tt(mask))
    stats = sc.new_stats()
    sc.traverse_primary(ctx, stats=stats)
    torch_mod.cuda.synchronize()
    got = (ctx.distance.cpu().numpy(), ctx.object.cpu().numpy(), ctx.barycentric.cpu().numpy())
    util.assert_bit_equal(got[1], o2, what + " object")
    util.assert_bit_equal(got[0], d2, what + " distance")
    util.assert_bit_equal(got[2], b2, what + " barycentric")
    st = stats.cpu().numpy().astype(np.uint64)
    assert st[0] == ost[0] and st[1] == ost[1], (what, st, ost)
    d3, o3, b3 = dist.copy(), obj.copy(), bary.copy()
    sc.trace_rays_host(origin, dirs, idir, mask, d3, o3, b3, npk, size, shared)
    util.assert_bit_equal(d3, d2, what + " host distance")
    util.assert_bit_equal(o3, o2, what + " host object")
    util.assert_bit_equal(b3, b2, what + " host barycentric")
    return got


def _shadow(torch_mod, sc, osc, pk, npk, size, mode, what):
    from snail_amd.scene import ShadowContext
    origin, dirs, idir, dist = pk
    d2, ost = X.run_shadow(osc, pk, npk, size, mode)
    tt = lambda a: torch_mod.from_numpy(np.ascontiguousarray(a)).cuda()
    ctx = ShadowContext(tt(origin), tt(dirs), tt(idir), tt(dist.copy()), size=size)
    stats = sc.new_stats()
    sc.traverse_shadow(ctx, stats=stats)
    torch_mod.cuda.synchronize()
    got = ctx.distance.cpu().numpy()
    util.assert_bit_equal(got, d2, what + " shadow distance")
    st = stats.cpu().numpy().astype(np.uint64)
    assert st[0] == ost[0] and st[1] == ost[1] and st[3] == ost[3], (what, st, ost)
    d3 = dist.copy()
    sc.trace_shadow_host(origin, dirs, idir, d3, npk, size)
    util.assert_bit_equal(d3, d2, what + " host shadow distance")
    return got


def _whitted(torch_mod, sc, osc, cam, lights, refl, mode, what):
    stats = sc.new_stats()
    g = sc.render_whitted(cam, RES[0], RES[1], lights, stats=stats, reflections=refl)
    torch_mod.cuda.synchronize()
    want, wst = osc.render_whitted(cam.as_array13(), RES[0], RES[1], lights, mode=mode, reflections=refl, threads=4)
    g = g.cpu().numpy()
    assert np.array_equal(g, want), (what, "whitted refl=%s" % refl, int((g != want).sum()))
    assert np.array_equal(stats.cpu().numpy().astype(np.uint64), wst), (what, stats.cpu().numpy(), wst)
    return g


# ---- (a) the scale sweep -------------------------------------------------------------------------------------------------------------------

PACKET_FORMS = [(True, True, 64), (False, True, 64), (True, False, 23), (False, False, 23)]     # shared, masked, size


@pytest.mark.parametrize("arith,mode", ARITHS)
@pytest.mark.parametrize("name", ["atrium:0.02", "box"])
def test_scale_sweep_bit_exact(torch_mod, name, arith, mode):
    flags, sane, base = set(), set(), {}
    npk = 3
    for k in [0] + [k for k in SWEEP_KS if k != 0]:
        tv, hb, osc = X.scaled_pair(name, k)
        cam = X.scaled_camera(name, k)
        sc = _scene(hb, arith)
        what = "%s k=%d %s" % (name, k, arith)
        fast = sc.flags()[0]
        assert bool(fast) == X.fast_ok(osc.tris, osc.nodes), what
        flags.add(bool(fast)); sane.add(X.origin_sane(cam.pos))
        res = {"primary": _primary(torch_mod, sc, osc, cam, mode, what)}
        for shared, masked, size in PACKET_FORMS:
            pk = X.generic_packets(name, k, shared, masked, size, npk)
            res[(shared, masked, size)] = _rays(torch_mod, sc, osc, pk, npk, size, shared, mode, "%s rays %s/%s/%d" % (what, shared, masked, size))
        res["shadow"] = _shadow(torch_mod, sc, osc, X.shadow_packets_scaled(name, k, npk), npk, 64, mode, what)
        lights = X.scaled_lights(name, k)
        res["whitted"] = _whitted(torch_mod, sc, osc, cam, lights, False, mode, what)
        _whitted(torch_mod, sc, osc, cam, lights, True, mode, what)
        sc.close()
        if k == 0:
            base = res
        elif k in EXACT_KS:      # the GPU's own k = 0 result, scaled: a reference that does not go through the oracle
            p, p0 = res["primary"], base["primary"]
            util.assert_bit_equal(p[0], (p0[0] * X.pow2(k)).astype(np.float32), what + " t vs 2^k t(k=0)")
            for i in (1, 2, 3):
                util.assert_bit_equal(p[i], p0[i], what + " u/v/triId vs k=0")
            assert np.array_equal(p[4], p0[4]), what
            for key in [f for f in PACKET_FORMS]:
                util.assert_bit_equal(res[key][0], (base[key][0] * X.pow2(k)).astype(np.float32), what + " rays distance vs k=0")
                util.assert_bit_equal(res[key][1], base[key][1], what + " rays object vs k=0")
                util.assert_bit_equal(res[key][2], base[key][2], what + " rays barycentric vs k=0")
            util.assert_bit_equal(res["shadow"], (base["shadow"] * X.pow2(k)).astype(np.float32), what + " shadow vs k=0")
            if k >= -3:          # (below, the absolute 0.0001f of Scene::TraceLight breaks the scaling: tests/test_oracle_scale.py)
                assert np.array_equal(res["whitted"], base["whitted"]), what + " lights-only frame vs k=0"
    assert flags == {True, False}, "the sweep must cross the fastOK boundary"
    assert False in sane, "the sweep must reach cameras that fail originSane"


# ---- (b) far from the origin ---------------------------------------------------------------------------------------------------------------

def _box_at_1e9(cx):
    """box * 2^20 with its +x face 1.5e6 short of x = 1e9 (fastOK), seen from x = cx looking -x: the camera just inside / just outside
    |o| <= 1e9 (float32 1e9 + 64 is the next value)"""
    return ("box", 20, (1e9 - 2.5e6, 0.0, 0.0)), FPSCamera(np.zeros(3, np.float32), math.pi / 2, 0.0).camera(), (cx, 0.0, 0.0), True

FAR_CASES = {
    "atrium-rounding": (("atrium:0.02", 0, (1e5 + 0.37, -3e6, 2.0 ** 24 + 5)), None, (1e5 + 0.37, -3e6, 2.0 ** 24 + 5), None),
    "atrium-2^20-offset": (("atrium:0.02", 20, (3.0e8 + 0.37, -1e8, 2.0 ** 28 + 5)), None, (3.0e8 + 0.37, -1e8, 2.0 ** 28 + 5), True),
    "box-1e9-inside": _box_at_1e9(1e9),
    "box-1e9-outside": _box_at_1e9(1e9 + 64),
}


def _first_principles(tv_bvh, osc, cam, t, tid, seed=0):
    """float64 check of >= 200 hit pixels: the reported triangle is hit at about t, and no front-facing triangle is hit clearly closer
    except next to an edge"""
    rng = np.random.RandomState(seed)
    o = cam.pos.astype(np.float64)
    bmin, bmax = osc.nodes[0]["bmin"].astype(np.float64), osc.nodes[0]["bmax"].astype(np.float64)
    extent = float((bmax - bmin).max())
    tol = 1e-4 * (float(np.abs(o).max()) + extent)
    ys, xs = np.nonzero(np.isfinite(t))
    assert len(ys) >= 200
    pick = rng.choice(len(ys), 200, replace=False)

    def edge_dist(tri, p):
        e = tri.astype(np.float64)
        return min(np.linalg.norm(np.cross(e[(k + 1) % 3] - e[k], p - e[k])) / max(np.linalg.norm(e[(k + 1) % 3] - e[k]), 1e-300) for k in range(3))

    for i in pick:
        y, x = int(ys[i]), int(xs[i])
        px, py = (x // 16) * 16, (y // 16) * 16
        dd, _ = O.gen_packet(cam.as_array13(), RES[0], RES[1], px, py)
        q, l = (y - py) * 4 + (x - px) // 4, (x - px) % 4
        d = np.array([dd[q * 12 + l], dd[q * 12 + 4 + l], dd[q * 12 + 8 + l]], dtype=np.float64)
        own, _ = brute_force(tv_bvh[[tid[y, x]]], o, d)
        p = o + d * float(t[y, x])
        assert (np.isfinite(own) and abs(own - float(t[y, x])) <= tol) or edge_dist(tv_bvh[tid[y, x]], p) <= 1e-3 * extent, (x, y, own, t[y, x])
        bt, bi = brute_force(tv_bvh, o, d)
        if bi >= 0 and bt < float(t[y, x]) - tol:
            front = float(osc.tris[bi]["plane"][:3].astype(np.float64) @ d) > 1e-6
            assert not front or edge_dist(tv_bvh[bi], o + d * bt) <= 1e-3 * extent, (x, y, bt, t[y, x])


@pytest.mark.parametrize("arith,mode", ARITHS)
@pytest.mark.parametrize("case", sorted(FAR_CASES))
def test_far_from_origin_bit_exact(torch_mod, case, arith, mode):
    (name, k, off), cam0, cam_off, want_fast = FAR_CASES[case]
    tv, hb, osc = X.moved_pair(name, k, off)
    cam0 = cam0 if cam0 is not None else X.base_camera(name)
    cam = X.moved_camera(cam0, k, cam_off)
    sc = _scene(hb, arith)
    what = "%s %s" % (case, arith)
    assert bool(sc.flags()[0]) == X.fast_ok(osc.tris, osc.nodes), what
    if want_fast is not None:
        assert X.fast_ok(osc.tris, osc.nodes) == want_fast, what
    if case.startswith("box-1e9"):
        assert X.origin_sane(cam.pos) == case.endswith("inside"), (what, cam.pos)
    p = _primary(torch_mod, sc, osc, cam, mode, what)
    assert np.isfinite(p[0]).sum() >= 200
    # the translation rounds atrium:0.02's vertices (the scaled scenes' move exactly).  The origin-relative differences o - a and
    # bmin - o of a camera inside or next to the scene stay exact even here (both operands within a factor of 2: Sterbenz); what rounds are
    # the vertices, the products and the cameras' and packets' own coordinates
    if case == "atrium-rounding":
        exact = (X.scaled_pair(name, k)[0].astype(np.float64) + np.asarray(off, dtype=np.float32).astype(np.float64))
        assert (tv.astype(np.float64) != exact).any(), what
    if mode == O.MODE_IEEE:
        _first_principles(tv[osc.perm], osc, cam, p[0], p[3])
    npk = 3
    for shared, masked, size in PACKET_FORMS[:2] + PACKET_FORMS[3:]:
        pk = util.secondary_packets(osc, cam, RES[0], RES[1], npk, seed=21, shared=shared, masked=masked, size=size)
        _rays(torch_mod, sc, osc, pk, npk, size, shared, mode, "%s rays %s/%s/%d" % (what, shared, masked, size))
    _shadow(torch_mod, sc, osc, util.shadow_packets(osc, npk, seed=4), npk, 64, mode, what)
    # three frames of a dolly path in one launch
    from snail_amd.scene import Scene  # noqa: F401  (the HitFrame allocator lives on the scene)
    cams = [X.moved_camera(cam0, k, cam_off, dolly) for dolly in (0.0, 0.75, 1.5)]
    outs = [sc.alloc_frame(RES[0], RES[1]) for _ in cams]
    stats = sc.new_stats()
    sc.trace_primary_batch(cams, RES[0], RES[1], outs, stats=stats)
    torch_mod.cuda.synchronize()
    tot = np.zeros(4, dtype=np.uint64)
    for c, f in zip(cams, outs):
        ref = osc.render_primary(c.as_array13(), RES[0], RES[1], mode=mode, threads=4)
        for g, r, n in zip((f.t, f.u, f.v, f.tri_id), ref[:4], ("t", "u", "v", "triId")):
            util.assert_bit_equal(g.cpu().numpy(), r, "%s batch %s" % (what, n))
        tot += ref[4]
    assert np.array_equal(stats.cpu().numpy().astype(np.uint64), tot), (what, stats.cpu().numpy(), tot)
    sc.close()


# ---- (c) constructed rays through the generic entry points ---------------------------------------------------------------------------------

def _edge_scene():
    """A few triangles with exact coordinates: a plane z = 0 triangle (normal +z), one with normal (1, -1, 0) / sqrt 2 (det == 0 for any
    direction with dx == dy bit for bit), and two that share an edge and a vertex."""
    tv = np.array([
        [[0, 0, 0], [4, 0, 0], [0, 4, 0]],
        [[0, 0, 2], [0, 0, 6], [3, 3, 2]],           # normal ∝ cross((0,0,4), (3,3,0)) = (-12, 12, 0)
        [[6, 0, 1], [8, 0, 1], [6, 2, 1]],           # shared edge (8,0,1)-(6,2,1) with the next one
        [[8, 0, 1], [8, 2, 1], [6, 2, 1]],
        [[20, 20, 20], [22, 20, 20], [20, 22, 21]],  # (a fifth one splits the root: inner slab planes)
        [[-9, 5, -3], [-7, 5, -3], [-9, 8, -2]],
    ], dtype=np.float32)
    from snail_amd import HostBVH
    return tv, HostBVH.build(tv), O.OracleScene(tv)


def _packet(origins, dirs, idir=None, shared=True):
    """one packet of 64 quads (256 rays) from per-ray origins / directions (lists cycled), idir = SafeInv unless given"""
    nq = 64
    org = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
    d = np.asarray(dirs, dtype=np.float32).reshape(-1, 3)
    idr = None if idir is None else np.asarray(idir, dtype=np.float32).reshape(-1, 3)
    D = np.zeros((nq, 12), np.float32); Oa = np.zeros((nq, 12), np.float32); I = np.zeros((nq, 12), np.float32)
    for r in range(nq * 4):
        q, l = r // 4, r % 4
        for c in range(3):
            D[q, c * 4 + l] = d[r % len(d), c]
            Oa[q, c * 4 + l] = org[0 if shared else r % len(org), c]
            I[q, c * 4 + l] = (np.float32(1.0) / (d[r % len(d), c] + np.float32(0.00000001))) if idr is None else idr[r % len(idr), c]
    origin = np.ascontiguousarray(Oa[:1]) if shared else Oa
    return [origin, D, I, None, np.full((nq, 4), np.inf, np.float32), np.zeros((nq, 4), np.int32), np.zeros((nq, 8), np.float32)]


def _aim(origin, targets):
    """unit directions from origin to targets, computed in float64"""
    o = np.asarray(origin, dtype=np.float64)
    t = np.asarray(targets, dtype=np.float64)
    d = t - o
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _targets(tv, n=64, seed=0):
    """random points on random triangles (float64)"""
    rng = np.random.RandomState(seed)
    t = np.asarray(tv, dtype=np.float64)[rng.randint(len(tv), size=n)]
    w = rng.dirichlet((1.0, 1.0, 1.0), size=n)
    return (t * w[:, :, None]).sum(1)


def _overflows(origin, osc):
    """float32 numpy replay of o - a and cross(ba, o - a): does any product overflow?"""
    with np.errstate(over="ignore", invalid="ignore"):
        tvec = (np.asarray(origin, np.float32)[None, :] - osc.tris["a"]).astype(np.float32)
        c = np.cross(osc.tris["ba"], tvec).astype(np.float32)
    return not np.isfinite(c).all() or not np.isfinite(tvec).all()


def _edge_cases():
    """(label, scene name or 'edge', packets, is-shared, expect-overflow) -- every input finite, so M_FAST / M_COH is eligible on a
    fastOK scene unless the kernel classifies by magnitude"""
    cases = []
    tg = _targets(X.scaled_pair("box", 0)[0])
    for M in (1e10, 1e20, 1e30, 3e38):
        o = np.array([0.25, -0.125, -M])
        for shared in (True, False):
            origins = [o] if shared else [o + np.array([0.0, 0.0, s * M * 1e-3]) for s in range(8)]
            dirs = _aim(o, tg)
            cases.append(("origin %.0e %s" % (M, "shared" if shared else "per-ray"), "box", _packet(origins, dirs, shared=shared), shared, M >= 3e38))
        cases.append(("origin -%.0e x" % M, "box", _packet([[-M, 0.3, 0.1]], _aim([-M, 0.3, 0.1], tg)), True, M >= 3e38))
    o = np.array([0.3, 0.2, -3.0])
    for s in (1e3, 1e10, 1e19, 1e30):
        cases.append(("|dir| %.0e" % s, "box", _packet([o], _aim(o, tg) * s), True, False))
    for big in (1e30, 1e35, 3.4e38):
        d = _aim(o, tg)
        d[::3, 0] = 0.0
        d[1::3, 1] = -0.0
        idir = 1.0 / (d + 1e-8)
        idir[::3, 0] = big
        idir[1::3, 1] = -big
        idir[2::6, 2] = np.sign(d[2::6, 2]) * big
        cases.append(("idir %.1e" % big, "box", _packet([o], d, idir), True, False))
    # det == 0: dx == dy bit for bit against the (1, -1, 0) triangle, aimed through its plane x == y
    o2 = np.array([-1.0, -1.0, 3.0], np.float32)
    dz = np.linspace(-0.3, 0.3, 16)
    d = np.stack([np.full(16, 0.7), np.full(16, 0.7), dz], 1).astype(np.float32)
    cases.append(("det == 0", "edge", _packet([o2], d), True, False))
    # denormal det against the z = 0 triangle: d = (1, 0, dz), origin z = -dz (hit at t = 1 at x = 0 .. 1 within the triangle), caller idir
    # exact where 1 / dz is finite, so that the slab test keeps the ray; |det| = dz < 2^-126 takes recipExact's full division
    dzs = np.array([1.5 * 2.0 ** -128, 2.0 ** -127, 1.25 * 2.0 ** -127, 1.75 * 2.0 ** -127, 2.0 ** -126, 3 * 2.0 ** -127], np.float32)
    orgs = [[-0.5, 0.25 + 0.25 * i, -float(dz)] for i, dz in enumerate(dzs)]
    dirs = [[1.0, 0.0, float(dz)] for dz in dzs]
    idirs = [[1.0, 1e8, float(np.float32(1.0) / dz)] for dz in dzs]
    cases.append(("denormal det", "edge", _packet(orgs, dirs, idirs, shared=False), False, False))
    # origins on slab planes of the root and of a child, and on a shared edge / vertex
    tv, hb, esc = _edge_scene()
    etg = _targets(tv, seed=3)
    assert len(esc.nodes) >= 3
    for i in (0, 1, 2):
        bmin, bmax = esc.nodes[i]["bmin"], esc.nodes[i]["bmax"]
        for p in ([bmin[0], 0.5, 0.5], [0.5, bmax[1], 0.5], [bmin[0], bmin[1], bmax[2]]):
            cases.append(("slab node %d %s" % (i, p), "edge", _packet([p], _aim(p, etg)), True, False))
    for p in ([7.0, 1.0, 1.0], [8.0, 0.0, 1.0], [6.0, 2.0, 1.0]):        # mid-edge, vertices
        dirs = _aim(p, etg)
        dirs[::4] = [0.0, 0.0, 1.0]
        dirs[1::4] = [0.0, 0.0, -1.0]
        cases.append(("on edge / vertex %s" % p, "edge", _packet([p], dirs), True, False))
        cases.append(("on edge / vertex per-ray %s" % p, "edge", _packet([p, p], dirs, shared=False), False, False))
    return cases


@pytest.mark.parametrize("arith,mode", ARITHS)
def test_constructed_rays_bit_exact(torch_mod, arith, mode):
    scenes_ = {"box": X.scaled_pair("box", 0)[1:], "edge": _edge_scene()[1:]}
    for hb, osc in scenes_.values():
        assert X.fast_ok(osc.tris, osc.nodes)
    scs = {n: _scene(hb, arith) for n, (hb, osc) in scenes_.items()}
    hits = {}
    for label, sname, pk, shared, overflow in _edge_cases():
        hb, osc = scenes_[sname]
        sc = scs[sname]
        assert sc.flags()[0] == 1
        assert all(np.isfinite(a).all() for a in pk[:3]), label                 # every input finite: M_FAST / M_COH eligible
        if overflow:
            assert _overflows(pk[0][0, [0, 4, 8]], osc), label
        elif label.startswith("origin"):
            assert not _overflows(pk[0][0, [0, 4, 8]], osc), label
        got = _rays(torch_mod, sc, osc, pk, 1, 64, shared, mode, "%s %s" % (label, arith))
        hits[label] = int((got[1] != 0).sum() + np.isfinite(got[0]).sum())
        if sname == "box" and label.startswith("origin") and shared:
            # the same rays as a shadow packet (origin = the light), distances up to the far side of the scene
            o = pk[0][0, [0, 4, 8]]
            dist = np.full((64, 4), min(2.0 * float(np.abs(o).max()), 3.0e38), np.float32)
            dist[3] = -np.inf
            _shadow(torch_mod, sc, osc, [o[None, :].copy(), pk[1], pk[2], dist], 1, 64, mode, "%s shadow %s" % (label, arith))
    for s in scs.values():
        s.close()
    assert any(v for v in hits.values())
