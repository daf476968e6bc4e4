"""GPU parity tests (run with -m gpu on an MI355X): the HIP path through the C-ABI vs the CPU oracle.

Bar (BASELINE.json north_star): triId bit-exact, t/u/v within 1e-4.  Because both sides implement the
two approximate operations of the path with veclib's scalar definitions (Inv = 1/x, RSqrt = 1/sqrt(x),
IEEE-rounded) and every other operation is a separately rounded fp32 mul/add/min/max, these tests hold
the HIP path to the stronger bar of BIT-EXACT t, u, v, triId and TreeStats counters against the oracle
in ORC_MODE_IEEE.  The oracle's ORC_MODE_SSE (what the reference executes on x86: rcpps/rsqrtps + one
Newton step) is compared with tolerance 1e-4 in test_sse_mode_tolerance."""
import os

import numpy as np
import pytest

from snail_amd import FPSCamera, scenes
from tests import oracle_lib as O
from tests import util

pytestmark = pytest.mark.gpu

TOL = 1e-4   # north_star tolerance on t/u/v (relative to max(1,|t|))


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def gpu_scene(name):
    from snail_amd.scene import Scene
    tv, hbvh, osc = util.scene_pair(name)
    return tv, Scene(hbvh, 0), osc


def compare_frames(frame, oracle_out, what):
    t, u, v, tid, _ = oracle_out
    gt, gu, gv, gid = (x.cpu().numpy() for x in (frame.t, frame.u, frame.v, frame.tri_id))
    util.assert_bit_equal(gid, tid, what + " triId")
    util.assert_bit_equal(gt, t, what + " t")
    util.assert_bit_equal(gu, u, what + " u")
    util.assert_bit_equal(gv, v, what + " v")


@pytest.mark.parametrize("name,resx,resy", [
    ("box", 256, 256),            # BASELINE config 0
    ("box", 250, 130),            # ragged: not a multiple of 16 (and resx % 4 != 0 -> scalar stores)
    ("atrium:0.05", 640, 368),
    ("atrium:0.05", 328, 200),
    ("chain", 256, 144),          # depth-63 tree (second stack register pair) and a > 64-triangle leaf (chunked leaf loop)
    ("stress:0.05", 320, 192),
    ("patches", 96, 96),          # squares covering 1 .. 64 quads of a packet: the narrow-range leaf forms at every width
    ("patches", 200, 120),
    ("offgrid", 640, 400),        # full-mantissa vertices far from the origin, four decades of triangle sizes, slivers, near-coplanar shingles (scenes.offgrid)
    ("offgrid-in", 328, 200),     # the same from inside
])
def test_primary_frame_bit_exact(torch_mod, name, resx, resy):
    tv, sc, osc = gpu_scene(name)
    cam = util.camera_for(name, tv)
    stats = sc.new_stats()
    frame = sc.trace_primary(cam, resx, resy, stats=stats)
    torch_mod.cuda.synchronize()
    ref = osc.render_primary(cam.as_array13(), resx, resy, mode=O.MODE_IEEE)
    compare_frames(frame, ref, "%s %dx%d" % (name, resx, resy))
    assert np.array_equal(stats.cpu().numpy().astype(np.uint64), ref[4]), (stats.cpu().numpy(), ref[4])
    assert np.isfinite(ref[0]).sum() > 0
    sc.close()


def test_full_size_frame_bit_exact_and_properties(torch_mod):
    """BASELINE config 1 size: atrium (sponza stand-in, ~263 K triangles) at 1920x1080."""
    name = "atrium"
    tv, sc, osc = gpu_scene(name)
    cam = util.camera_for(name, tv)
    stats = sc.new_stats()
    frame = sc.trace_primary(cam, 1920, 1080, stats=stats)
    torch_mod.cuda.synchronize()
    ref = osc.render_primary(cam.as_array13(), 1920, 1080, mode=O.MODE_IEEE, threads=16)
    compare_frames(frame, ref, "atrium 1920x1080")
    st = stats.cpu().numpy()
    assert np.array_equal(st.astype(np.uint64), ref[4])
    assert st[2] == 1920 * 1088                       # padded to whole packets (src/render.cpp:67-68)
    # size-independent properties
    t = frame.t.cpu().numpy(); tid = frame.tri_id.cpu().numpy()
    u = frame.u.cpu().numpy(); v = frame.v.cpu().numpy()
    hit = np.isfinite(t)
    assert hit.mean() > 0.9                            # interior camera: almost every pixel hits
    assert (tid[~hit] == 0).all() and (u[~hit] == 0).all() and (v[~hit] == 0).all()
    assert (t[hit] > 0).all() and (tid[hit] >= 0).all() and (tid[hit] < len(tv)).all()
    assert (u[hit] >= -1e-4).all() and (v[hit] >= -1e-4).all() and ((u + v)[hit] <= 1 + 1e-4).all()
    # idempotence: a second launch into the same buffers gives the same bytes
    frame2 = sc.trace_primary(cam, 1920, 1080, out=frame)
    torch_mod.cuda.synchronize()
    util.assert_bit_equal(frame2.t.cpu().numpy(), t, "idempotence")
    # hit points lie on their triangle's plane: |n.(o + t d) - n.a| small
    hb = util.scene_pair(name)[1]
    ys, xs = np.nonzero(hit)
    sel = np.random.RandomState(0).choice(len(ys), 4096, replace=False)
    d, _ = O.gen_packet(cam.as_array13(), 1920, 1080, 0, 0)   # just to exercise the API; directions rebuilt below
    for i in sel[:256]:
        y, x = ys[i], xs[i]
        px, py = (x // 16) * 16, (y // 16) * 16
        dd, _ = O.gen_packet(cam.as_array13(), 1920, 1080, int(px), int(py))
        q = (y - py) * 4 + (x - px) // 4
        l = (x - px) % 4
        dirv = np.array([dd[q * 12 + l], dd[q * 12 + 4 + l], dd[q * 12 + 8 + l]], dtype=np.float64)
        P = cam.pos.astype(np.float64) + dirv * float(t[y, x])
        pl = hb.tris[tid[y, x]]["plane"].astype(np.float64)
        assert abs(pl[:3] @ P - pl[3]) < 1e-3 * max(1.0, abs(pl[3]))
    sc.close()


def test_rect_and_packet_list_match_full_frame(torch_mod):
    name = "atrium:0.05"
    tv, sc, osc = gpu_scene(name)
    cam = util.camera_for(name, tv)
    resx, resy = 640, 368
    full = sc.trace_primary(cam, resx, resy)
    # rect: only the rect is written, the rest keeps its previous contents
    part = sc.alloc_frame(resx, resy)
    part.t.fill_(-7.0)
    rect = (160, 64, 320, 128)
    sc.trace_primary(cam, resx, resy, rect=rect, out=part)
    torch_mod.cuda.synchronize()
    x0, y0, w, h = rect
    assert torch_mod.equal(part.t[y0:y0 + h, x0:x0 + w], full.t[y0:y0 + h, x0:x0 + w])
    assert torch_mod.equal(part.tri_id[y0:y0 + h, x0:x0 + w], full.tri_id[y0:y0 + h, x0:x0 + w])
    outside = part.t.clone(); outside[y0:y0 + h, x0:x0 + w] = -7.0
    assert (outside == -7.0).all()
    # packet list in a shuffled order + scatter == full frame
    xs, ys = np.meshgrid(np.arange(0, resx, 16), np.arange(0, resy, 16))
    xy = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.int32)
    np.random.RandomState(3).shuffle(xy)
    dxy = torch_mod.from_numpy(xy).cuda()
    planes = sc.trace_packets(cam, resx, resy, dxy)
    fr = sc.alloc_frame(resx, resy)
    sc.packets_to_frame(dxy, planes, fr)
    torch_mod.cuda.synchronize()
    for a, b in ((fr.t, full.t), (fr.u, full.u), (fr.v, full.v), (fr.tri_id, full.tri_id)):
        assert torch_mod.equal(a, b)
    # packet-major layout is the reference's quad order: quad ty*4+k = pixels x+4k.. of row y+ty
    p0 = planes[0][0].cpu().numpy().reshape(16, 4, 4)
    x, y = xy[0]
    np.testing.assert_array_equal(p0.reshape(16, 16), full.t[y:y + 16, x:x + 16].cpu().numpy())
    sc.close()


def test_host_pointer_entry_point(torch_mod):
    name = "box"
    tv, sc, osc = gpu_scene(name)
    cam = util.camera_for(name, tv)
    t, u, v, tid, stats = sc.trace_primary_host(cam, 256, 256)
    ref = osc.render_primary(cam.as_array13(), 256, 256, mode=O.MODE_IEEE)
    util.assert_bit_equal(t, ref[0], "t"); util.assert_bit_equal(tid, ref[3], "id")
    util.assert_bit_equal(u, ref[1], "u"); util.assert_bit_equal(v, ref[2], "v")
    assert np.array_equal(stats, ref[4])
    sc.close()


@pytest.mark.parametrize("shared,masked,size,poison,coherent,want_bary", [
    (True, False, 64, False, False, True), (True, True, 64, False, False, True), (False, False, 64, False, False, True), (False, True, 64, False, False, True),
    (False, True, 16, False, False, True), (True, False, 1, False, False, True),
    (True, False, 64, True, False, True), (False, True, 64, True, False, True),       # non-finite idir -> EXACT instantiation
    # coherent packets without barycentrics: the instantiations that take the narrow-range leaf forms (shared / per-ray origins, masks)
    (True, False, 64, False, True, False), (False, False, 64, False, True, False), (False, True, 64, False, True, False), (False, True, 16, False, True, False),
    (False, True, 64, False, True, True),
])
def test_trace_rays_bit_exact(torch_mod, shared, masked, size, poison, coherent, want_bary):
    name = "atrium:0.05"
    tv, sc, osc = gpu_scene(name)
    cam = util.camera_for(name, tv)
    npk = 24
    origin, dirs, idir, mask, dist, obj, bary = util.secondary_packets(osc, cam, 640, 368, npk, seed=11 + size, shared=shared, masked=masked,
                                                                       size=size, poison=poison, coherent=coherent)
    d2, o2, b2 = dist.copy(), obj.copy(), bary.copy()
    ost = osc.trace_rays(origin, dirs, idir, mask, d2, o2, b2, npk, size, shared, mode=O.MODE_IEEE)
    from snail_amd.scene import Context
    tt = torch_mod.from_numpy
    ctx = Context(tt(origin).cuda(), tt(dirs).cuda(), tt(idir).cuda(), tt(dist.copy()).cuda(), tt(obj.copy()).cuda(), tt(bary.copy()).cuda() if want_bary else None,
                  size=size, shared_origin=shared, mask=None if mask is None else tt(mask).cuda())
    stats = sc.new_stats()
    sc.traverse_primary(ctx, stats=stats)
    torch_mod.cuda.synchronize()
    util.assert_bit_equal(ctx.object.cpu().numpy(), o2, "object")
    util.assert_bit_equal(ctx.distance.cpu().numpy(), d2, "distance")
    if want_bary: util.assert_bit_equal(ctx.barycentric.cpu().numpy(), b2, "barycentric")
    st = stats.cpu().numpy().astype(np.uint64)
    assert st[0] == ost[0] and st[1] == ost[1], (st, ost)
    assert (o2 != 0).any() or poison
    # host-pointer variant gives the same bytes
    d3, o3, b3 = dist.copy(), obj.copy(), bary.copy()
    sc.trace_rays_host(origin, dirs, idir, mask, d3, o3, b3 if want_bary else None, npk, size, shared)
    util.assert_bit_equal(d3, d2, "host distance"); util.assert_bit_equal(o3, o2, "host object")
    sc.close()


@pytest.mark.parametrize("size,poison", [(64, False), (16, False), (64, True)])
def test_trace_shadow_bit_exact(torch_mod, size, poison):
    name = "atrium:0.05"
    tv, sc, osc = gpu_scene(name)
    npk = 32
    origin, dirs, idir, dist = util.shadow_packets(osc, npk, seed=5, size=size)
    if poison:   # SafeInv singularity (dir == -1e-8 -> idir = inf) and axis-parallel rays: the M_EXACT shadow walk,
        # including ComputeMinMax's distance-mask variant (src/rtbase.cpp:99-121) on packets with NaN-producing lanes
        dirs[3, 0:4] = np.float32(-0.00000001); dirs[70, 4:8] = 0.0; dirs[200, 8:12] = np.float32(-0.00000001)
        idir = (np.float32(1.0) / (dirs + np.float32(0.00000001))).astype(np.float32)
    d2 = dist.copy()
    ost = osc.trace_shadow(origin, dirs, idir, d2, npk, size)
    from snail_amd.scene import ShadowContext
    tt = torch_mod.from_numpy
    ctx = ShadowContext(tt(origin).cuda(), tt(dirs).cuda(), tt(idir).cuda(), tt(dist.copy()).cuda(), size=size)
    stats = sc.new_stats()
    sc.traverse_shadow(ctx, stats=stats)
    torch_mod.cuda.synchronize()
    util.assert_bit_equal(ctx.distance.cpu().numpy(), d2, "shadow distance")
    st = stats.cpu().numpy().astype(np.uint64)
    assert st[0] == ost[0] and st[1] == ost[1] and st[3] == ost[3], (st, ost)
    occl = np.isneginf(d2) & ~np.isneginf(dist)
    assert occl.any() and (~np.isneginf(d2)).any()          # both outcomes are exercised
    d3 = dist.copy()
    sc.trace_shadow_host(origin, dirs, idir, d3, npk, size)
    util.assert_bit_equal(d3, d2, "host shadow distance")
    sc.close()


def test_accounting_walk_matches_oracle(torch_mod):
    name = "atrium:0.05"
    tv, sc, osc = gpu_scene(name)
    cam = util.camera_for(name, tv)
    got = sc.account_primary(cam, 640, 368)
    want = osc.account_primary(cam.as_array13(), 640, 368, mode=O.MODE_IEEE)
    assert np.array_equal(got, want), (got, want)
    sc.close()


def test_sse_mode_tolerance(torch_mod):
    """The north_star bar proper: the SAME rays (dir and idir exactly as the reference's SSE generator
    produces them on this CPU: rsqrtps/rcpps + one Newton step) go to the HIP path and to the oracle in
    ORC_MODE_SSE.  The only remaining difference is Inv(det) on a hit (src/triangle.cpp:55: rcpps+NR vs
    IEEE divide), so: hit/miss identical, triId identical except where two candidates are closer than
    the tolerance (tie rule), t/u/v within 1e-4."""
    name = "atrium:0.05"
    tv, sc, osc = gpu_scene(name)
    cam = util.camera_for(name, tv)
    resx, resy = 640, 368
    pk = [(x, y) for y in range(0, resy, 16) for x in range(0, resx, 16)]
    npk = len(pk)
    dirs = np.zeros((npk * 64, 12), dtype=np.float32); idir = np.zeros_like(dirs)
    for i, (x, y) in enumerate(pk):
        d, di = O.gen_packet(cam.as_array13(), resx, resy, x, y, mode=O.MODE_SSE)
        dirs[i * 64:(i + 1) * 64] = d.reshape(64, 12); idir[i * 64:(i + 1) * 64] = di.reshape(64, 12)
    origin = np.repeat(cam.pos.astype(np.float32), 4)[None, :].repeat(npk, axis=0).copy()
    dist = np.full((npk * 64, 4), np.inf, dtype=np.float32)
    obj = np.zeros((npk * 64, 4), dtype=np.int32); bary = np.zeros((npk * 64, 8), dtype=np.float32)
    d2, o2, b2 = dist.copy(), obj.copy(), bary.copy()
    osc.trace_rays(origin, dirs, idir, None, d2, o2, b2, npk, 64, True, mode=O.MODE_SSE)
    d3, o3, b3 = dist.copy(), obj.copy(), bary.copy()
    sc.trace_rays_host(origin, dirs, idir, None, d3, o3, b3, npk, 64, True)
    assert np.array_equal(np.isfinite(d3), np.isfinite(d2))
    hit = np.isfinite(d2)
    assert hit.mean() > 0.9
    scale = np.maximum(1.0, np.abs(d2[hit]))
    assert (np.abs(d3[hit] - d2[hit]) <= TOL * scale).all()
    same = o3 == o2
    assert same[hit].mean() > 0.9999, same[hit].mean()
    u2, v2, u3, v3 = b2[:, :4], b2[:, 4:], b3[:, :4], b3[:, 4:]
    m = hit & same
    assert (np.abs(u3 - u2)[m] <= TOL).all() and (np.abs(v3 - v2)[m] <= TOL).all()
    # where ids differ the two candidates must be a genuine near-tie in t
    diff = hit & ~same
    if diff.any():
        assert (np.abs(d3[diff] - d2[diff]) <= TOL * np.maximum(1.0, np.abs(d2[diff]))).all()
    # frame-level generator difference (IEEE vs SSE rsqrt/rcp) stays inside the t tolerance as well
    frame = sc.trace_primary(cam, resx, resy)
    torch_mod.cuda.synchronize()
    t = osc.render_primary(cam.as_array13(), resx, resy, mode=O.MODE_SSE)[0]
    gt = frame.t.cpu().numpy()
    assert np.array_equal(np.isfinite(gt), np.isfinite(t))
    h2 = np.isfinite(t)
    assert (np.abs(gt[h2] - t[h2]) <= TOL * np.maximum(1.0, np.abs(t[h2]))).all()
    sc.close()


def sse_path_counts(torch_mod, name, resx=1920, resy=1080, arith="ieee"):
    """The HIP path against the arithmetic the reference executes on x86 (ORC_MODE_SSE: rsqrtps / rcpps + one Newton step), at
    BASELINE size.  Returns the counts the north_star bar is about -- bit-exact triId, t/u/v within 1e-4 -- for two legs:
      same rays    : dir / idir exactly as the reference's SSE generator produces them on this CPU go to the HIP path (generic packet
                     entry) and to the oracle in ORC_MODE_SSE; the only remaining difference is Inv(det) on a hit (src/triangle.cpp:55)
      device rays  : the HIP path's own frame (IEEE generator) against the oracle's ORC_MODE_SSE frame"""
    tv, sc, osc = gpu_scene(name)
    sc.set_arith(arith)
    cam = util.camera_for(name, tv)
    cam13 = cam.as_array13()
    pk = [(x, y) for y in range(0, resy, 16) for x in range(0, resx, 16)]
    npk = len(pk)
    dirs = np.zeros((npk * 64, 12), dtype=np.float32); idir = np.zeros_like(dirs)
    for i, (x, y) in enumerate(pk):
        d, di = O.gen_packet(cam13, resx, resy, x, y, mode=O.MODE_SSE)
        dirs[i * 64:(i + 1) * 64] = d.reshape(64, 12); idir[i * 64:(i + 1) * 64] = di.reshape(64, 12)
    origin = np.repeat(cam.pos.astype(np.float32), 4)[None, :].repeat(npk, axis=0).copy()
    dist = np.full((npk * 64, 4), np.inf, dtype=np.float32)
    obj = np.zeros((npk * 64, 4), dtype=np.int32); bary = np.zeros((npk * 64, 8), dtype=np.float32)
    d2, o2, b2 = dist.copy(), obj.copy(), bary.copy()
    osc.trace_rays(origin, dirs, idir, None, d2, o2, b2, npk, 64, True, mode=O.MODE_SSE)
    d3, o3, b3 = dist.copy(), obj.copy(), bary.copy()
    sc.trace_rays_host(origin, dirs, idir, None, d3, o3, b3, npk, 64, True)

    def leg(gt, gid, gu, gv, rt, rid, ru, rv):
        gh, rh = np.isfinite(gt), np.isfinite(rt)
        both = gh & rh
        same = both & (gid == rid)
        diff = both & (gid != rid)
        with np.errstate(invalid="ignore"):
            rel = np.where(both, np.abs(gt - rt) / np.maximum(1.0, np.abs(rt)), 0.0)
            duv = np.where(same, np.maximum(np.abs(gu - ru), np.abs(gv - rv)), 0.0)
        return {"rays": int(gt.size), "hits": int(rh.sum()), "hit_miss_flips": int((gh != rh).sum()), "triId_mismatches": int(diff.sum()),
                # same triangle on both sides: t / u / v outside the north_star tolerance (COUNTS) and the largest deviations
                "t_outside_tol_same_tri": int((rel[same] > TOL).sum()), "uv_outside_tol_same_tri": int((duv[same] > TOL).sum()),
                "max_rel_dt_same_tri": float(rel[same].max()) if same.any() else 0.0, "max_duv_same_tri": float(duv[same].max()) if same.any() else 0.0,
                # different triangles: a near-tie in t (same rays: the only legitimate cause) or another surface altogether (a ray that differs
                # in its last bits passes the other side of a silhouette edge)
                "mismatches_not_near_tie": int((rel[diff] > TOL).sum()), "max_rel_dt_at_mismatch": float(rel[diff].max()) if diff.any() else 0.0}
    res = {"same_rays": leg(d3, o3, b3[:, :4], b3[:, 4:], d2, o2, b2[:, :4], b2[:, 4:])}
    frame = sc.trace_primary(cam, resx, resy)
    torch_mod.cuda.synchronize()
    rt, ru, rv, rid, _ = osc.render_primary(cam13, resx, resy, mode=O.MODE_SSE, threads=16)
    res["device_rays"] = leg(frame.t.cpu().numpy(), frame.tri_id.cpu().numpy(), frame.u.cpu().numpy(), frame.v.cpu().numpy(), rt, rid, ru, rv)
    sc.close()
    return res


@pytest.mark.parametrize("name", ["atrium", "stress"])
def test_sse_path_full_size_counted(torch_mod, name):
    """How far the DEFAULT arithmetic (SNAIL_ARITH_IEEE: veclib's scalar Inv / RSqrt, host-independent results) is from what the reference's
    SSE build computes, at BASELINE size (1920x1080; atrium = configs 1-3, stress = config 5) -- hit/miss flips, triId mismatches and pixels
    outside north_star's 1e-4 are COUNTED and held below the recorded counts of tests/golden/sse_bounds.json (x 1.5 + 16: another CPU's
    rcpps / rsqrtps tables move a few pixels).  This is a regression bound on a documented difference, not the parity claim: parity with
    the SSE path is SNAIL_ARITH_HOST_SSE, where the same comparison gives ZERO everywhere and equal bits (asserted at the end here and, record
    by record, in tests/test_gpu_host_sse.py).  Same rays (only Inv(det) differs): the bar holds without exception in either arithmetic."""
    import json
    res = sse_path_counts(torch_mod, name)
    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sse_bounds.json")))
    keys = ("hit_miss_flips", "triId_mismatches", "t_outside_tol_same_tri", "uv_outside_tol_same_tri", "mismatches_not_near_tie")
    assert gold["by_cpu"], "tests/golden/sse_bounds.json holds no recorded counts"
    for legname in ("same_rays", "device_rays"):
        r = res[legname]
        assert r["rays"] == (1920 * 1080 if legname == "device_rays" else 1920 * 1088)
        assert r["hits"] > 0.5 * r["rays"]
        for key in keys:
            worst = max(e[name][legname][key] for e in gold["by_cpu"].values())
            assert r[key] <= gold["elsewhere"]["factor"] * worst + gold["elsewhere"]["plus"], (legname, key, r[key], worst)
    # same rays: nothing but Inv(det) differs (src/triangle.cpp:55) -- the bar holds without exception: no ray changes between hit and
    # miss, t / u / v within 1e-4 wherever the triangle is the same, and a different triangle only where the two distances tie
    s_ = res["same_rays"]
    assert s_["hit_miss_flips"] == 0 and s_["t_outside_tol_same_tri"] == 0 and s_["uv_outside_tol_same_tri"] == 0 and s_["mismatches_not_near_tie"] == 0, s_
    # ... and in the host's SSE arithmetic the device-rays leg is zero in every column
    z = sse_path_counts(torch_mod, name, arith="host_sse")["device_rays"]
    assert all(z[k] == 0 for k in keys) and z["max_rel_dt_same_tri"] == 0.0 and z["max_duv_same_tri"] == 0.0, z


@pytest.mark.parametrize("refl", [False, True])
def test_config3_full_size_frame_byte_exact(torch_mod, refl):
    """BASELINE config 3 at its own size: atrium 1920x1080, primary + the point light's shadow packets (and with the mirrored bounce),
    frame bytes and TreeStats counters equal to the oracle's Scene::RayTrace restatement."""
    name = "atrium"
    tv, sc, osc = gpu_scene(name)
    cam = util.camera_for(name, tv)
    bmin, bmax = osc.nodes[0]["bmin"], osc.nodes[0]["bmax"]
    c, e = (bmin + bmax) * 0.5, (bmax - bmin)
    lights = np.array([[c[0], c[1] + 0.35 * e[1], c[2], 1.0, 0.9, 0.8, 2.0 * float(e.max())]], dtype=np.float32)     # bench.py --config 3's light
    want, wst = osc.render_whitted(cam.as_array13(), 1920, 1080, lights, mode=O.MODE_IEEE, threads=16, reflections=refl)
    stats = sc.new_stats()
    got = sc.render_whitted(cam, 1920, 1080, lights, stats=stats, reflections=refl)
    torch_mod.cuda.synchronize()
    g = got.cpu().numpy()
    assert np.array_equal(g, want), int((g != want).sum())
    assert np.array_equal(stats.cpu().numpy().astype(np.uint64), wst), (stats.cpu().numpy(), wst)
    assert wst[2] > 1920 * 1088 * (2.5 if refl else 1.3)            # shadow (and mirrored) lanes were traced
    lit = want.reshape(-1, 3).max(axis=1)
    assert (lit > 0).mean() > 0.9 and len(np.unique(lit)) > 100    # a real picture
    sc.close()


@pytest.mark.parametrize("name,resx,resy,nl", [("atrium:0.05", 320, 192, 1), ("atrium:0.05", 250, 130, 0), ("box", 64, 64, 1), ("stress:0.05", 160, 96, 1)])
def test_transparency_stage_bit_exact(torch_mod, name, resx, resy, nl):
    """Scene::TraceTransparency (src/scene_trace.cpp:620-634) staged on the device: continuation rays behind the hits of the caller's
    selector lanes, RayGroup<0,1> through the nested RayTrace -- colours (float) and TreeStats counters bit-identical to the oracle's
    restatement, and to the committed digest of the first case."""
    import hashlib
    import json
    tv, sc, osc = gpu_scene(name)
    cam = util.camera_for(name, tv)
    xy, tp, ip, sel, lights = util.transparency_case(osc, cam, resx, resy, 5)
    lights = lights[:nl]
    want, wst = osc.trace_transparency(cam.as_array13(), resx, resy, xy, tp, sel, lights)
    dev = lambda a: torch_mod.from_numpy(np.ascontiguousarray(a)).cuda()
    stats = sc.new_stats()
    got = sc.trace_transparency(cam, resx, resy, dev(xy), dev(tp), dev(ip), dev(sel), lights, stats=stats)
    torch_mod.cuda.synchronize()
    util.assert_bit_equal(got.cpu().numpy(), want, "transColor")
    assert np.array_equal(stats.cpu().numpy().astype(np.uint64), wst), (stats.cpu().numpy(), wst)
    on = ((sel[:, :, None] >> np.arange(4)[None, None, :]) & 1).astype(bool).reshape(len(xy), 256) & np.isfinite(tp)
    assert wst[2] >= on.sum() > 0 and (want[~on] == 0).all()          # unselected lanes: no ray, black
    if name == "atrium:0.05" and nl == 1:
        g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_transparency.json")))
        assert hashlib.sha256(got.cpu().numpy().tobytes()).hexdigest() == g["sha_color"] and [int(x) for x in wst] == g["stats"]
    sc.close()


@pytest.mark.parametrize("env", [{"SNAIL_DEBUG_NO_PACK": "1"}, {"SNAIL_DEBUG_FORCE_DEEP": "1"}, {"SNAIL_DEBUG_NO_PACK": "1", "SNAIL_DEBUG_FORCE_DEEP": "1"}])
def test_walk_variants_selected_by_scene_size(torch_mod, env):
    """The walks that the test scenes never select by themselves -- two-word stack entries without record prefetch (scenes of more than 2^20
    node slots) and the second stack register pair (trees deeper than 62) -- forced through the library's debug switches in a child
    process (tests/walk_variants_env.py): primary frame, light pipeline with the mirrored bounce, generic and shadow packets, all
    bit-identical to the oracle."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "walk_variants_env.py")], capture_output=True, text=True, timeout=300, cwd=root,
                       env=dict(os.environ, SNAIL_LIB_PATH=os.path.join(root, "snail_amd", "libsnailhip_debug.so"), **env))   # the switches exist in the workbench build only
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["primary"] and d["whitted_refl"] and d["rays"] and d["shadow"], d


@pytest.mark.parametrize("max_leaf", [12, 16, 40, 70])
def test_leaves_of_many_triangles(torch_mod, max_leaf):
    """Caller trees whose leaves hold up to 12 / 16 / 40 / 70 triangles (the builder's tree with small subtrees collapsed): the packet-level
    triangle cull runs with four lanes per triangle, 16 triangles at a time -- every quad of lanes is exercised, leaves of more than 16
    take several rounds, and the narrow leaf forms hand them to the wide one.  Primary frame, light pipeline with the mirrored bounce
    (any-hit leaves, per-ray-origin leaves), TreeStats: bit-identical to the oracle's walk of the same tree."""
    from snail_amd.scene import Scene
    name, resx, resy = "atrium:0.05", 328, 200
    tv, hb, _ = util.scene_pair(name)
    hb2 = util.collapsed_tree(hb, max_leaf)
    osc = O.OracleScene.from_arrays(hb2.tris, hb2.nodes, hb2.depth, hb2.perm)
    cam = util.camera_for(name, tv)
    sc = Scene(hb2, 0)
    assert sc.flags() == (True, True)
    stats = sc.new_stats()
    frame = sc.trace_primary(cam, resx, resy, stats=stats)
    torch_mod.cuda.synchronize()
    ref = osc.render_primary(cam.as_array13(), resx, resy, mode=O.MODE_IEEE)
    compare_frames(frame, ref, "collapsed tree (leaves <= %d)" % max_leaf)
    assert np.array_equal(stats.cpu().numpy().astype(np.uint64), ref[4]), (stats.cpu().numpy(), ref[4])
    bmin, bmax = hb.bbox()
    c, e = (bmin + bmax) * 0.5, (bmax - bmin)
    lights = np.array([[c[0], c[1] + 0.35 * e[1], c[2], 1.0, 0.9, 0.8, 2.0 * float(e.max())]], dtype=np.float32)
    wst = sc.new_stats()
    img = sc.render_whitted(cam, resx, resy, lights, stats=wst, reflections=True)
    torch_mod.cuda.synchronize()
    oimg, ost = osc.render_whitted(cam.as_array13(), resx, resy, lights, reflections=True)
    assert img.cpu().numpy().tobytes() == oimg.tobytes()
    assert np.array_equal(wst.cpu().numpy().astype(np.uint64), ost), (wst.cpu().numpy(), ost)
    sc.close()


def test_non_nested_caller_tree(torch_mod):
    """The C-ABI takes caller trees verbatim; nothing in the reference's walk needs a child box to lie inside its parent's (every box test
    rescans the whole inherited quad range, src/bounding_box.cpp:71-139), while the record-prefetching node loop keeps only the parent's
    survivors in EXEC.  snail_scene_create therefore checks nesting and routes a tree that is not nested to the loop that rescans the
    range: primary frame, the light pipeline with the mirrored bounce, generic and shadow packets -- all bit-identical to the oracle's walk
    of the SAME tree, TreeStats included.  The workbench build with SNAIL_DEBUG_ASSUME_NESTED=1 (the prefetching loop forced onto this
    tree) must differ: the scene discriminates."""
    import json
    import subprocess
    import sys
    from snail_amd.scene import Scene
    name, resx, resy = "atrium:0.02", 328, 200
    tv, hb, _ = util.scene_pair(name)
    hb2 = util.non_nested_tree(hb)
    osc = O.OracleScene.from_arrays(hb2.tris, hb2.nodes, hb2.depth, hb2.perm)
    cam = util.camera_for(name, tv)
    ok = Scene(hb, 0)
    assert ok.flags() == (True, True)
    ok.close()
    sc = Scene(hb2, 0)
    assert sc.flags() == (True, False)
    stats = sc.new_stats()
    frame = sc.trace_primary(cam, resx, resy, stats=stats)
    torch_mod.cuda.synchronize()
    ref = osc.render_primary(cam.as_array13(), resx, resy, mode=O.MODE_IEEE)
    compare_frames(frame, ref, "non-nested tree, primary")
    assert np.array_equal(stats.cpu().numpy().astype(np.uint64), ref[4]), (stats.cpu().numpy(), ref[4])
    # ... and the walk of the reference's own tree differs from it (the shrunk boxes cull what the real ones do not): not a no-op edit
    assert not np.array_equal(ref[4], util.scene_pair(name)[2].render_primary(cam.as_array13(), resx, resy, mode=O.MODE_IEEE)[4])
    bmin, bmax = hb.bbox()
    c, e = (bmin + bmax) * 0.5, (bmax - bmin)
    lights = np.array([[c[0], c[1] + 0.35 * e[1], c[2], 1.0, 0.9, 0.8, 2.0 * float(e.max())]], dtype=np.float32)
    wst = sc.new_stats()
    img = sc.render_whitted(cam, resx, resy, lights, stats=wst, reflections=True)
    torch_mod.cuda.synchronize()
    oimg, ost = osc.render_whitted(cam.as_array13(), resx, resy, lights, reflections=True)
    assert img.cpu().numpy().tobytes() == oimg.tobytes(), "non-nested tree: light pipeline + mirrored bounce"
    assert np.array_equal(wst.cpu().numpy().astype(np.uint64), ost), (wst.cpu().numpy(), ost)
    sc.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for assume, want_equal in (("0", True), ("1", False)):
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "nonnested_env.py")], capture_output=True, text=True, timeout=300, cwd=root,
                           env=dict(os.environ, SNAIL_LIB_PATH=os.path.join(root, "snail_amd", "libsnailhip_debug.so"), SNAIL_DEBUG_ASSUME_NESTED=assume))
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert d["flags"] == [True, False] and d["equal_to_oracle"] is want_equal, d


def test_invalid_arguments_fail_loudly(torch_mod):
    from snail_amd import SnailError
    name = "box"
    tv, sc, osc = gpu_scene(name)
    cam = util.camera_for(name, tv)
    with pytest.raises(SnailError):
        sc.trace_primary(cam, 256, 256, rect=(8, 0, 64, 64))      # rect origin not on the packet grid
    with pytest.raises(SnailError):
        sc.trace_primary(cam, 0, 256)
    sc.close()
    # snail_scene_create validates what it is handed: a walk must not be able to run away on a shared GPU
    from snail_amd import HostBVH
    from snail_amd.scene import Scene
    tv2, hb, _ = util.scene_pair("atrium:0.02")
    assert hb.depth >= 3
    inner = [i for i in range(hb.n_nodes) if not (int(hb.nodes["sub"][i]) & 0x80000000)]
    deep_inner = inner[-1]
    def broken(mutate, depth=None):
        nodes = hb.nodes.copy()
        mutate(nodes)
        return HostBVH(hb.tris, nodes, hb.depth if depth is None else depth, hb.perm)
    def cyc(nodes):     # a back-edge: an inner node's children are the root's children again
        nodes["sub"][deep_inner] = nodes["sub"][0]
    def shared(nodes):  # two parents share one subtree (no cycle, but a node reachable twice)
        a, b = inner[1], inner[2]
        nodes["sub"][b] = nodes["sub"][a]
    for bad in (broken(cyc), broken(shared), broken(lambda n: None, depth=hb.depth - 1)):
        with pytest.raises(SnailError, match="reachable twice|deeper than the declared depth"):
            Scene(bad, 0)
    ok = Scene(broken(lambda n: None, depth=hb.depth + 5), 0)     # an over-stated depth is harmless
    ok.close()


def test_gpu_against_committed_fixtures(torch_mod):
    """HIP path vs the bytes committed under tests/golden/ (oracle ORC_MODE_IEEE outputs + their inputs)."""
    import hashlib
    import json
    import os
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

    def sha(a):
        return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()

    frames = json.load(open(os.path.join(gold, "oracle_frames.json")))
    for key, g in frames.items():
        tv, sc, osc = gpu_scene(g["scene"])
        cam = util.camera_for(g["scene"], tv)
        stats = sc.new_stats()
        fr = sc.trace_primary(cam, g["res"][0], g["res"][1], stats=stats)
        torch_mod.cuda.synchronize()
        assert (sha(fr.t.cpu().numpy()), sha(fr.u.cpu().numpy()), sha(fr.v.cpu().numpy()), sha(fr.tri_id.cpu().numpy())) == \
               (g["sha_t"], g["sha_u"], g["sha_v"], g["sha_id"]), key
        assert stats.cpu().numpy().tolist() == g["stats"]
        assert sc.account_primary(cam, g["res"][0], g["res"][1]).tolist() == g["account"]
        sc.close()
    g = np.load(os.path.join(gold, "oracle_packets_atrium_005.npz"))
    tv, sc, osc = gpu_scene("atrium:0.05")
    for shared, masked in ((1, 0), (1, 1), (0, 0), (0, 1)):
        k = "rays_s%d_m%d_" % (shared, masked)
        d, o, b = g[k + "dist_in"].copy(), np.zeros_like(g[k + "obj_out"]), np.zeros_like(g[k + "bary_out"])
        st = sc.trace_rays_host(g[k + "origin"], g[k + "dir"], g[k + "idir"], g[k + "mask"] if masked else None, d, o, b, 6, 64, bool(shared))
        util.assert_bit_equal(d, g[k + "dist_out"], k + "dist"); util.assert_bit_equal(o, g[k + "obj_out"], k + "obj")
        util.assert_bit_equal(b, g[k + "bary_out"], k + "bary")
        assert st[0] == g[k + "stats"][0] and st[1] == g[k + "stats"][1]
    d = g["shadow_dist_in"].copy()
    st = sc.trace_shadow_host(g["shadow_origin"], g["shadow_dir"], g["shadow_idir"], d, 8, 64)
    util.assert_bit_equal(d, g["shadow_dist_out"], "shadow")
    assert st[0] == g["shadow_stats"][0] and st[1] == g["shadow_stats"][1] and st[3] == g["shadow_stats"][3]
    sc.close()


@pytest.mark.parametrize("refl,depth_mode,host_sse", [(False, False, False), (True, False, False), (False, True, False), (True, False, True), (False, True, True)])
def test_cpp_adapter_end_to_end(torch_mod, tmp_path, refl, depth_mode, host_sse):
    """A C++ host in the reference's shape (tests/cpp/adapter_mock.cpp over include/snail_adapter.hpp, mock types with the reference's
    member names) gets the oracle's bytes from every path of the adapter: the prefetched primary path (HipBVH::BeginFrame + per-packet
    TraversePrimary(Context<1,0>) copies, frame TreeStats delivered), the immediate path (TraverseShadow, TraversePrimary(Context<0,1>)),
    the batched path (ShadowBatch, RayBatch), and the two Render(...) overloads with the reference's signatures (src/render.h:16-23):
    tile list -> planar R, G-R, B-R bytes at data + offsets[k] and image -> rgb8, with the TreeStats they return.  host_sse: the same after
    HipBVH::SetArith(SNAIL_ARITH_HOST_SSE), every expectation from the oracle's ORC_MODE_SSE."""
    MODE = O.MODE_SSE if host_sse else O.MODE_IEEE
    import subprocess
    from snail_amd import render as R
    from tests.test_host_side import build_adapter_mock
    name = "atrium:0.05"
    tv, hb, osc = util.scene_pair(name)
    cam = util.camera_for(name, tv)
    resx, resy = 320, 192                       # the reference's server demands resx % 16 == 0, resy % 64 == 0 (src/server.cpp:227-231)
    d = tmp_path
    hb.nodes.tofile(str(d / "nodes.bin")); hb.tris.tofile(str(d / "tris.bin"))
    cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32); cam13.tofile(str(d / "cam.bin"))
    bmin, bmax = osc.nodes[0]["bmin"], osc.nodes[0]["bmax"]
    c, e = (bmin + bmax) * 0.5, (bmax - bmin)
    lights = np.array([[c[0], c[1] + 0.35 * e[1], c[2], 1.0, 0.9, 0.8, 2.0 * float(e.max())],
                       [c[0] - 0.3 * e[0], c[1] + 0.1 * e[1], c[2] + 0.2 * e[2], 0.3, 0.5, 1.0, 0.6 * float(e.max())]], dtype=np.float32)
    lights.tofile(str(d / "lights.bin"))
    n_sh, n_ry = 19, 13                         # (odd counts: the 8 threads of the concurrency case get uneven shares)
    so, sd, si, sdist = util.shadow_packets(osc, n_sh, 71)
    for nm, a in (("sh_origin", so), ("sh_dir", sd), ("sh_idir", si), ("sh_dist", sdist)):
        a.tofile(str(d / (nm + ".bin")))
    ro, rd, ri, rmask, rdist, robj, rbary = util.secondary_packets(osc, cam, resx, resy, n_ry, 72, shared=False, masked=True)
    for nm, a in (("ry_origin", ro), ("ry_dir", rd), ("ry_idir", ri), ("ry_mask", rmask), ("ry_dist", rdist)):
        a.tofile(str(d / (nm + ".bin")))
    plan = R.ShardPlan.make(resx, resy, 2)
    tiles = plan.tiles[plan.owner == 1]                      # one rank's tiles, as a render node receives them
    offsets = (np.arange(len(tiles), dtype=np.int32)[::-1].copy()) * (3 * 16 * 64)      # any layout of the per-tile buffers: here reversed
    tiles.astype(np.int32).tofile(str(d / "tiles.bin")); offsets.tofile(str(d / "offsets.bin"))
    np.array([hb.depth, resx, resy, n_sh, n_ry, int(refl), int(depth_mode), 0, int(host_sse)], dtype=np.int32).tofile(str(d / "meta.bin"))
    exe = build_adapter_mock(tmp_path)
    r = subprocess.run([exe, str(d)], capture_output=True, text=True)
    assert r.returncode == 0 and "adapter ok" in r.stdout, r.stdout + r.stderr
    stats = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in open(str(d / "stats.txt")).read().splitlines()}
    # prefetched primary frame
    raw = np.fromfile(str(d / "out_primary.bin"), dtype=np.uint8)
    t = raw[:resx * resy * 4].view(np.float32).reshape(resy, resx)
    tid = raw[resx * resy * 4:].view(np.int32).reshape(resy, resx)
    ref = osc.render_primary(cam.as_array13(), resx, resy, mode=MODE)
    util.assert_bit_equal(t, ref[0], "adapter t"); util.assert_bit_equal(tid, ref[3], "adapter triId")
    assert stats["primary"][:2] == [int(ref[4][0]), int(ref[4][1])]
    # shadow packets: immediate (packet 0) and batched (all)
    want = sdist.copy()
    wst = osc.trace_shadow(so, sd, si, want, n_sh, 64, mode=MODE)
    util.assert_bit_equal(np.fromfile(str(d / "out_sh_batch.bin"), dtype=np.float32).reshape(-1, 4), want, "shadow batch")
    util.assert_bit_equal(np.fromfile(str(d / "out_sh_imm.bin"), dtype=np.float32).reshape(-1, 4), want[:64], "shadow immediate")
    assert stats["shadow_batch"] == [int(wst[0]), int(wst[1]), 0, int(wst[3])]
    w0 = sdist[:64].copy(); st0 = osc.trace_shadow(so[:1], sd[:64], si[:64], w0, 1, 64, mode=MODE)
    assert stats["shadow_imm"] == [int(st0[0]), int(st0[1]), 0, int(st0[3])]
    # secondary packets RayGroup<0,1>
    wd, wo, wb = rdist.copy(), robj.copy(), rbary.copy()
    wst = osc.trace_rays(ro, rd, ri, rmask, wd, wo, wb, n_ry, 64, False, mode=MODE)
    raw = np.fromfile(str(d / "out_ry_batch.bin"), dtype=np.uint8)
    nq = n_ry * 64
    util.assert_bit_equal(raw[:nq * 16].view(np.float32).reshape(-1, 4), wd, "rays batch dist")
    util.assert_bit_equal(raw[nq * 16:nq * 32].view(np.int32).reshape(-1, 4), wo, "rays batch obj")
    util.assert_bit_equal(raw[nq * 32:].view(np.float32).reshape(-1, 8), wb, "rays batch bary")
    assert stats["rays_batch"][:2] == [int(wst[0]), int(wst[1])]
    raw = np.fromfile(str(d / "out_ry_imm.bin"), dtype=np.uint8)
    util.assert_bit_equal(raw[:64 * 16].view(np.float32).reshape(-1, 4), wd[:64], "rays immediate dist")
    util.assert_bit_equal(raw[64 * 16:64 * 32].view(np.int32).reshape(-1, 4), wo[:64], "rays immediate obj")
    # the reference's concurrency contract (src/render.cpp:214-267, src/thread_pool.cpp:151-180: `threads` workers share ONE const scene): the same
    # packets, one TraverseShadow / TraversePrimary<0,1> call each, from 8 threads at once -- every packet and the summed TreeStats are the oracle's
    util.assert_bit_equal(np.fromfile(str(d / "out_sh_thr.bin"), dtype=np.float32).reshape(-1, 4), want, "shadow, 8 threads")
    assert stats["shadow_thr"] == stats["shadow_batch"]
    raw = np.fromfile(str(d / "out_ry_thr.bin"), dtype=np.uint8)
    util.assert_bit_equal(raw[:nq * 16].view(np.float32).reshape(-1, 4), wd, "rays, 8 threads, dist")
    util.assert_bit_equal(raw[nq * 16:nq * 32].view(np.int32).reshape(-1, 4), wo, "rays, 8 threads, obj")
    util.assert_bit_equal(raw[nq * 32:].view(np.float32).reshape(-1, 8), wb, "rays, 8 threads, bary")
    assert stats["rays_thr"][:2] == [int(wst[0]), int(wst[1])]
    # the tile API: planar bytes per tile and the rgb8 image, against the oracle's frame
    if depth_mode:
        want_frame = O.shade_depth(ref[0], mode=MODE).reshape(resy, resx, 3)
        wst = ref[4]
    else:
        want_frame, wst = osc.render_whitted(cam.as_array13(), resx, resy, lights, mode=MODE, reflections=refl)
    data = np.fromfile(str(d / "out_tiles.bin"), dtype=np.uint8)
    for k, wp in enumerate(O.planar_encode(want_frame, tiles)):
        assert np.array_equal(data[offsets[k]:offsets[k] + len(wp)], wp), ("tile", k)
    pitch = stats["image"][4]
    img = np.fromfile(str(d / "out_image.bin"), dtype=np.uint8).reshape(resy, pitch)
    assert np.array_equal(img[:, :resx * 3].reshape(resy, resx, 3), want_frame)
    assert (img[:, resx * 3:] == 0xCD).all()                 # row padding untouched
    assert stats["image"][:4] == [int(wst[0]), int(wst[1]), int(wst[2]), int(wst[3])], (stats["image"], wst)
    assert stats["tiles_multi"] == [1, 3]                     # three handles, one frame's tiles dealt over them: same bytes, same counters
    # the tile call traced this rank's tiles only: its counters are the oracle's over exactly those tiles
    if depth_mode:
        mine = np.zeros(4, dtype=np.uint64)
        for x, y, w, h in tiles.tolist():
            mine += osc.render_primary(cam.as_array13(), resx, resy, rect=(x, y, w, h), mode=MODE, threads=1)[4]
        assert stats["tiles"] == [int(mine[0]), int(mine[1]), int(mine[2]), int(mine[3])]
    else:
        assert 0 < stats["tiles"][1] < int(wst[1]) and stats["tiles"][2] >= len(R.tile_packets(tiles)) * 256


@pytest.mark.parametrize("sw", [5, 6, 8, 59])
def test_cpp_adapter_render_honours_or_hands_over(torch_mod, tmp_path, sw):
    """Render(...) with the reference's signatures must not silently drop a switch of the reference's renderer that the device pipeline
    does not implement (gVals[5] stats heat-map, [6] full shading on a scene with shading data, [8] per-rank tint of the tile list): such a
    call is handed to the reference's OWN renderer (here: the mock's generic Render templates) with the frame it will ask for prefetched
    by one launch -- at twice the resolution when 4x antialiasing is on as well (sw = 59: gVals[5] and gVals[9], src/render.cpp:60-62) --
    and the prefetch is released afterwards.  (gVals[9] alone IS implemented on the device: test_antialiased_tile_renderer.)"""
    import subprocess
    from snail_amd import render as R
    from tests.test_host_side import build_adapter_mock
    name = "atrium:0.02"
    tv, hb, osc = util.scene_pair(name)
    cam = util.camera_for(name, tv)
    resx, resy = 128, 64
    d = tmp_path
    hb.nodes.tofile(str(d / "nodes.bin")); hb.tris.tofile(str(d / "tris.bin"))
    np.ascontiguousarray(cam.as_array13(), dtype=np.float32).tofile(str(d / "cam.bin"))
    tiles = R.divide_image(resx, resy)
    tiles.astype(np.int32).tofile(str(d / "tiles.bin")); (np.arange(len(tiles), dtype=np.int32) * (3 * 16 * 64)).tofile(str(d / "offsets.bin"))
    np.array([hb.depth, resx, resy, 0, 0, 0, 1, sw], dtype=np.int32).tofile(str(d / "meta.bin"))
    exe = build_adapter_mock(tmp_path)
    r = subprocess.run([exe, str(d)], capture_output=True, text=True)
    assert r.returncode == 0 and "adapter ok" in r.stdout, r.stdout + r.stderr
    scale = 2 if sw == 59 else 1
    assert "host tile Render: prefetched %d x %d 1" % (resx * scale, resy * scale) in r.stdout, r.stdout
    if sw == 8:     # the tint belongs to the tile-list renderer only: the image call stays on the device
        assert "host image Render" not in r.stdout and "switch 8: tile stats 777 image stats" in r.stdout
    else:
        assert "host image Render: prefetched %d x %d 1" % (resx * scale, resy * scale) in r.stdout, r.stdout
        assert "switch %d: tile stats 777 image stats 778 frame left 0" % sw in r.stdout, r.stdout


@pytest.mark.parametrize("name,resx,resy,mode", [("atrium:0.05", 320, 192, "lights"), ("atrium:0.05", 320, 192, "refl"), ("atrium:0.05", 250, 130, "depth"),
                                                 ("box", 64, 64, "lights"), ("stress:0.05", 160, 96, "lights")])
def test_antialiased_tile_renderer(torch_mod, name, resx, resy, mode):
    """gVals[9], the tile renderer's 4x antialiasing (src/render.cpp:60-62, :71-110), on the device: every image packet is the 2x2 reduction
    of four packets of the double-resolution frame through the same pipeline (light pipeline with or without the mirrored bounce, or
    gVals[1]'s depth shading), in the reference's operation order.  The rgb8 image, the tile list's planar bytes and the TreeStats are
    the oracle's; the tile list dealt over two scene handles (snail_render_tiles_multi) gives the same bytes and counters."""
    from snail_amd import render as R
    from snail_amd.scene import Scene
    tv, sc, osc = gpu_scene(name)
    cam = util.camera_for(name, tv)
    bmin, bmax = osc.nodes[0]["bmin"], osc.nodes[0]["bmax"]
    c, e = (bmin + bmax) * 0.5, (bmax - bmin)
    lights = np.array([[c[0], c[1] + 0.35 * e[1], c[2], 1.0, 0.9, 0.8, 2.0 * float(e.max())]], dtype=np.float32)
    flags = Scene.RENDER_AA4 | (Scene.RENDER_REFLECTIONS if mode == "refl" else 0) | (Scene.RENDER_DEPTH if mode == "depth" else 0)
    want, wst = osc.render_whitted(cam.as_array13(), resx, resy, lights, reflections=mode == "refl", antialias=True, depth=mode == "depth")
    img, st = sc.render_image_host(cam, resx, resy, lights, flags)
    assert np.array_equal(img, want), int((img != want).sum())
    assert np.array_equal(st, wst), (st, wst)
    plain, _ = osc.render_whitted(cam.as_array13(), resx, resy, lights, reflections=mode == "refl", depth=mode == "depth")
    assert not np.array_equal(plain, want)                       # antialiasing changes the picture
    tiles = R.divide_image(resx, resy)
    data, offsets, tst = sc.render_tiles_host(cam, resx, resy, tiles, lights, flags)
    for k, wp in enumerate(O.planar_encode(want, tiles)):
        assert np.array_equal(data[offsets[k]:offsets[k] + len(wp)], wp), ("tile", k)
    sc2 = Scene(sc.bvh, 0)
    data2, _, tst2 = sc.render_tiles_host(cam, resx, resy, tiles, lights, flags, scenes=[sc, sc2])
    assert np.array_equal(data2, data) and np.array_equal(tst2, tst), (tst2, tst)
    with pytest.raises(Exception, match="again"):
        sc.render_tiles_host(cam, resx, resy, tiles, lights, flags, scenes=[sc, sc])      # one handle per share
    sc2.close()
    sc.close()


def test_depth_shading_and_tile_pipeline(torch_mod):
    """f2 row: gVals[1] depth shading + ConvColor + RGB8 store, and the multi-rank tile pipeline executed rank by
    rank in one process (plan -> trace_packets -> shade_depth -> scatter); the collective itself is covered on
    CPU by tests/test_distributed_cpu.py."""
    from snail_amd import render as R
    name = "atrium:0.05"
    tv, sc, osc = gpu_scene(name)
    cam = util.camera_for(name, tv)
    resx, resy = 328, 200
    t_ref = osc.render_primary(cam.as_array13(), resx, resy, mode=O.MODE_IEEE)[0]
    want = O.shade_depth(t_ref).reshape(resy, resx, 3)
    assert want.max() > 0 and (want.reshape(-1, 3).max(axis=0) > 0).all()
    for world in (1, 2, 3):
        plan = R.ShardPlan.make(resx, resy, world)
        frame = torch_mod.zeros((resy, resx, 3), dtype=torch_mod.uint8, device="cuda")
        for r in range(world):
            xy = torch_mod.from_numpy(plan.padded_packets(r)).cuda()
            planes = sc.trace_packets(cam, resx, resy, xy)
            bgr = sc.shade_depth(planes[0])
            assert torch_mod.equal(sc.trace_packets_shaded(cam, resx, resy, xy), bgr)      # the fused kernel epilogue
            sc.packets_bgr_to_frame(xy, bgr, frame)
        torch_mod.cuda.synchronize()
        got = frame.cpu().numpy()
        assert np.array_equal(got, want), (world, int((got != want).sum()))
    # the render node's tile wire format (planes R, G-R, B-R per 16x64 tile) and its inverse, against the oracle
    plan = R.ShardPlan.make(resx, resy, 2)
    for r in range(2):
        tiles = plan.tiles[plan.owner == r]
        xy = torch_mod.from_numpy(R.tile_packets(tiles)).cuda()
        bgr = sc.shade_depth(sc.trace_packets(cam, resx, resy, xy)[0])
        first, off, total = sc.tile_layout(tiles)
        td, fd, od = (torch_mod.from_numpy(np.ascontiguousarray(a)).cuda() for a in (tiles, first, off))
        planar = sc.packets_bgr_to_planar(td, fd, od, bgr, torch_mod.zeros(total, dtype=torch_mod.uint8, device="cuda"))
        # oracle: tiles cut from the oracle's frame, padded rows/columns of edge tiles do not exist in the frame -> compare per tile
        want_planes = O.planar_encode(want, tiles)
        got_planar = planar.cpu().numpy()
        for k, wp in enumerate(want_planes):
            assert np.array_equal(got_planar[off[k]:off[k] + len(wp)], wp), (r, k)
        back = sc.planar_to_frame(td, od, planar, torch_mod.zeros((resy, resx, 3), dtype=torch_mod.uint8, device="cuda")).cpu().numpy()
        for x, y, w, h in tiles.tolist():
            assert np.array_equal(back[y:y + h, x:x + w], want[y:y + h, x:x + w])
    # special values: miss (+inf) -> black, tiny t -> saturated, NaN -> black
    t = torch_mod.tensor([[float("inf"), 1e-6, float("nan"), 1.0] + [2.0] * 252], dtype=torch_mod.float32, device="cuda")
    b = sc.shade_depth(t).cpu().numpy().reshape(-1, 3)
    assert np.array_equal(b[:4], O.shade_depth(t.cpu().numpy())[:4])
    assert tuple(b[0]) == (0, 0, 0) and tuple(b[1]) == (255, 255, 255) and tuple(b[2]) == (0, 0, 0)
    sc.close()


@pytest.mark.parametrize("extra,scaling,res", [([], "strong", (1920, 1080)), (["--rank0-share", "0.25"], "strong", (1920, 1080)),
                                               (["--scaling", "weak"], "weak", (2720, 1528)), (["--config", "3"], "strong", (1920, 1080)),
                                               (["--frames-per-launch", "1"], "strong", (1920, 1080)), (["FULL", "--arith", "ieee"], "strong", (1920, 1080)),
                                               (["FULL", "--config", "3"], "strong", (1920, 1080))])
def test_two_rank_bench_rehearsal(torch_mod, extra, scaling, res):
    """The N>1 flow of bench.py end to end with two ranks sharing this GPU (gloo, payload staged through the host --
    NCCL refuses two ranks on one device): plan, packet-list launches, shading, per-frame gather, rank-0 scatter,
    JSON contract -- in BASELINE's strong-scaling mode (the same 1920x1080 frame cut for 2 ranks; also with rank 0 taking a
    quarter share, and with config 3's light pipeline) and in the weak mode.  The RCCL transport itself is the only part not exercised."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    full = "FULL" in extra          # the bench's own scene (263 K triangles) instead of the small one: the gathered frame is then checked against the committed digest
    extra = [e for e in extra if e != "FULL"]
    tail = ["--gpus", "2", "--steps", "6", "--warmup", "2", "--backend", "gloo", "--full"] + ([] if full else ["--scene", "atrium:0.05"]) + extra
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    if extra in ([], ["--frames-per-launch", "1"], ["--arith", "ieee"]):
        # the PLAIN command, as the driver's scaling run issues it: bench.py starts its own two ranks (a child torch.distributed.run)
        cmd = [sys.executable, os.path.join(root, "bench.py")] + tail
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29517",
               os.path.join(root, "bench.py")] + tail
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["config"]["ranks"] == 2 and d["config"]["frames_in_flight"] >= 1 and d["config"]["lone_launch_ms"] > 0
    assert d["config"]["frames_per_launch"] == (1 if "--frames-per-launch" in extra or "--config" in extra else d["config"]["frames_per_launch"])
    assert "roofline" in d and d["roofline"]["peak"] == pytest.approx(2 * 1228.8)
    assert d["n_gpus"] == 2 and d["steps"] == 6 and d["value"] > 0 and d["scaling"] == scaling
    assert d["config"]["primary_rays_per_step"] == (res[0] // 16) * ((res[1] + 15) // 16) * 256
    assert sum(d["config"]["packets_per_rank"]) * 256 == d["config"]["primary_rays_per_step"]
    if "--rank0-share" in extra:
        assert d["config"]["packets_per_rank"][0] * 3 < d["config"]["packets_per_rank"][1]
    if "--config" in extra:
        assert d["config"]["rays_per_step"] > d["config"]["primary_rays_per_step"]      # + shadow lanes with N.L > 0
    else:
        assert d["config"]["rays_per_step"] == d["config"]["primary_rays_per_step"]
    assert d["config"]["hit_fraction"] > 0.5
    # the line audits its own ranks: what the process group counted, the device of every rank (a rehearsal: both on this box's one GPU, and
    # the line says so), the stream switch, the collective alone
    c = d["config"]
    assert c["rccl_ranks_seen"] == 2 and len(c["rank_devices"]) == 2 and [e["rank"] for e in c["rank_devices"]] == [0, 1]
    assert c["devices_distinct"] is False and c["rank_devices"][0]["uuid"] == c["rank_devices"][1]["uuid"] != ""
    assert c["raw_stream_switch"] in (True, False)
    g = c["gather_alone"]
    assert g["bytes_per_collective"] == c["frames_per_launch"] * max(c["packets_per_rank"]) * 768 and g["ms"] > 0 and g["GBps"] > 0
    # the gathered frame = the oracle's depth-shaded (config 3: lit) frame: checked live on rank 0 (the oracle renders the frame in the timed arithmetic)
    # and, for the bench's own scene, by committed digest as well (host_sse: if the file knows this box's CPU)
    assert d["verified"] is True and d["verification"]["live_oracle"] is True, d["verification"]
    if full:
        assert d["verification"].get("committed") in (True, None) and (d["verification"].get("committed") is True or d["config"]["arith"] == "host_sse")
        assert d["config"]["arith"] == ("ieee" if "--arith" in extra else "host_sse")      # the default arithmetic is the reference's own
    else:
        assert d["verification"].get("committed") is None and "no committed digest" in d["verification"]["note"]


def _bench_json(root, args):
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + args, capture_output=True, text=True, timeout=300, cwd=root, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_run_dumps_the_last_step(torch_mod, tmp_path):
    """A plain bench.py run (no --full) times exactly --steps steps and reports only the headline; --dump-outputs DIR holds the hit records
    the last timed step returned (the buffers are poisoned before the timed region), bit-equal to the oracle's frame of that view."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "dump"
    d = _bench_json(root, ["--gpus", "1", "--steps", "7", "--warmup", "2", "--scene", "atrium:0.05", "--arith", "ieee", "--dump-outputs", str(out)])
    assert d["steps"] == 7 and d["warmup"] == 2 and d["n_gpus"] == 1 and d["full"] is False
    assert d["metric"] == "Mrays/sec (primary)" and d["unit"] == "Mrays/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(d["config"]["rays_per_step"] / d["ms_per_step"] / 1e3, rel=0.01)
    assert not any(k in d for k in ("roofline", "verified", "verification", "cpu_baseline")) and d["config"]["lone_launch_ms"] is None
    assert sorted(os.listdir(str(out))) == ["hit.npy", "t.npy", "tri_id.npy", "u.npy", "v.npy"]
    got = {k: np.load(str(out / (k + ".npy"))) for k in ("t", "u", "v", "tri_id", "hit")}
    assert [got[k].dtype for k in ("t", "u", "v", "tri_id", "hit")] == [np.float32] * 3 + [np.float64, np.float32]
    assert all(np.isfinite(a).all() for a in got.values())
    tv = scenes.scene_by_name("atrium:0.05")
    osc = O.OracleScene(tv)
    t, u, v, tid, _ = osc.render_primary(util.camera_for("atrium:0.05", tv).as_array13(), 1920, 1080, mode=O.MODE_IEEE, threads=8)
    hit = np.isfinite(t)
    assert hit.any() and not hit.all() and np.array_equal(got["hit"], hit.astype(np.float32))
    util.assert_bit_equal(got["t"], np.where(hit, t, np.float32(-1.0)).astype(np.float32), "dumped t (a miss = -1)")
    for a, b, n in ((got["u"], u, "u"), (got["v"], v, "v")):
        util.assert_bit_equal(a, b, "dumped " + n)
    assert np.array_equal(got["tri_id"], tid.astype(np.float64))


def test_bench_dumps_the_same_views_whatever_the_settle_count(torch_mod, tmp_path):
    """With the same arguments a moving camera's timed views -- and so the dumped last step -- do not depend on how many untimed settle frames
    the run measured it needed: two runs with different --settle-ms write the same arrays."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--gpus", "1", "--steps", "5", "--warmup", "3", "--camera-path", "orbit", "--arith", "ieee"]
    a = _bench_json(root, common + ["--settle-ms", "2", "--dump-outputs", str(tmp_path / "a")])
    b = _bench_json(root, common + ["--settle-ms", "40", "--dump-outputs", str(tmp_path / "b")])
    assert a["config"]["camera_path"] == b["config"]["camera_path"] == "orbit" and a["config"]["settle_frames"] < b["config"]["settle_frames"]
    for k in ("t", "u", "v", "tri_id", "hit"):
        x, y = np.load(str(tmp_path / "a" / (k + ".npy"))), np.load(str(tmp_path / "b" / (k + ".npy")))
        assert x.shape == (1080, 1920) and np.array_equal(x.view(np.uint8), y.view(np.uint8)), k


def test_rccl_code_path_single_rank(torch_mod):
    """The same route with the nccl (= RCCL) backend and ONE rank (tests/nccl_single_rank.py, a child process): process-group
    initialisation on the device, dist.gather into per-rank views of one receive buffer -- on the slot's own stream (the default)
    and asynchronously with work.wait() on the slot's stream -- barrier: the calls the 2/4/8-GPU bench makes, with results checked
    against the oracle for both payloads."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "nccl_single_rank.py")], capture_output=True, text=True, timeout=300, cwd=root, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["rgb8_equal"] and d["hits_equal"] and d["moving_equal"] and d["moving_hits_equal"], d
    assert d["uneven_frame_equal"] and d["uneven_stats_equal"], d
    assert d["batched_equal"] and d["batched_stats_equal"] and d["batched_all_frames_equal"], d
    assert d["audit_ok"], d


@pytest.mark.parametrize("name,resx,resy,nl,refl", [("offgrid-in", 328, 200, 2, True), ("offgrid", 320, 192, 1, False),
                                                     ("atrium:0.05", 640, 368, 2, False), ("atrium:0.05", 250, 130, 1, False), ("box", 256, 256, 1, False),
                                                     ("stress:0.05", 320, 192, 3, False), ("atrium:0.05", 320, 192, 0, False),
                                                     ("atrium:0.05", 640, 368, 2, True), ("atrium:0.05", 250, 130, 0, True), ("box", 256, 256, 1, True),
                                                     ("stress:0.05", 320, 192, 3, True), ("chain", 128, 96, 1, True)])
def test_whitted_primary_plus_shadow_bit_exact(torch_mod, name, resx, resy, nl, refl):
    """BASELINE config 3 (primary + one shadow packet per point light), staged on the device, without and with the
    reference's one-bounce reflections (gVals[7]: mirrored packets with per-ray origins and lane masks, shaded and lit like
    the primaries): the rgb8 frame and the TreeStats counters (incl. the traced-ray count = primary + mirrored lanes +
    shadow lanes with N.L > 0) equal the oracle's Scene::RayTrace restatement byte for byte."""
    tv, sc, osc = gpu_scene(name)
    cam = util.camera_for(name, tv)
    bmin, bmax = osc.nodes[0]["bmin"], osc.nodes[0]["bmax"]
    c, e = (bmin + bmax) * 0.5, (bmax - bmin)
    lights = np.array([[c[0], c[1] + 0.35 * e[1], c[2], 1.0, 0.9, 0.8, 2.0 * float(e.max())],
                       [c[0] - 0.3 * e[0], c[1] + 0.1 * e[1], c[2] + 0.2 * e[2], 0.3, 0.5, 1.0, 0.6 * float(e.max())],
                       [cam.pos[0], cam.pos[1], cam.pos[2], 0.6, 0.6, 0.6, 0.25 * float(e.max())]], dtype=np.float32)[:nl]
    want, wst = osc.render_whitted(cam.as_array13(), resx, resy, lights, mode=O.MODE_IEEE, reflections=refl)
    stats = sc.new_stats()
    got = sc.render_whitted(cam, resx, resy, lights, stats=stats, reflections=refl)
    torch_mod.cuda.synchronize()
    g = got.cpu().numpy()
    assert np.array_equal(g, want), (int((g != want).sum()), g.shape)
    assert np.array_equal(stats.cpu().numpy().astype(np.uint64), wst), (stats.cpu().numpy(), wst)
    assert want.max() > 0
    if refl:                                          # the bounce changes the picture and traces more rays
        plain, pst = osc.render_whitted(cam.as_array13(), resx, resy, lights, mode=O.MODE_IEEE)
        assert (plain != want).any() and wst[2] > pst[2]
    if nl and name != "box" and not name.startswith("chain"):                          # (the box's lights sit inside the cube: no lane has N.L > 0)
        assert wst[2] > ((resx + 15) // 16) * ((resy + 15) // 16) * 256        # shadow rays were traced
    sc.close()


@pytest.mark.parametrize("fixture,refl", [("oracle_whitted.json", False), ("oracle_whitted_refl.json", True)])
def test_whitted_against_committed_fixture(torch_mod, fixture, refl):
    import hashlib
    import json
    import os
    g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", fixture)))
    tv, sc, osc = gpu_scene(g["scene"])
    cam = util.camera_for(g["scene"], tv)
    stats = sc.new_stats()
    fr = sc.render_whitted(cam, g["res"][0], g["res"][1], np.asarray(g["lights"], dtype=np.float32), stats=stats, reflections=refl)
    torch_mod.cuda.synchronize()
    assert hashlib.sha256(fr.cpu().numpy().tobytes()).hexdigest() == g["sha_bgr"]
    assert stats.cpu().numpy().tolist() == g["stats"]
    sc.close()


@pytest.mark.parametrize("mode", ["lights", "refl", "depth"])
def test_antialiasing_against_committed_fixture(torch_mod, mode):
    """HIP tile renderer with 4x antialiasing vs the bytes committed under tests/golden/oracle_whitted_aa.json."""
    import hashlib
    import json
    from snail_amd.scene import Scene
    g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_whitted_aa.json")))
    tv, sc, osc = gpu_scene(g["scene"])
    cam = util.camera_for(g["scene"], tv)
    flags = Scene.RENDER_AA4 | (Scene.RENDER_REFLECTIONS if mode == "refl" else 0) | (Scene.RENDER_DEPTH if mode == "depth" else 0)
    img, st = sc.render_image_host(cam, g["res"][0], g["res"][1], np.asarray(g["lights"], dtype=np.float32), flags)
    assert hashlib.sha256(img.tobytes()).hexdigest() == g["modes"][mode]["sha_bgr"]
    assert [int(x) for x in st] == g["modes"][mode]["stats"]
    sc.close()


def test_config4_4k_frame_via_tile_plan(torch_mod):
    """BASELINE config 4 size (3840x2160), traced as eight rank-shards of the reference's 16x64 tiles one after the
    other on this GPU and reassembled; hit records bit-exact vs the oracle frame."""
    from snail_amd import render as R
    name = "atrium"
    tv, sc, osc = gpu_scene(name)
    cam = util.camera_for(name, tv)
    resx, resy = 3840, 2160
    ref = osc.render_primary(cam.as_array13(), resx, resy, mode=O.MODE_IEEE, threads=16)
    plan = R.ShardPlan.make(resx, resy, 8)
    frame = sc.alloc_frame(resx, resy)
    for r in range(8):
        xy = torch_mod.from_numpy(plan.padded_packets(r)).cuda()
        planes = sc.trace_packets(cam, resx, resy, xy)
        sc.packets_to_frame(xy, planes, frame)
    torch_mod.cuda.synchronize()
    compare_frames(frame, ref, "atrium 3840x2160 (8 shards)")
    sc.close()


def test_config5_stress_1m_full_size(torch_mod):
    """BASELINE config 5 scene class: ~1 M triangles (stress), 1920x1080, deep tree; bit-exact vs the oracle."""
    name = "stress"
    tv, sc, osc = gpu_scene(name)
    assert len(tv) > 900000
    cam = util.camera_for(name, tv)
    stats = sc.new_stats()
    frame = sc.trace_primary(cam, 1920, 1080, stats=stats)
    torch_mod.cuda.synchronize()
    ref = osc.render_primary(cam.as_array13(), 1920, 1080, mode=O.MODE_IEEE, threads=16)
    compare_frames(frame, ref, "stress-1M 1920x1080")
    assert np.array_equal(stats.cpu().numpy().astype(np.uint64), ref[4])
    assert np.isfinite(ref[0]).mean() > 0.5
    sc.close()


def test_exact_mode_primary_frame_with_degenerate_triangles(torch_mod):
    """A scene holding zero-area triangles (t0 = 0, it0 = inf, NaN normal: what the reference gets when Repair's
    1e-8 threshold lets one through) disables the FAST/COH arithmetic for the whole scene: every primary packet
    is deferred to the M_EXACT kernel (select-based Min/Max, interval culls).  Results must still be the oracle's, bit for bit."""
    from snail_amd import HostBVH, scenes, survey_camera
    from snail_amd.scene import Scene
    tv = scenes.box_scene()
    p = np.array([[0.2, 0.3, -0.5]] * 3, dtype=np.float32)          # a point-triangle inside the cube
    q = np.array([[-0.4, 0.1, 0.2], [0.4, 0.1, 0.2], [0.0, 0.1, 0.2]], dtype=np.float32)   # collinear
    tv2 = np.concatenate([tv, p[None], q[None]], axis=0)
    hb, osc = HostBVH.build(tv2), O.OracleScene(tv2)
    assert hb.nodes.tobytes() == osc.nodes.tobytes()
    assert not np.isfinite(hb.tris["it0"]).all()
    cam = survey_camera(tv)
    sc = Scene(hb, 0)
    stats = sc.new_stats()
    frame = sc.trace_primary(cam, 256, 256, stats=stats)
    torch_mod.cuda.synchronize()
    ref = osc.render_primary(cam.as_array13(), 256, 256, mode=O.MODE_IEEE)
    compare_frames(frame, ref, "box + degenerate triangles (M_EXACT)")
    assert np.array_equal(stats.cpu().numpy().astype(np.uint64), ref[4])
    # a second launch reuses the re-armed deferred-packet list
    frame2 = sc.trace_primary(cam, 256, 256)
    torch_mod.cuda.synchronize()
    compare_frames(frame2, ref, "second launch")
    sc.close()


@pytest.mark.parametrize("name,resx,resy,nf", [("atrium:0.05", 328, 200, 3), ("stress:0.05", 250, 130, 8), ("box", 256, 256, 2)])
def test_multi_frame_launch_equals_single_frame_launches(torch_mod, name, resx, resy, nf):
    """snail_trace_primary_batch_dev / snail_trace_packets_shaded_batch_dev: ONE launch for several frames, each with its own camera and output
    planes -- hit records, shaded bytes and the summed TreeStats are those of the oracle frame by frame; with a fed-back dispatch order and
    through DistributedRenderer(frames_per_launch=...) (a partial last batch at flush()); and with every packet deferred to the M_EXACT pass
    (the deferred list carries the frame index)."""
    from snail_amd import FPSCamera, HostBVH, scenes, survey_camera
    from snail_amd import render as R
    from snail_amd.scene import Scene
    tv, sc, osc = gpu_scene(name)
    base = util.camera_for(name, tv)
    rng = np.random.RandomState(17)
    bmin, bmax = osc.nodes[0]["bmin"], osc.nodes[0]["bmax"]
    ext = (bmax - bmin)
    cams = [base] + [FPSCamera((base.pos + (rng.rand(3) - 0.5) * 0.05 * ext).astype(np.float32), float(rng.rand() * 6.28), float(rng.rand() - 0.5) * 0.4).camera() for _ in range(nf - 1)]
    refs = [osc.render_primary(c.as_array13(), resx, resy, mode=O.MODE_IEEE) for c in cams]
    outs = [sc.alloc_frame(resx, resy) for _ in range(nf)]
    stats = sc.new_stats()
    n = sc.primary_slots(resx, resy)
    cost = torch_mod.zeros(n, dtype=torch_mod.int32, device="cuda")
    sc.trace_primary_batch(cams, resx, resy, outs, stats=stats, slot_cost=cost)
    torch_mod.cuda.synchronize()
    for k in range(nf):
        compare_frames(outs[k], refs[k], "batched frame %d" % k)
    assert np.array_equal(stats.cpu().numpy().astype(np.uint64), sum(r[4] for r in refs))
    assert int(cost.sum().item()) == int(refs[0][4][1])              # the first frame's node visits
    order = sc.order_from_cost(cost)
    outs2 = [sc.alloc_frame(resx, resy) for _ in range(nf)]
    sc.trace_primary_batch(cams, resx, resy, outs2, order=order)
    torch_mod.cuda.synchronize()
    for k in range(nf):
        compare_frames(outs2[k], refs[k], "batched + ordered frame %d" % k)
    # the packet-list form with the fused depth shading (a rank's share of the frames)
    plan = R.ShardPlan.make(resx, resy, 2)
    xy = torch_mod.from_numpy(plan.packets[1]).cuda()
    bg = [torch_mod.zeros((len(plan.packets[1]), 256, 3), dtype=torch_mod.uint8, device="cuda") for _ in range(nf)]
    sc.trace_packets_shaded_batch(cams, resx, resy, xy, bg)
    for k in range(nf):
        assert torch_mod.equal(bg[k], sc.trace_packets_shaded(cams[k], resx, resy, xy)), k
    # through the renderer: nf + 1 frames with batches of min(nf, 3): full batches and a partial one at flush()
    rnd = R.DistributedRenderer(sc, resx, resy, frames_per_launch=min(nf, 3))
    for c in cams + [cams[0]]:
        rnd.render(c)
    fr = rnd.flush()
    torch_mod.cuda.synchronize()
    compare_frames(fr, refs[0], "renderer, last frame of a partial batch")
    sc.close()
    if name == "box":   # every packet deferred (a scene with non-finite records): the M_EXACT pass decodes frame and packet
        p = np.array([[0.2, 0.3, -0.5]] * 3, dtype=np.float32)
        tv2 = np.concatenate([scenes.box_scene(), p[None]], axis=0)
        hb, osc2 = HostBVH.build(tv2), O.OracleScene(tv2)
        sc2 = Scene(hb, 0)
        refs2 = [osc2.render_primary(c.as_array13(), resx, resy, mode=O.MODE_IEEE) for c in cams]
        outs3 = [sc2.alloc_frame(resx, resy) for _ in range(nf)]
        st2 = sc2.new_stats()
        sc2.trace_primary_batch(cams, resx, resy, outs3, stats=st2)
        torch_mod.cuda.synchronize()
        for k in range(nf):
            compare_frames(outs3[k], refs2[k], "deferred batched frame %d" % k)
        assert np.array_equal(st2.cpu().numpy().astype(np.uint64), sum(r[4] for r in refs2))
        sc2.close()


def test_every_sign_octant_and_walk_variant(torch_mod):
    """The node loop exists once per sign octant (coherent packets) plus once for non-coherent packets, for closest-hit and for
    any-hit walks: cameras looking into all eight octants from inside the atrium, with a light, so that every variant runs.
    Hit records, shaded frames and counters equal the oracle's bit for bit; the test checks itself that all octants occur."""
    import math
    name = "atrium:0.05"
    tv, sc, osc = gpu_scene(name)
    pos, _, _ = scenes.atrium_camera()
    bmin, bmax = osc.nodes[0]["bmin"], osc.nodes[0]["bmax"]
    c, e = (bmin + bmax) * 0.5, (bmax - bmin)
    lights = np.array([[c[0] + 0.1 * e[0], c[1] + 0.2 * e[1], c[2] - 0.1 * e[2], 1.0, 0.9, 0.8, 2.0 * float(e.max())]], dtype=np.float32)
    resx, resy = 192, 160
    seen_primary, seen_mixed = set(), 0
    for yaw in (0.3, 0.3 + math.pi / 2, 0.3 + math.pi, 0.3 + 3 * math.pi / 2):
        for pitch in (0.7, -0.7):
            cam = FPSCamera(np.asarray(pos, dtype=np.float32), yaw, pitch).camera()
            for py in range(0, resy, 16):
                for px in range(0, resx, 16):
                    d, idir = O.gen_packet(cam.as_array13(), resx, resy, px, py)
                    sg = np.signbit(idir.reshape(64, 3, 4)).transpose(1, 0, 2).reshape(3, -1)
                    if all(sg[k].all() or (~sg[k]).all() for k in range(3)):
                        seen_primary.add(int(sg[0, 0]) | int(sg[1, 0]) << 1 | int(sg[2, 0]) << 2)
                    else:
                        seen_mixed += 1
            want = osc.render_primary(cam.as_array13(), resx, resy, mode=O.MODE_IEEE)
            stats = sc.new_stats()
            fr = sc.trace_primary(cam, resx, resy, stats=stats)
            torch_mod.cuda.synchronize()
            for got, w, nm in zip((fr.t, fr.u, fr.v, fr.tri_id), want[:4], "t u v id".split()):
                util.assert_bit_equal(got.cpu().numpy(), w, "%s yaw %.2f pitch %.2f" % (nm, yaw, pitch))
            assert np.array_equal(stats.cpu().numpy().astype(np.uint64), want[4])
            wimg, wst = osc.render_whitted(cam.as_array13(), resx, resy, lights, mode=O.MODE_IEEE, reflections=True)
            stats = sc.new_stats()
            img = sc.render_whitted(cam, resx, resy, lights, stats=stats, reflections=True)
            torch_mod.cuda.synchronize()
            assert np.array_equal(img.cpu().numpy(), wimg), (yaw, pitch)
            assert np.array_equal(stats.cpu().numpy().astype(np.uint64), wst), (yaw, pitch)
    assert seen_primary == set(range(8)) and seen_mixed > 0, (seen_primary, seen_mixed)
    sc.close()


@pytest.mark.parametrize("name,max_leaf", [("atrium:0.05", 4), ("box", 1), ("stress:0.05", 8), ("chain", 4)])
def test_gpu_lbvh_builder_option(torch_mod, name, max_leaf):
    """The GPU builder option (snail_scene_create_lbvh; not the parity tree): (1) the tree is a valid BVH in the reference's record
    formats -- children adjacent and inside their parent, the leaves partition the triangle array, triangle records bit-identical to
    Triangle::ComputeData of the permuted input; (2) the traversal kernels on THAT tree equal the oracle's walk of the same tree bit
    for bit (hit records and counters); (3) the picture agrees with the SAH tree's: same distances except where the reference's
    order-dependent packet culls differ, same input triangle wherever the distance is the same."""
    from snail_amd import HostBVH
    from snail_amd.scene import Scene
    tv, sc_sah, osc = gpu_scene(name)
    cam = util.camera_for(name, tv)
    sc = Scene.from_lbvh(tv, 0, max_leaf_tris=max_leaf)
    n = len(tv)
    nodes, tris, perm = sc.bvh.nodes, sc.bvh.tris, sc.perm
    assert sorted(perm.tolist()) == list(range(n)) and len(nodes) == 2 * n - 1
    want_tris = HostBVH.triangles(np.asarray(tv, dtype=np.float32).reshape(-1, 3, 3)[perm])
    for f in ("a", "ba", "ca", "t0", "it0", "plane"):
        util.assert_bit_equal(tris[f], want_tris[f], "triangle record field " + f)
    # (1) topology: the validity walk of tests/lbvh_ref.py (it also holds the records to its own restatement of ComputeData)
    from tests import lbvh_ref
    lbvh_ref.check_tree(nodes, tris, perm, tv, max_leaf, sc.bvh.depth)
    # (2) the oracle walks the same tree
    osc2 = O.OracleScene.__new__(O.OracleScene)
    osc2.tris = np.ascontiguousarray(tris.view(O.TRI_DTYPE)); osc2.nodes = np.ascontiguousarray(nodes.view(O.NODE_DTYPE)); osc2.depth = sc.bvh.depth; osc2.perm = perm
    resx, resy = 320, 192
    want = osc2.render_primary(cam.as_array13(), resx, resy, mode=O.MODE_IEEE)
    stats = sc.new_stats()
    fr = sc.trace_primary(cam, resx, resy, stats=stats)
    torch_mod.cuda.synchronize()
    for got, w, nm in zip((fr.t, fr.u, fr.v, fr.tri_id), want[:4], "t u v id".split()):
        util.assert_bit_equal(got.cpu().numpy(), w, "lbvh " + nm)
    assert np.array_equal(stats.cpu().numpy().astype(np.uint64), want[4])
    # (3) against the SAH tree
    fs = sc_sah.trace_primary(cam, resx, resy)
    torch_mod.cuda.synchronize()
    t1, t2 = fr.t.cpu().numpy(), fs.t.cpu().numpy()
    same_t = t1.view(np.uint32) == t2.view(np.uint32)
    assert same_t.mean() > 0.995, same_t.mean()
    assert (np.isfinite(t1) == np.isfinite(t2)).mean() > 0.999
    hit = same_t & np.isfinite(t1)
    src1 = perm[fr.tri_id.cpu().numpy()[hit]]
    src2 = sc_sah.bvh.perm[fs.tri_id.cpu().numpy()[hit]]
    assert (src1 == src2).mean() > 0.995
    assert sc.build_ms > 0.0
    # the downloaded arrays are a valid input for snail_scene_create (unused slots are empty leaves): re-upload, same picture
    from snail_amd.scene import Scene as _Scene
    sc2 = _Scene(sc.bvh, 0)
    fr2 = sc2.trace_primary(cam, resx, resy)
    torch_mod.cuda.synchronize()
    assert torch_mod.equal(fr2.t, fr.t) and torch_mod.equal(fr2.tri_id, fr.tri_id)
    sc2.close()
    sc.close()
    sc_sah.close()


def test_dev_entry_points_are_graph_capturable(torch_mod):
    """include/snail_hip.h promises that the *_dev entry points never synchronise and can be captured into a HIP graph once their
    scratch exists: capture one primary frame and one staged config-3 frame, replay, compare with the direct launches."""
    name = "atrium:0.05"
    tv, sc, osc = gpu_scene(name)
    cam = util.camera_for(name, tv)
    resx, resy = 320, 192
    lights = np.array([[0.0, 10.0, 0.0, 1.0, 0.9, 0.8, 90.0]], dtype=np.float32)
    ref = sc.trace_primary(cam, resx, resy)
    ref_img = sc.render_whitted(cam, resx, resy, lights, reflections=True)
    for _ in range(10):                                   # every round-robin scratch slot allocated
        sc.trace_primary(cam, resx, resy); sc.render_whitted(cam, resx, resy, lights, reflections=True)
    torch_mod.cuda.synchronize()
    fr = sc.alloc_frame(resx, resy)
    img = torch_mod.zeros_like(ref_img)
    g = torch_mod.cuda.CUDAGraph()
    with torch_mod.cuda.graph(g):
        sc.trace_primary(cam, resx, resy, out=fr)
        sc.render_whitted(cam, resx, resy, lights, out=img, reflections=True)
    fr.t.fill_(0); img.fill_(0)
    for _ in range(3):
        g.replay()
    torch_mod.cuda.synchronize()
    assert torch_mod.equal(fr.t, ref.t) and torch_mod.equal(fr.tri_id, ref.tri_id) and torch_mod.equal(fr.u, ref.u)
    assert torch_mod.equal(img, ref_img)
    # round 4: the staged pipeline with its per-stage dispatch orders, the order kernel itself, and the host's SSE arithmetic, captured as well
    n = sc.primary_slots(resx, resy)
    cost = torch_mod.zeros((sc.WHITTED_STAGES, n), dtype=torch_mod.int32, device="cuda")
    order = torch_mod.empty_like(cost)
    sc.render_whitted(cam, resx, resy, lights, reflections=True, slot_cost=cost)
    for k in range(sc.WHITTED_STAGES):
        sc.order_from_cost(cost[k], order[k])
    sc.set_arith("host_sse")
    ref_sse = sc.render_whitted(cam, resx, resy, lights, reflections=True)
    for _ in range(10):
        sc.render_whitted(cam, resx, resy, lights, reflections=True, order=order, slot_cost=cost)
    torch_mod.cuda.synchronize()
    img2 = torch_mod.zeros_like(ref_img)
    order2 = torch_mod.empty_like(order)
    g2 = torch_mod.cuda.CUDAGraph()
    with torch_mod.cuda.graph(g2):
        sc.render_whitted(cam, resx, resy, lights, out=img2, reflections=True, order=order, slot_cost=cost)
        for k in range(sc.WHITTED_STAGES):
            sc.order_from_cost(cost[k], order2[k])
    img2.fill_(0)
    for _ in range(3):
        g2.replay()
    torch_mod.cuda.synchronize()
    assert torch_mod.equal(img2, ref_sse) and not torch_mod.equal(ref_sse, ref_img)
    for k in range(sc.WHITTED_STAGES):
        assert torch_mod.equal(torch_mod.sort(order2[k]).values, torch_mod.arange(n, dtype=torch_mod.int32, device="cuda"))
    sc.close()


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_gpu_lbvh_tiny_inputs(torch_mod, n):
    """Edge cases of the GPU builder: a single triangle (one leaf, no internal node), two, three, five."""
    from snail_amd.scene import Scene
    tv = np.ascontiguousarray(scenes.box_scene()[:n])
    cam = util.camera_for("box", scenes.box_scene())
    sc = Scene.from_lbvh(tv, 0, max_leaf_tris=1)
    osc2 = O.OracleScene.__new__(O.OracleScene)
    osc2.tris = np.ascontiguousarray(sc.bvh.tris.view(O.TRI_DTYPE)); osc2.nodes = np.ascontiguousarray(sc.bvh.nodes.view(O.NODE_DTYPE))
    osc2.depth = sc.bvh.depth; osc2.perm = sc.perm
    assert len(sc.bvh.nodes) == 2 * n - 1 and sorted(sc.perm.tolist()) == list(range(n))
    want = osc2.render_primary(cam.as_array13(), 128, 96, mode=O.MODE_IEEE)
    fr = sc.trace_primary(cam, 128, 96)
    torch_mod.cuda.synchronize()
    for got, w, nm in zip((fr.t, fr.u, fr.v, fr.tri_id), want[:4], "t u v id".split()):
        util.assert_bit_equal(got.cpu().numpy(), w, "lbvh n=%d %s" % (n, nm))
    assert np.isfinite(want[0]).any()
    sc.close()


@pytest.mark.parametrize("name", ["atrium:0.05", "stress:0.05", "box"])
def test_fuzzed_cameras_and_frame_sizes(torch_mod, name):
    """Seeded fuzz: cameras anywhere in and around the scene (also far outside, looking away, axis-parallel view directions, very
    narrow and very wide fields of view), frame sizes that are not multiples of the packet or the tile, down to 1x1 -- primary hit
    records and the staged config-3 frame (with the mirrored bounce) against the oracle, bit for bit, counters included."""
    import math
    tv, sc, osc = gpu_scene(name)
    rng = np.random.RandomState(sum(name.encode()) % 1000 + 7)
    bmin, bmax = osc.nodes[0]["bmin"], osc.nodes[0]["bmax"]
    c, e = (bmin + bmax) * 0.5, (bmax - bmin)
    sizes = [(1, 1), (5, 3), (16, 16), (17, 33), (100, 7), (64, 130), (129, 65), (200, 120)]
    for case in range(16):
        where = rng.rand()
        pos = c + (rng.rand(3) - 0.5) * e * (0.8 if where < 0.6 else 3.5)
        yaw = [0.0, math.pi / 2, math.pi, rng.rand() * 2 * math.pi][case % 4] if case % 3 == 0 else rng.rand() * 2 * math.pi
        pitch = 0.0 if case % 5 == 0 else (rng.rand() - 0.5) * 2.6
        pd = [1.0, 0.15, 6.0, 1.0][case % 4]
        cam = FPSCamera(pos.astype(np.float32), yaw, pitch, plane_dist=pd).camera()
        resx, resy = sizes[case % len(sizes)]
        want = osc.render_primary(cam.as_array13(), resx, resy, mode=O.MODE_IEEE)
        stats = sc.new_stats()
        fr = sc.trace_primary(cam, resx, resy, stats=stats)
        torch_mod.cuda.synchronize()
        for got, w, nm in zip((fr.t, fr.u, fr.v, fr.tri_id), want[:4], "t u v id".split()):
            util.assert_bit_equal(got.cpu().numpy(), w, "%s case %d %s" % (name, case, nm))
        assert np.array_equal(stats.cpu().numpy().astype(np.uint64), want[4]), (case, stats.cpu().numpy(), want[4])
        lights = np.array([[*(c + (rng.rand(3) - 0.5) * e * 0.7), 1.0, 0.8, 0.6, float(e.max()) * (0.3 + 2.0 * rng.rand())],
                           [*(pos + 0.01), 0.5, 0.5, 0.9, float(e.max())]], dtype=np.float32)[:1 + case % 2]
        refl = case % 2 == 0
        wimg, wst = osc.render_whitted(cam.as_array13(), resx, resy, lights, mode=O.MODE_IEEE, reflections=refl)
        stats = sc.new_stats()
        img = sc.render_whitted(cam, resx, resy, lights, stats=stats, reflections=refl)
        torch_mod.cuda.synchronize()
        assert np.array_equal(img.cpu().numpy(), wimg), (name, case, int((img.cpu().numpy() != wimg).sum()))
        assert np.array_equal(stats.cpu().numpy().astype(np.uint64), wst), (name, case, stats.cpu().numpy(), wst)
    sc.close()


def test_many_streams_share_one_scene_handle(torch_mod):
    """tools/stress_streams.py: 600 launches over 6 HIP streams mixing every device entry point on one scene handle (the round-robin
    scratch slots and their events), every result equal to the one computed alone."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "stress_streams.py"), "600"], capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0 and "mismatches: 0" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


def test_config3_shading_through_the_tile_plan(torch_mod):
    """BASELINE configs 3 x 4: the staged config-3 pipeline on each rank's packet list (with the mirrored bounce), gathered and
    scattered like the depth-shaded tiles -- for 1, 2 and 3 ranks on this GPU the frame and the summed counters equal the oracle's."""
    from snail_amd import render as R
    name = "atrium:0.05"
    tv, sc, osc = gpu_scene(name)
    cam = util.camera_for(name, tv)
    resx, resy = 328, 200
    bmin, bmax = osc.nodes[0]["bmin"], osc.nodes[0]["bmax"]
    c, e = (bmin + bmax) * 0.5, (bmax - bmin)
    lights = np.array([[c[0], c[1] + 0.35 * e[1], c[2], 1.0, 0.9, 0.8, 2.0 * float(e.max())]], dtype=np.float32)
    for refl in (False, True):
        want, wst = osc.render_whitted(cam.as_array13(), resx, resy, lights, mode=O.MODE_IEEE, reflections=refl)
        for world in (1, 2, 3):
            plan = R.ShardPlan.make(resx, resy, world)
            frame = torch_mod.zeros((resy, resx, 3), dtype=torch_mod.uint8, device="cuda")
            stats = sc.new_stats()
            for r in range(world):
                xy = torch_mod.from_numpy(plan.packets[r]).cuda()          # unpadded: every packet exactly once, so the counters add up
                bgr = sc.render_whitted_packets(cam, resx, resy, xy, lights, stats=stats, reflections=refl)
                sc.packets_bgr_to_frame(xy, bgr, frame)
            torch_mod.cuda.synchronize()
            got = frame.cpu().numpy()
            assert np.array_equal(got, want), (refl, world, int((got != want).sum()))
            assert np.array_equal(stats.cpu().numpy().astype(np.uint64), wst), (refl, world, stats.cpu().numpy(), wst)
    sc.close()


@pytest.mark.parametrize("name,resx,resy", [("atrium:0.05", 640, 368), ("stress:0.05", 250, 130), ("box", 16, 16)])
def test_dispatch_order_feedback_changes_nothing_but_the_order(torch_mod, name, resx, resy):
    """snail_trace_primary_ordered_dev / snail_trace_packets_ordered_dev / snail_order_from_cost_dev: the per-slot costs add up to
    the frame's node-visit counter, the derived order is a permutation with non-increasing cost classes, and a frame dispatched in that
    order (or in a reversed / random one) has the hit records and counters of the oracle.  DistributedRenderer(feedback_order=True)
    end to end."""
    from snail_amd import render as R
    tv, sc, osc = gpu_scene(name)
    cam = util.camera_for(name, tv)
    ref = osc.render_primary(cam.as_array13(), resx, resy, mode=O.MODE_IEEE)
    n = sc.primary_slots(resx, resy)
    assert n % 128 == 0 and n >= ((resx + 15) // 16) * ((resy + 15) // 16)
    cost = torch_mod.full((n,), -7, dtype=torch_mod.int32, device="cuda")
    stats = sc.new_stats()
    frame = sc.trace_primary(cam, resx, resy, stats=stats, slot_cost=cost)
    order = sc.order_from_cost(cost)
    torch_mod.cuda.synchronize()
    compare_frames(frame, ref, "cost pass")
    c, o = cost.cpu().numpy(), order.cpu().numpy()
    assert (c >= 0).all() and int(c.sum()) == int(ref[4][1]), (int(c.sum()), ref[4])          # every slot written; sum = TreeStats iters
    kind = util.check_derived_order(c, o)            # a permutation: sorted by cost class for heavy-tailed costs, the built-in order otherwise (round 5)
    shift = 0
    while (int(c.max()) >> shift) > 4095: shift += 1
    rng = np.random.default_rng(5)
    if kind == "built-in":                           # ... and a cost array with a tail gets the sorted order: the same costs with one slot in fifty made 40 x heavier
        tail = c.copy(); tail[::50] = tail[::50] * 40 + 400
        ot = sc.order_from_cost(torch_mod.from_numpy(tail.astype(np.int32)).cuda()).cpu().numpy()
        assert util.check_derived_order(tail, ot) == "sorted"
        o = ot
    for label, perm in (("heaviest first", o), ("lightest first", o[::-1].copy()), ("random", rng.permutation(n).astype(np.int32))):
        stats2 = sc.new_stats()
        cost2 = torch_mod.zeros_like(cost)
        f2 = sc.trace_primary(cam, resx, resy, stats=stats2, order=torch_mod.from_numpy(np.ascontiguousarray(perm)).cuda(), slot_cost=cost2)
        torch_mod.cuda.synchronize()
        compare_frames(f2, ref, label)
        assert np.array_equal(stats2.cpu().numpy().astype(np.uint64), ref[4]), label
        assert np.array_equal(cost2.cpu().numpy(), c), label
    # the next order derived INSIDE the launch (snail_trace_primary_batch_reorder_dev: the last workgroup of the deferred-packet pass sorts the costs the
    # traversal kernel has just written -- no launch of its own): the same costs, a permutation with the stand-alone sort's classes in descending order,
    # hit records untouched; also IN PLACE (next_order = the order the launch reads) and for a two-frame launch
    def classes_descend(perm_):
        return util.check_derived_order(c, perm_) == kind
    nxt = torch_mod.full((n,), -1, dtype=torch_mod.int32, device="cuda")
    cost3 = torch_mod.zeros_like(cost)
    outs = [sc.alloc_frame(resx, resy)]
    sc.trace_primary_batch([cam], resx, resy, outs, slot_cost=cost3, next_order=nxt)
    torch_mod.cuda.synchronize()
    o3 = nxt.cpu().numpy()
    compare_frames(outs[0], ref, "reorder launch")
    assert np.array_equal(cost3.cpu().numpy(), c) and np.array_equal(np.sort(o3), np.arange(n)) and classes_descend(o3)
    buf = torch_mod.from_numpy(o[::-1].copy()).cuda()             # read lightest first, rewritten heaviest first
    outs2 = [sc.alloc_frame(resx, resy), sc.alloc_frame(resx, resy)]
    st4 = sc.new_stats()
    sc.trace_primary_batch([cam, cam], resx, resy, outs2, stats=st4, order=buf, slot_cost=cost3, next_order=buf)
    torch_mod.cuda.synchronize()
    o4 = buf.cpu().numpy()
    for f in outs2:
        compare_frames(f, ref, "reorder launch, in place, two frames")
    assert np.array_equal(st4.cpu().numpy().astype(np.uint64), 2 * ref[4])
    assert np.array_equal(np.sort(o4), np.arange(n)) and classes_descend(o4) and np.array_equal(cost3.cpu().numpy(), c)
    # ... and with the costs declared exact (SNAIL_ORDER_SORTED: the same camera will use the order): sorted whatever their shape
    sc.trace_primary_batch([cam], resx, resy, outs, slot_cost=cost3, next_order=nxt, order_exact=True)
    torch_mod.cuda.synchronize()
    compare_frames(outs[0], ref, "reorder launch, exact costs")
    assert util.check_derived_order(c, nxt.cpu().numpy(), exact=True) == "sorted"
    with pytest.raises(Exception, match="d_slot_cost"):
        sc.trace_primary_batch([cam], resx, resy, outs, next_order=nxt)
    # packet-list form
    plan = R.ShardPlan.make(resx, resy, 1)
    xy = torch_mod.from_numpy(plan.packets[0]).cuda()
    m = int(xy.shape[0])
    pc = torch_mod.zeros(m, dtype=torch_mod.int32, device="cuda")
    base = sc.trace_packets(cam, resx, resy, xy)
    sc.trace_packets(cam, resx, resy, xy, slot_cost=pc)
    po = sc.order_from_cost(pc)
    stats3 = sc.new_stats()
    got = sc.trace_packets(cam, resx, resy, xy, stats=stats3, order=po)
    torch_mod.cuda.synchronize()
    assert np.array_equal(np.sort(po.cpu().numpy()), np.arange(m))
    assert int(pc.sum().item()) == int(ref[4][1])
    for a, b in zip(got, base):
        assert torch_mod.equal(a.view(torch_mod.int32), b.view(torch_mod.int32))
    assert np.array_equal(stats3.cpu().numpy().astype(np.uint64), ref[4])
    with pytest.raises(ValueError):
        sc.trace_primary(cam, resx, resy, order=torch_mod.zeros(n + 1, dtype=torch_mod.int32, device="cuda"))
    # an order with out-of-range entries is refused entry by entry (no out-of-bounds access, the other packets are traced)
    bad = o.copy(); bad[::7] = n + 5; bad[3] = -1
    sc.trace_primary(cam, resx, resy, order=torch_mod.from_numpy(bad).cuda())
    torch_mod.cuda.synchronize()
    # the sort alone: sizes around the block size, constant / negative / huge costs
    for m2, gen in ((1, lambda k: np.zeros(k)), (1023, lambda k: rng.integers(0, 50, k)), (1025, lambda k: rng.integers(-5, 3, k)),
                    (200_003, lambda k: rng.integers(0, 2**31 - 1, k)), (4096, lambda k: np.full(k, 17)),
                    (49152, lambda k: np.full(k, 70000))):      # (the largest sum the one-read form can meet: 49152 x 65535 > 2^31)
        cst = gen(m2).astype(np.int32)
        od = sc.order_from_cost(torch_mod.from_numpy(cst).cuda()).cpu().numpy()
        # (up to 49152 slots: sorted for heavy-tailed costs, the built-in order otherwise; beyond: the multi-pass kernel, always sorted)
        if m2 <= 49152:
            util.check_derived_order(cst, od)
        else:
            assert np.array_equal(np.sort(od), np.arange(m2)), m2
            sh = 0
            while (max(int(cst.max()), 0) >> sh) > 4095: sh += 1
            assert (np.diff(np.minimum(np.maximum(cst[od], 0) >> sh, 4095)) <= 0).all(), m2
    # round 4's one-read form (up to 49152 slots, 16-byte aligned input): the bench's sizes (8192 = 1080p, 32640 = 4K: more than 32 KB of
    # dynamic LDS), its limits (49152 / 49153: the multi-pass kernel again), ragged tails, an unaligned input (multi-pass kernel), and costs
    # beyond 16 bits (clamped: every slot of 65535 visits or more shares the heaviest class)
    for m2, hi, off in ((8192, 3000, 0), (32640, 60000, 0), (49152, 65535, 0), (49153, 65535, 0), (8191, 500, 0), (8189, 500, 0), (5, 9, 0), (8192, 3000, 1),
                        (4097, 1 << 20, 0)):
      for tailed in (False, True):                                # flat costs (p99 ~ 2x the mean: built-in order) and heavy-tailed ones (p99 ~ 12x: sorted)
        cst = rng.integers(0, (hi >> 3 if tailed else hi) + 1, m2 + off).astype(np.int32)
        cst[rng.integers(0, m2 + off, max(1, m2 // 50))] = hi
        dev_c = torch_mod.from_numpy(cst).cuda()[off:]            # off = 1: a view that starts 4 bytes into the allocation
        od = sc.order_from_cost(dev_c).cpu().numpy()
        lds_form = m2 <= 49152 and off == 0
        if lds_form:
            kind = util.check_derived_order(cst[off:], od)
            if 100 <= m2 and hi <= 65535:
                assert kind == ("sorted" if tailed else "built-in"), (m2, hi, tailed, kind)
            # costs the caller declares exact (SNAIL_ORDER_SORTED): sorted whatever their shape
            assert util.check_derived_order(cst[off:], sc.order_from_cost(dev_c, exact=True).cpu().numpy(), exact=True) == "sorted"
        else:                                                     # the multi-pass kernel: 32-bit costs, always sorted
            assert np.array_equal(np.sort(od), np.arange(m2)), (m2, off)
            c2 = cst[off:]
            sh = 0
            while (int(c2.max()) >> sh) > 4095: sh += 1
            assert (np.diff(np.minimum(c2[od] >> sh, 4095)) <= 0).all(), (m2, off)
    # the renderer with the feedback on: every frame of a moving camera equals the oracle's
    rnd = R.DistributedRenderer(sc, resx, resy, feedback_order=True, order_refresh=2)
    bmin, bmax = osc.nodes[0]["bmin"], osc.nodes[0]["bmax"]
    ctr, ext = (bmin + bmax) * 0.5, (bmax - bmin)
    cams = [cam] * 3 + [FPSCamera((ctr + (rng.random(3) - 0.5) * ext * 0.8).astype(np.float32), rng.random() * 6.28, (rng.random() - 0.5) * 1.5).camera()
                        for _ in range(9)]
    outs = []
    for cm in cams:
        f = rnd.render(cm)
        outs.append((cm, f))
        if len(outs) == rnd.nslots:
            rnd.flush()
            for cm2, f2 in outs:
                compare_frames(f2, osc.render_primary(cm2.as_array13(), resx, resy, mode=O.MODE_IEEE), "renderer feedback")
            outs = []
    rnd.flush()
    assert all(rnd.order_valid)
    # a camera that stands still: each slot re-derives its order ONCE from that camera's own (exact) costs, sorted whatever their shape; then no more refreshes
    for _ in range(4 * rnd.nslots):
        rnd.render(cam)
    rnd.flush()
    torch_mod.cuda.synchronize()
    assert all(rnd.order_exact) and all(a > 0 for a in rnd.order_age)
    for k in range(rnd.nslots):
        assert util.check_derived_order(rnd.slot_cost[k].cpu().numpy(), rnd.order_buf[k].cpu().numpy(), exact=True) == "sorted"
        assert np.array_equal(rnd.slot_cost[k].cpu().numpy(), c), "the slot's costs are this camera's"
    # poison_outputs (bench.py, in front of its timed region): every buffer the renderer has written becomes all-ones and is forgotten; what
    # output_buffers() names afterwards was written after the call
    assert len(rnd.output_buffers()) == rnd.nslots
    old = rnd.output_buffers()
    rnd.poison_outputs()
    assert rnd.output_buffers() == [] and all(bool((f.tri_id == -1).all()) and bool((f.t.view(torch_mod.int32) == -1).all()) for f in old)
    f = rnd.render(cam)
    rnd.flush()
    compare_frames(f, ref, "after the poison")
    assert len(rnd.output_buffers()) == 1
    moved = osc.render_primary(cams[-1].as_array13(), resx, resy, mode=O.MODE_IEEE)
    for _ in range(rnd.nslots):                  # the camera moves again: the orders are predictions, the library's rule
        f = rnd.render(cams[-1])
        rnd.flush()
        compare_frames(f, moved, "renderer feedback, moved again")
    assert not any(rnd.order_exact)
    sc.close()


@pytest.mark.gpu
def test_hit_reciprocal_equals_ieee_division_for_every_float(torch_mod):
    """Inv(det) of Triangle::Collide (src/triangle.cpp:55) is the exact IEEE 1/x in the oracle; the kernels compute it as v_rcp_f32 + one
    Newton step where that is bit-identical and as the full division elsewhere.  Proof by enumeration over all 2^32 inputs."""
    import ctypes
    from snail_amd import _lib
    out = (ctypes.c_uint64 * 2)()
    assert _lib.debug_lib().snail_debug_recip_check(out) == 0      # (the workbench build of the same sources: same recipExact())
    assert out[0] == 0, "%d of 2^32 reciprocals differ from 1.0f / x" % out[0]
    assert out[1] == 2 * 252 * (1 << 23)


@pytest.mark.gpu
@pytest.mark.parametrize("resx,resy", [(96, 96), (200, 120)])
def test_big_leaf_under_a_narrow_range(torch_mod, resx, resy):
    """A hand-made tree, walked by the kernels and by the oracle alike: the SAH tree of the `patches` scene with the subtree of its 100
    coincident triangles collapsed into ONE leaf (the reference's trees reach such leaves only at BVH::maxDepth, i.e. on the deep-tree
    walk).  A shallow tree keeps the packet on the hand-written walk, whose narrow-range leaf forms must hand a leaf of more than 64
    triangles to the chunked wide form."""
    from snail_amd.bvh import HostBVH
    from snail_amd.scene import Scene
    tv, hb, osc = util.scene_pair("patches")
    nodes = hb.nodes.copy()
    sub = nodes["sub"].astype(np.int64)
    is_leaf = (sub & 0x80000000) != 0

    def tris_below(i):
        if is_leaf[i]:
            f = int(sub[i] & 0x7fffffff); return list(range(f, f + int(nodes["aux"][i])))
        c = int(sub[i]); return tris_below(c) + tris_below(c + 1)

    clump = set(np.nonzero((hb.tris["a"][:, 2] == np.float32(-0.25)))[0].tolist())
    assert len(clump) == 100
    # the highest node whose triangles are all clump triangles and contiguous: becomes the leaf
    best = None
    for i in range(len(nodes)):
        t = tris_below(i)
        if set(t) <= clump and len(t) > 64 and sorted(t) == list(range(min(t), min(t) + len(t))):
            if best is None or len(t) > best[1]: best = (i, len(t), min(t))
    assert best is not None, "no contiguous clump subtree of more than 64 triangles"
    i, n, first = best
    nodes["sub"][i] = np.uint32(0x80000000 | first); nodes["aux"][i] = n        # (the now unreachable nodes stay in the array)
    # unreachable nodes are rejected by snail_scene_create? -> compact the array instead
    keep = []
    def reach(k):
        keep.append(k)
        if (int(nodes["sub"][k]) & 0x80000000) == 0:
            c = int(nodes["sub"][k]); reach(c); reach(c + 1)
    reach(0)
    order = sorted(keep)
    # children must stay adjacent: BFS re-layout
    new_nodes = np.zeros(len(order), dtype=nodes.dtype); slot = {0: 0}; nxt = 1; queue = [0]
    while queue:
        k = queue.pop(0)
        new_nodes[slot[k]] = nodes[k]
        if (int(nodes[k]["sub"]) & 0x80000000) == 0:
            c = int(nodes[k]["sub"]); slot[c] = nxt; slot[c + 1] = nxt + 1
            new_nodes[slot[k]]["sub"] = nxt; nxt += 2; queue += [c, c + 1]
    depth = 0
    def dep(k, d):
        nonlocal depth; depth = max(depth, d)
        if (int(new_nodes[k]["sub"]) & 0x80000000) == 0:
            c = int(new_nodes[k]["sub"]); dep(c, d + 1); dep(c + 1, d + 1)
    dep(0, 1)
    assert depth <= 62 and int(new_nodes["aux"][(new_nodes["sub"] & 0x80000000) != 0].max()) == n
    hb2 = HostBVH(hb.tris, new_nodes, depth, hb.perm)
    osc2 = O.OracleScene.__new__(O.OracleScene)
    osc2.tris = np.ascontiguousarray(hb.tris.view(O.TRI_DTYPE)); osc2.nodes = np.ascontiguousarray(new_nodes.view(O.NODE_DTYPE)); osc2.depth = depth; osc2.perm = hb.perm
    sc = Scene(hb2, 0)
    cam = util.camera_for("patches", tv)
    stats = sc.new_stats()
    frame = sc.trace_primary(cam, resx, resy, stats=stats)
    torch_mod.cuda.synchronize()
    ref = osc2.render_primary(cam.as_array13(), resx, resy, mode=O.MODE_IEEE)
    compare_frames(frame, ref, "patches, collapsed clump %dx%d" % (resx, resy))
    assert np.array_equal(stats.cpu().numpy().astype(np.uint64), ref[4]), (stats.cpu().numpy(), ref[4])
    hit_clump = np.isin(ref[3][np.isfinite(ref[0])], np.arange(first, first + n)).sum()
    assert hit_clump > 0
    sc.close()



@pytest.mark.gpu
def test_origin_relative_record_cache_over_many_origins(torch_mod):
    """Shared-origin packets walk node records relative to their origin (camera / light position), kept per scene in an LRU cache of 16
    arrays: 14 cameras x 3 lights each -- more distinct origins than the cache holds, entries recycled while earlier frames are still in
    flight on the stream -- and the first views again at the end; every frame and its counters equal the oracle's."""
    from snail_amd import FPSCamera
    name = "atrium:0.02"
    tv, sc, osc = gpu_scene(name)
    bmin, bmax = osc.nodes[0]["bmin"], osc.nodes[0]["bmax"]
    c, e = (bmin + bmax) * 0.5, (bmax - bmin)
    rng = np.random.RandomState(11)
    views = []
    for k in range(14):
        pos = (c + (rng.rand(3) - 0.5) * e * 0.8).astype(np.float32)
        cam = FPSCamera(pos, float(rng.rand() * 6.28), float((rng.rand() - 0.5) * 0.8)).camera()
        lights = np.zeros((3, 7), dtype=np.float32)
        for n in range(3):
            lights[n, :3] = c + (rng.rand(3) - 0.5) * e * 1.1
            lights[n, 3:6] = rng.rand(3); lights[n, 6] = float(e.max()) * float(np.exp(rng.uniform(-1.5, 0.8)))
        views.append((cam, lights))
    views += views[:2]
    frames = []
    for cam, lights in views:                      # enqueue everything first: cache entries are recycled under frames in flight
        st = sc.new_stats()
        frames.append((sc.render_whitted(cam, 200, 120, lights, stats=st, reflections=False), st))
    torch_mod.cuda.synchronize()
    for (cam, lights), (img, st) in zip(views, frames):
        want, wst = osc.render_whitted(cam.as_array13(), 200, 120, lights, mode=O.MODE_IEEE, reflections=False)
        assert np.array_equal(img.cpu().numpy(), want)
        assert np.array_equal(st.cpu().numpy().astype(np.uint64), wst)
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["stress:0.05", "atrium:0.05"])
def test_tiny_masked_per_ray_origin_packets(torch_mod, name):
    """Packets of one to three quads with lane masks and per-ray origins (what a mirrored bounce leaves of a packet that mostly missed):
    400 seeded batches through the generic entry point, hit records, barycentrics and counters equal the oracle's -- the packets a work-in-progress
    version of the coherent per-ray loop got wrong in round 3 (planes chosen by lane 0's signs instead of the packet's octant: profiles/r3_final_soak.txt)."""
    from snail_amd.scene import Context
    tv, sc, osc = gpu_scene(name)
    cam = util.camera_for(name, tv)
    rng = np.random.RandomState(5)
    tt = torch_mod.from_numpy
    for b in range(400):
        size, npk = int(rng.randint(1, 4)), int(rng.randint(1, 40))
        origin, dirs, idir, mask, dist, obj, bary = util.secondary_packets(osc, cam, 640, 368, npk, seed=int(rng.randint(1 << 30)), shared=False, masked=True,
                                                                           size=size, poison=False)
        d2, o2, b2 = dist.copy(), obj.copy(), bary.copy()
        ost = osc.trace_rays(origin, dirs, idir, mask, d2, o2, b2, npk, size, False, mode=O.MODE_IEEE)
        ctx = Context(tt(origin).cuda(), tt(dirs).cuda(), tt(idir).cuda(), tt(dist.copy()).cuda(), tt(obj.copy()).cuda(), tt(bary.copy()).cuda(),
                      size=size, shared_origin=False, mask=tt(mask).cuda())
        st = sc.new_stats(); sc.traverse_primary(ctx, stats=st); torch_mod.cuda.synchronize()
        s = st.cpu().numpy().astype(np.uint64)
        assert np.array_equal(ctx.object.cpu().numpy(), o2), (b, size, npk)
        assert np.array_equal(ctx.distance.cpu().numpy().view(np.uint32), d2.view(np.uint32)), (b, size, npk)
        assert np.array_equal(ctx.barycentric.cpu().numpy().view(np.uint32), b2.view(np.uint32)), (b, size, npk)
        assert s[0] == ost[0] and s[1] == ost[1], (b, size, npk, s, ost)
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,resx,resy,nl,refl", [("atrium:0.05", 640, 368, 1, False), ("atrium:0.05", 640, 368, 1, True), ("atrium:0.05", 328, 200, 2, True),
                                                     ("stress:0.05", 250, 130, 1, True), ("box", 64, 64, 1, True)])
def test_staged_pipeline_dispatch_orders_change_nothing_but_the_order(torch_mod, name, resx, resy, nl, refl):
    """snail_render_whitted_ordered_dev: every walking stage of the staged pipeline (primary packets, their shadow packets, the mirrored
    packets, their shadow packets) takes a dispatch order and returns its packets' node visits.  The frame and the counters are those of
    the plain call -- and the oracle's -- under the fed-back orders, reversed orders and random ones; the costs add up to the counters."""
    tv, sc, osc = gpu_scene(name)
    cam = util.camera_for(name, tv)
    bmin, bmax = osc.nodes[0]["bmin"], osc.nodes[0]["bmax"]
    c, e = (bmin + bmax) * 0.5, (bmax - bmin)
    lights = np.array([[c[0], c[1] + 0.35 * e[1], c[2], 1.0, 0.9, 0.8, 2.0 * float(e.max())],
                       [c[0] - 0.3 * e[0], c[1] + 0.1 * e[1], c[2] + 0.2 * e[2], 0.3, 0.5, 1.0, 0.6 * float(e.max())]], dtype=np.float32)[:nl]
    want, wst = osc.render_whitted(cam.as_array13(), resx, resy, lights, mode=O.MODE_IEEE, reflections=refl)
    n = sc.primary_slots(resx, resy)
    S = sc.WHITTED_STAGES
    cost = torch_mod.full((S, n), -7, dtype=torch_mod.int32, device="cuda")
    st0 = sc.new_stats()
    got = sc.render_whitted(cam, resx, resy, lights, stats=st0, reflections=refl, slot_cost=cost).cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(st0.cpu().numpy().astype(np.uint64), wst)
    cst = cost.cpu().numpy()
    stages = range(S) if refl else range(2)
    for k in stages:
        assert (cst[k] >= 0).all(), k                               # every slot of a stage that ran was written
    if nl == 1:                                                      # one light: the stages' node visits are ALL the frame's node visits
        assert int(cst[list(stages)].astype(np.int64).sum()) == int(wst[1]), (cst[list(stages)].sum(axis=1), wst)
    rng = np.random.default_rng(3)
    fed = torch_mod.empty((S, n), dtype=torch_mod.int32, device="cuda")
    for k in range(S):
        sc.order_from_cost(cost[k] if k in stages else torch_mod.zeros(n, dtype=torch_mod.int32, device="cuda"), fed[k])
    rev = torch_mod.flip(fed, dims=[1]).contiguous()
    rnd = torch_mod.from_numpy(np.stack([rng.permutation(n) for _ in range(S)]).astype(np.int32)).cuda()
    for what, order in (("fed back", fed), ("reversed", rev), ("random", rnd)):
        st = sc.new_stats()
        c2 = torch_mod.zeros((S, n), dtype=torch_mod.int32, device="cuda")
        g = sc.render_whitted(cam, resx, resy, lights, stats=st, reflections=refl, order=order, slot_cost=c2).cpu().numpy()
        assert np.array_equal(g, want), (what, int((g != want).sum()))
        assert np.array_equal(st.cpu().numpy().astype(np.uint64), wst), (what, st.cpu().numpy(), wst)
        for k in stages:
            assert np.array_equal(c2[k].cpu().numpy(), cst[k]), (what, k)        # a packet's cost does not depend on when it ran
    # the next orders of every stage derived inside the launch, in place (snail_render_whitted_reorder_dev): same frame, same costs, each stage's buffer a
    # permutation whose cost classes descend
    buf = rev.clone()
    c3 = torch_mod.zeros((S, n), dtype=torch_mod.int32, device="cuda")
    st = sc.new_stats()
    g = sc.render_whitted(cam, resx, resy, lights, stats=st, reflections=refl, order=buf, slot_cost=c3, next_order=buf).cpu().numpy()
    assert np.array_equal(g, want) and np.array_equal(st.cpu().numpy().astype(np.uint64), wst)
    ob = buf.cpu().numpy()
    for k in stages:
        assert np.array_equal(c3[k].cpu().numpy(), cst[k]), k
        assert util.check_derived_order(cst[k], ob[k]) == util.check_derived_order(cst[k], fed[k].cpu().numpy()), k      # (the stand-alone sort decides the same)
    g = sc.render_whitted(cam, resx, resy, lights, reflections=refl, order=buf, slot_cost=c3, next_order=buf, order_exact=True).cpu().numpy()   # costs declared exact
    assert np.array_equal(g, want)
    ob = buf.cpu().numpy()
    for k in stages:
        assert util.check_derived_order(cst[k], ob[k], exact=True) == "sorted", k
    # the renderer with the feedback on (bench.py --config 3): frames of a moving camera equal the oracle's
    from snail_amd import render as R
    r = R.DistributedRenderer(sc, resx, resy, lights7=lights, reflections=refl, feedback_order=True, order_refresh=2)
    assert r.feedback and r.whitted_single
    cams = [cam] * 5 + [FPSCamera(np.asarray(cam.pos) + np.float32(0.05 * i) * np.asarray(cam.front), *((scenes.atrium_camera() if name.startswith("atrium") else (None, 0.3, 0.1))[1:])).camera()
                        for i in range(1, 8)]
    for i, cm in enumerate(cams):
        f = r.render(cm)
        r.flush()
        w2, _ = osc.render_whitted(cm.as_array13(), resx, resy, lights, mode=O.MODE_IEEE, reflections=refl)
        assert np.array_equal(f.cpu().numpy(), w2), i
    assert all(r.order_valid)
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("config,arith", [("1", "ieee"), ("5", "ieee"), ("4", "ieee"), ("3", "ieee"), ("3r", "ieee"), ("1", "host_sse"), ("3r", "host_sse")])
def test_timed_path_at_its_own_size_against_committed_digests(torch_mod, config, arith):
    """What bench.py times -- two frames per launch, four launches in flight, fed-back dispatch orders (config 3: the staged pipeline with
    its per-stage orders) -- at the bench's own sizes, checked the way bench.py checks itself: every output buffer holds the same frame,
    and its SHA-256 is the committed digest of the ORACLE's frame (tests/golden/oracle_full_size.json; host_sse: the section of this
    box's CPU, skipped on a CPU the file does not know)."""
    import hashlib
    import json
    from snail_amd import HostBVH
    from snail_amd import render as R
    from snail_amd.scene import Scene
    from tests.golden import full_size as FS
    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_full_size.json")))
    name, resx, resy, nl, refl = FS.WORKLOADS[config]
    sec = gold["ieee"] if arith == "ieee" else gold.get("host_sse", {}).get(FS.host_table_key())
    if sec is None:
        pytest.skip("no committed host_sse digests for this CPU (tests/golden/full_size.py host_sse)")
    want = sec["%s_%dx%d_c%s" % (name, resx, resy, config)]
    tv, hb, _ = util.scene_pair(name)
    sc = Scene(hb, 0)
    sc.set_arith(arith)
    cam = FS.bench_camera(name)
    lights = FS.bench_light(*hb.bbox()) if nl else None
    rnd = R.DistributedRenderer(sc, resx, resy, lights7=lights, reflections=refl, feedback_order=True, frames_per_launch=2)
    st = sc.new_stats()
    rnd.render(cam, stats=st)
    rnd.flush()
    rnd2 = R.DistributedRenderer(sc, resx, resy, lights7=lights, reflections=refl, feedback_order=True, frames_per_launch=2)
    for _ in range(3 * rnd2.nslots * rnd2.batch):        # every slot: a frame in built-in order, then frames under the order derived from it
        rnd2.render(cam)
    rnd2.flush()
    torch_mod.cuda.synchronize()
    sha = lambda t: hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()
    bufs = rnd2.output_buffers()
    assert len(bufs) == rnd2.nslots * rnd2.batch
    for b in bufs:
        if nl:
            assert sha(b) == want["sha_bgr"]
        else:
            assert (sha(b.t), sha(b.u), sha(b.v), sha(b.tri_id)) == (want["sha_t"], want["sha_u"], want["sha_v"], want["sha_id"])
    got = [int(x) for x in st.cpu().numpy()]
    assert got == want["stats"], (got, want["stats"])
    sc.close()
