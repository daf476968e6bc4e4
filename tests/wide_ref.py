"""BVH::WideTrace (src/bvh/traverse.cpp:197-225) restated in NumPy float32, per ray, with counters -- what include/snail_wide.h states.

The reference's index lists only batch rays; for ONE ray the recursion is fixed, so every ray here carries its own state (node, the right
siblings still to be tested, the triangle it is at) and the rays advance side by side, one box test or one triangle test per step.  Every
operation is a separately rounded float32 NumPy operation; Min / Max are the selects a < b ? a : b and a > b ? a : b (second operand on
NaN and +-0), division and square root are correctly rounded.

MUTATIONS (tests/test_wide_host.py shows that the cases tell each of them from the walk):
  "right_first"   the right child's box and subtree before the left's
  "fminf"         fmin in place of the select in the leaf (a NaN distance is dropped instead of kept)
  "stored_plane"  the triangle's stored plane normal and t0 in place of the recomputed ones
  "t_positive"    a t > 0 filter on the hit

EDGE_MUTATIONS (tests/test_wide_edges_host.py shows that the cases of tests/wide_edge_cases.py tell each of them from the walk):
  "flush_denormals"  every operand read and every product, sum, difference, quotient and square root of wide_test and collide0 with
                     |x| < 2^-126 becomes a zero of the same sign (a build that flushes fp32 denormals)
  "stack_short"      a ray that would push with slots - 1 entries already stacked ends instead (the kernel's sp < A.slots off by one)
photons() has mutations of its own: "keep_less" keeps dist < inf, "keep_finite" keeps isfinite(dist), in place of !(dist == inf).
"""
import numpy as np

F = np.float32
INF = F(np.inf)
MUTATIONS = ("right_first", "fminf", "stored_plane", "t_positive")
EDGE_MUTATIONS = ("flush_denormals", "stack_short")
PHOTON_MUTATIONS = ("keep_less", "keep_finite")
TINY = F(2.0 ** -126)       # the smallest normal float32


def _same(x):
    return x


def flush(x):
    """|x| < 2^-126 -> a zero of the same sign (NaN stays)"""
    x = np.asarray(x, dtype=F)
    return np.where(np.abs(x) < TINY, np.copysign(F(0.0), x), x).astype(F)


def sel_min(a, b):
    return np.where(a < b, a, b)


def sel_max(a, b):
    return np.where(a > b, a, b)


def wide_test(bmin, bmax, o, idir, dist, fz=_same):
    """BBox::WideTest (src/bounding_box.cpp:258-326) for rows of rays against rows of boxes -> bool.  fz = what every operand and every
    result goes through (the identity; `flush` under "flush_denormals")."""
    bmin, bmax, o, idir, dist = fz(bmin), fz(bmax), fz(o), fz(idir), fz(dist)
    l1 = fz(idir[:, 0] * fz(bmin[:, 0] - o[:, 0])); l2 = fz(idir[:, 0] * fz(bmax[:, 0] - o[:, 0]))
    lmin = sel_min(l1, l2); lmax = sel_max(l1, l2)
    for k in (1, 2):
        l1 = fz(idir[:, k] * fz(bmin[:, k] - o[:, k])); l2 = fz(idir[:, k] * fz(bmax[:, k] - o[:, k]))
        lmin = sel_max(sel_min(l1, l2), lmin); lmax = sel_min(sel_max(l1, l2), lmax)
    return (lmax >= F(0.0)) & (lmin <= sel_min(lmax, dist))


def _cross(b, c, fz=_same):
    return np.stack([fz(fz(b[:, 1] * c[:, 2]) - fz(b[:, 2] * c[:, 1])), fz(fz(b[:, 2] * c[:, 0]) - fz(b[:, 0] * c[:, 2])),
                     fz(fz(b[:, 0] * c[:, 1]) - fz(b[:, 1] * c[:, 0]))], axis=1)


def _dot(a, b, fz=_same):
    return fz(fz(fz(a[:, 0] * b[:, 0]) + fz(a[:, 1] * b[:, 1])) + fz(a[:, 2] * b[:, 2]))     # summed left to right


def collide0(tri, o, d, mutation=None):
    """Triangle::Collide<0> (src/triangle.h:139-164) for rows of TRI_DTYPE records against rows of rays -> distance or +inf.
    The locals `ba`, `ca` of the reference hide the members from line 146 on: the normal AND the cross products of u, v take the recomputed
    edges (ba + a) - a, (ca + a) - a."""
    fz = flush if mutation == "flush_denormals" else _same
    a, o, d = fz(tri["a"]), fz(o), fz(d)
    ba = fz(fz(fz(tri["ba"]) + a) - a)
    ca = fz(fz(fz(tri["ca"]) + a) - a)
    if mutation == "stored_plane":
        nrm = np.ascontiguousarray(tri["plane"][:, :3])
        t0 = tri["t0"]
    else:
        nrm = _cross(ba, ca, fz)
        t0 = fz(np.sqrt(_dot(nrm, nrm, fz)))
        nrm = fz(nrm * fz(F(1.0) / t0)[:, None])
    det = _dot(d, nrm, fz)
    tvec = fz(o - a)
    u = _dot(d, _cross(ba, tvec, fz), fz)
    v = _dot(d, _cross(tvec, ca, fz), fz)
    test = (sel_min(u, v) >= F(0.0)) & (fz(u + v) <= fz(det * t0))
    dist = fz(-_dot(tvec, nrm, fz) / det)
    if mutation == "t_positive":
        test = test & (dist > F(0.0))
    return np.where(test, dist, INF).astype(F)


def wide_trace(nodes, tris, origin, dir, dist, idir=None, indices=None, start_node=0, mutation=None, slots=None, diag=None):
    """-> (dist float32 [nRays], visits int32 [nRays, 2] = per ray {box tests, triangle tests}).  nodes / tris = NODE_DTYPE / TRI_DTYPE
    arrays; rays not listed in `indices` keep their dist and have zero visits.  slots = the stack entries a ray has (None: as many as it
    needs): a ray that would push onto a full stack ends where it is, as the kernel's does.  diag (a dict) receives "max_sp" = per ray the
    largest number of entries it had stacked."""
    assert mutation is None or mutation in MUTATIONS + EDGE_MUTATIONS
    fz = flush if mutation == "flush_denormals" else _same
    room = None if slots is None else int(slots) - (1 if mutation == "stack_short" else 0)
    origin = np.ascontiguousarray(origin, dtype=F).reshape(-1, 3)
    dir = np.ascontiguousarray(dir, dtype=F).reshape(-1, 3)
    out = np.array(dist, dtype=F).reshape(-1).copy()
    n_rays = len(out)
    visits = np.zeros((n_rays, 2), dtype=np.int32)
    rays = np.arange(n_rays) if indices is None else np.asarray(indices, dtype=np.int64)
    if diag is not None:
        diag["max_sp"] = np.zeros(n_rays, dtype=np.int64)
    if len(rays) == 0:
        return out, visits
    with np.errstate(all="ignore"):
        o, d = origin[rays], dir[rays]
        inv = (F(1.0) / d).astype(F) if idir is None else np.ascontiguousarray(idir, dtype=F).reshape(-1, 3)[rays]
        dd = out[rays].copy()
        m = len(rays)
        nbox, ntri = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
        nxt = np.full(m, int(start_node), dtype=np.int64)
        tested = np.zeros(m, dtype=bool)          # the start node's own box is not tested
        stack = np.zeros((66, m), dtype=np.int64)
        sp = np.zeros(m, dtype=np.int64)
        max_sp = np.zeros(m, dtype=np.int64)
        in_leaf = np.zeros(m, dtype=bool)
        t_at, t_end = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
        alive = np.ones(m, dtype=bool)
        while alive.any():
            pop = np.zeros(m, dtype=bool)
            # --- rays at a node ---
            r = np.flatnonzero(alive & ~in_leaf)
            if len(r):
                nd = nodes[nxt[r]]
                ok = np.ones(len(r), dtype=bool)
                t = tested[r]
                if t.any():
                    ok[t] = wide_test(nd["bmin"][t], nd["bmax"][t], o[r[t]], inv[r[t]], dd[r[t]], fz)
                    nbox[r[t]] += 1
                tested[r] = True
                sub = nd["sub"].astype(np.int64)
                leaf = (sub & 0x80000000) != 0
                pop[r[~ok]] = True
                rl = r[ok & leaf]
                in_leaf[rl] = True
                t_at[rl] = sub[ok & leaf] & 0x7fffffff
                t_end[rl] = t_at[rl] + nd["aux"][ok & leaf].astype(np.int64)
                ri = r[ok & ~leaf]
                c = sub[ok & ~leaf]
                if room is not None:              # a full stack: the ray ends here, whatever it still had stacked
                    full = sp[ri] >= room
                    alive[ri[full]] = False
                    ri, c = ri[~full], c[~full]
                first, second = (c + 1, c) if mutation == "right_first" else (c, c + 1)
                stack[sp[ri], ri] = second
                sp[ri] += 1
                max_sp[ri] = np.maximum(max_sp[ri], sp[ri])
                nxt[ri] = first
            # --- rays in a leaf: one triangle each ---
            empty = np.flatnonzero(alive & in_leaf & (t_at >= t_end))
            in_leaf[empty] = False
            pop[empty] = True
            r = np.flatnonzero(alive & in_leaf)
            if len(r):
                hit = collide0(tris[t_at[r]], o[r], d[r], mutation)
                dd[r] = np.fmin(dd[r], hit) if mutation == "fminf" else np.where(dd[r] < hit, dd[r], hit)
                ntri[r] += 1
                t_at[r] += 1
            # --- the next right sibling, or the end ---
            r = np.flatnonzero(pop)
            end = r[sp[r] == 0]
            alive[end] = False
            r = r[sp[r] > 0]
            sp[r] -= 1
            nxt[r] = stack[sp[r], r]
        out[rays] = dd
        visits[rays, 0] = nbox
        visits[rays, 1] = ntri
        if diag is not None:
            diag["max_sp"][rays] = max_sp
    return out, visits


def photon_colour(rgb):
    """Photon::Photon (src/photons.h:11-13): u8(Clamp(c * 255, 0, 255)), Clamp = Min(Max(x, 0), 255) in the select forms -> uint8[4], [3] = 0."""
    with np.errstate(all="ignore"):
        x = np.asarray(rgb, dtype=F) * F(255.0)
        x = sel_max(x, F(0.0))
        x = sel_min(x, F(255.0))
    return np.array([int(x[0]), int(x[1]), int(x[2]), 0], dtype=np.uint8)


def photons(origin, dir, dist, lights7, count, dtype, mutation=None):
    """TracePhotons:242-249 from traced distances: the records of the rays whose distance is not +inf, in ray order (NaN, -inf and
    negative distances leave one).  mutation: "keep_less" keeps dist < inf, "keep_finite" keeps isfinite(dist)."""
    assert mutation is None or mutation in PHOTON_MUTATIONS
    origin = np.ascontiguousarray(origin, dtype=F).reshape(-1, 3)
    dir = np.ascontiguousarray(dir, dtype=F).reshape(-1, 3)
    dist = np.asarray(dist, dtype=F)
    with np.errstate(all="ignore"):
        keep = np.flatnonzero(dist < INF if mutation == "keep_less" else np.isfinite(dist) if mutation == "keep_finite" else ~(dist == INF))
    out = np.zeros(len(keep), dtype=dtype)
    with np.errstate(all="ignore"):
        out["position"] = origin[keep] + dir[keep] * dist[keep][:, None]
    out["direction"] = dir[keep]
    l7 = np.asarray(lights7, dtype=F).reshape(-1, 7)
    cols = np.stack([photon_colour(l[3:6]) for l in l7]) if len(l7) else np.zeros((0, 4), dtype=np.uint8)
    out["color"] = cols[keep // max(int(count), 1)]
    out["temp"] = 1
    return out
