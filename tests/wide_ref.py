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
"""
import numpy as np

F = np.float32
INF = F(np.inf)
MUTATIONS = ("right_first", "fminf", "stored_plane", "t_positive")


def sel_min(a, b):
    return np.where(a < b, a, b)


def sel_max(a, b):
    return np.where(a > b, a, b)


def wide_test(bmin, bmax, o, idir, dist):
    """BBox::WideTest (src/bounding_box.cpp:258-326) for rows of rays against rows of boxes -> bool."""
    l1 = idir[:, 0] * (bmin[:, 0] - o[:, 0]); l2 = idir[:, 0] * (bmax[:, 0] - o[:, 0])
    lmin = sel_min(l1, l2); lmax = sel_max(l1, l2)
    for k in (1, 2):
        l1 = idir[:, k] * (bmin[:, k] - o[:, k]); l2 = idir[:, k] * (bmax[:, k] - o[:, k])
        lmin = sel_max(sel_min(l1, l2), lmin); lmax = sel_min(sel_max(l1, l2), lmax)
    return (lmax >= F(0.0)) & (lmin <= sel_min(lmax, dist))


def _cross(b, c):
    return np.stack([b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1], b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2], b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]], axis=1)


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]     # summed left to right


def collide0(tri, o, d, mutation=None):
    """Triangle::Collide<0> (src/triangle.h:139-164) for rows of TRI_DTYPE records against rows of rays -> distance or +inf.
    The locals `ba`, `ca` of the reference hide the members from line 146 on: the normal AND the cross products of u, v take the recomputed
    edges (ba + a) - a, (ca + a) - a."""
    a = tri["a"]
    ba = (tri["ba"] + a) - a
    ca = (tri["ca"] + a) - a
    if mutation == "stored_plane":
        nrm = np.ascontiguousarray(tri["plane"][:, :3])
        t0 = tri["t0"]
    else:
        nrm = _cross(ba, ca)
        t0 = np.sqrt(_dot(nrm, nrm))
        nrm = nrm * (F(1.0) / t0)[:, None]
    det = _dot(d, nrm)
    tvec = o - a
    u = _dot(d, _cross(ba, tvec))
    v = _dot(d, _cross(tvec, ca))
    test = (sel_min(u, v) >= F(0.0)) & (u + v <= det * t0)
    dist = -_dot(tvec, nrm) / det
    if mutation == "t_positive":
        test = test & (dist > F(0.0))
    return np.where(test, dist, INF).astype(F)


def wide_trace(nodes, tris, origin, dir, dist, idir=None, indices=None, start_node=0, mutation=None):
    """-> (dist float32 [nRays], visits int32 [nRays, 2] = per ray {box tests, triangle tests}).  nodes / tris = NODE_DTYPE / TRI_DTYPE
    arrays; rays not listed in `indices` keep their dist and have zero visits."""
    assert mutation is None or mutation in MUTATIONS
    origin = np.ascontiguousarray(origin, dtype=F).reshape(-1, 3)
    dir = np.ascontiguousarray(dir, dtype=F).reshape(-1, 3)
    out = np.array(dist, dtype=F).reshape(-1).copy()
    n_rays = len(out)
    visits = np.zeros((n_rays, 2), dtype=np.int32)
    rays = np.arange(n_rays) if indices is None else np.asarray(indices, dtype=np.int64)
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
                    ok[t] = wide_test(nd["bmin"][t], nd["bmax"][t], o[r[t]], inv[r[t]], dd[r[t]])
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
                first, second = (c + 1, c) if mutation == "right_first" else (c, c + 1)
                stack[sp[ri], ri] = second
                sp[ri] += 1
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
    return out, visits


def photon_colour(rgb):
    """Photon::Photon (src/photons.h:11-13): u8(Clamp(c * 255, 0, 255)), Clamp = Min(Max(x, 0), 255) in the select forms -> uint8[4], [3] = 0."""
    with np.errstate(all="ignore"):
        x = np.asarray(rgb, dtype=F) * F(255.0)
        x = sel_max(x, F(0.0))
        x = sel_min(x, F(255.0))
    return np.array([int(x[0]), int(x[1]), int(x[2]), 0], dtype=np.uint8)


def photons(origin, dir, dist, lights7, count, dtype):
    """TracePhotons:242-249 from traced distances: the records of the rays whose distance is not +inf, in ray order."""
    origin = np.ascontiguousarray(origin, dtype=F).reshape(-1, 3)
    dir = np.ascontiguousarray(dir, dtype=F).reshape(-1, 3)
    dist = np.asarray(dist, dtype=F)
    keep = np.flatnonzero(~(dist == INF))
    out = np.zeros(len(keep), dtype=dtype)
    with np.errstate(all="ignore"):
        out["position"] = origin[keep] + dir[keep] * dist[keep][:, None]
    out["direction"] = dir[keep]
    l7 = np.asarray(lights7, dtype=F).reshape(-1, 7)
    cols = np.stack([photon_colour(l[3:6]) for l in l7]) if len(l7) else np.zeros((0, 4), dtype=np.uint8)
    out["color"] = cols[keep // max(int(count), 1)]
    out["temp"] = 1
    return out
