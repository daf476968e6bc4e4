"""An independent numpy restatement of the reference's fast builder, BVH::Construct(scene, fastBuild) + BVH::FindSplit
(src/bvh/tree.cpp:161-287, :293-314), written from the reference and not from snail_amd/csrc/bvh_build.cpp: recursion as the reference has
it, an index list partitioned and then gathered, TestTris evaluated from P1 / P2 / P3.  Every operation is a float32 numpy operation, one
rounding each.  The one deviation of include/snail_bvh_fast.h is restated too: a bin index that is NaN or < 0 is 0, one >= 16 is 15.

Also here: the closed form of the order libstdc++'s std::partition leaves (partition_order), checked against the literal loop
(partition_loop) by tests/test_bvh_fast_host.py -- the device builder relies on it."""
from __future__ import annotations

import sys

import numpy as np

F = np.float32
N_BINS = 16
EPSILON = F(0.0001)      # constant::epsilon, veclib/vecbase.h:40
NODE_DTYPE = np.dtype([("bmin", "<f4", 3), ("bmax", "<f4", 3), ("sub", "<u4"), ("aux", "<i4")])


def tri_corners(tris):
    """P1, P2, P3 (src/triangle.h:35-37): a, ba + a, ca + a."""
    with np.errstate(all="ignore"):
        return tris["a"], tris["ba"] + tris["a"], tris["ca"] + tris["a"]


def vmin(a, b):
    """Min(a, b) = a < b ? a : b (veclib/vecbase.h:75-76): the SECOND operand on a tie (and on NaN)."""
    return np.where(a < b, a, b)


def vmax(a, b):
    return np.where(a > b, a, b)


def tri_boxes(tris):
    """Triangle::GetBBox (src/triangle.h:62-70): VMin(P1, VMin(P2, P3)), VMax(P1, VMax(P2, P3))."""
    p1, p2, p3 = tri_corners(tris)
    return vmin(p1, vmin(p2, p3)), vmax(p1, vmax(p2, p3))


def fold_min(acc, xs):
    """acc = Min(acc, x) over the rows of xs in order -- by its closed form: the LAST row among the numerically smallest (which replaces
    acc unless acc is strictly smaller).  No NaN in xs."""
    if len(xs) == 0:
        return acc
    m = xs.min(axis=0)
    last = len(xs) - 1 - np.argmax((xs == m)[::-1], axis=0)
    best = xs[last, np.arange(xs.shape[1])]
    return np.where(acc < best, acc, best)


def fold_max(acc, xs):
    if len(xs) == 0:
        return acc
    m = xs.max(axis=0)
    last = len(xs) - 1 - np.argmax((xs == m)[::-1], axis=0)
    best = xs[last, np.arange(xs.shape[1])]
    return np.where(acc > best, acc, best)


def fold_min_loop(acc, xs):
    """fold_min, literally (tests compare the two)."""
    for x in xs:
        acc = vmin(acc, x)
    return acc


def box_sa(lo, hi):
    """BoxSA (src/bvh/tree.cpp:45-47): (Width * (Depth + Height) + Depth * Height) * 2, Width = x, Height = y, Depth = z."""
    with np.errstate(all="ignore"):
        w, h, d = F(hi[0] - lo[0]), F(hi[1] - lo[1]), F(hi[2] - lo[2])
        return F(F(F(w * F(d + h)) + F(d * h)) * F(2.0))


def bin_index(c, sub, mul):
    with np.errstate(all="ignore"):
        v = (c - sub).astype(F) * mul
    out = np.zeros(v.shape, dtype=np.int64)
    ok = v >= 0
    big = ok & ~(v < F(N_BINS))
    mid = ok & ~big
    out[mid] = v[mid].astype(np.int64)      # int(float): truncation
    out[big] = N_BINS - 1
    return out


def partition_loop(pred):
    """libstdc++'s __partition for bidirectional iterators (bits/stl_algo.h) over the positions 0..n-1; pred = bool per position.
    -> the order it leaves: out[k] = the position whose element ends at k."""
    order = list(range(len(pred)))
    lo, hi = 0, len(pred)
    while True:
        while True:
            if lo == hi:
                return np.array(order, dtype=np.int64)
            if pred[order[lo]]:
                lo += 1
            else:
                break
        hi -= 1
        while True:
            if lo == hi:
                return np.array(order, dtype=np.int64)
            if not pred[order[hi]]:
                hi -= 1
            else:
                break
        order[lo], order[hi] = order[hi], order[lo]
        lo += 1


def partition_order(pred):
    """The same order in closed form: with L = number of true elements, the k-th (ascending) false element before L swaps with the k-th
    (descending) true element from L on; everything else stays."""
    pred = np.asarray(pred, dtype=bool)
    n, L = len(pred), int(pred.sum())
    order = np.arange(n, dtype=np.int64)
    a = np.nonzero(~pred[:L])[0]
    b = L + np.nonzero(pred[L:])[0][::-1]
    order[a], order[b] = b, a
    return order


class FastTree:
    pass


def build_fast(tris_in):
    """-> FastTree with nodes (NODE_DTYPE), tris (permuted copy), perm (slot -> input), depth."""
    tris = np.array(tris_in, copy=True)
    n = len(tris)
    perm = np.arange(n, dtype=np.int32)
    nodes = []   # [lo(3), hi(3), sub, aux]
    out = FastTree()
    out.depth = 0
    blo, bhi = tri_boxes(tris)
    nodes.append([fold_min(blo[0], blo[1:]), fold_max(bhi[0], bhi[1:]), 0, 0])
    inf = F(np.inf)

    def find_split(n_node, first, count, sdepth):
        lo, hi = nodes[n_node][0], nodes[n_node][1]
        if count <= 4:
            out.depth = max(out.depth, sdepth)
            nodes[n_node][2], nodes[n_node][3] = first | 0x80000000, count
            return
        sl = slice(first, first + count)
        with np.errstate(all="ignore"):
            size = (hi - lo).astype(F)
            axis = (2 if size[2] > size[1] else 1) if size[1] > size[0] else (2 if size[2] > size[0] else 0)
            mul = F(F(F(N_BINS) * F(F(1.0) - EPSILON)) / F(hi[axis] - lo[axis]))
            sub = lo[axis]
            tlo, thi = tri_boxes(tris[sl])
            c = ((thi[:, axis] + tlo[:, axis]).astype(F) * F(0.5)).astype(F)
        bins = bin_index(c, sub, mul)
        bin_lo = np.full((N_BINS, 3), inf, dtype=F)
        bin_hi = np.full((N_BINS, 3), -inf, dtype=F)
        bin_cnt = np.zeros(N_BINS, dtype=np.int64)
        for b in range(N_BINS):
            m = bins == b
            bin_cnt[b] = int(m.sum())
            bin_lo[b] = fold_min(bin_lo[b], tlo[m])
            bin_hi[b] = fold_max(bin_hi[b], thi[m])
        l_lo, l_hi, r_lo, r_hi = bin_lo.copy(), bin_hi.copy(), bin_lo.copy(), bin_hi.copy()
        l_cnt, r_cnt = bin_cnt.copy(), bin_cnt.copy()
        for b in range(1, N_BINS):
            l_lo[b], l_hi[b] = vmin(l_lo[b - 1], bin_lo[b]), vmax(l_hi[b - 1], bin_hi[b])
            l_cnt[b] = l_cnt[b - 1] + bin_cnt[b]
        for b in range(N_BINS - 2, -1, -1):
            r_lo[b], r_hi[b] = vmin(r_lo[b + 1], bin_lo[b]), vmax(r_hi[b + 1], bin_hi[b])
            r_cnt[b] = r_cnt[b + 1] + bin_cnt[b]
        min_cost = inf
        with np.errstate(all="ignore"):
            no_split = F(F(F(1.0) * F(count)) * box_sa(lo, hi))
            min_idx = 1
            for b in range(1, N_BINS):
                cl = F(box_sa(l_lo[b - 1], l_hi[b - 1]) * F(l_cnt[b - 1])) if l_cnt[b - 1] else F(0)
                cr = F(box_sa(r_lo[b], r_hi[b]) * F(r_cnt[b])) if r_cnt[b] else F(0)
                cost = F(cl + cr)
                if cost < min_cost:
                    min_cost, min_idx = cost, b
            min_cost = F(F(0.0) + F(F(1.0) * min_cost))
        if no_split < min_cost:
            out.depth = max(out.depth, sdepth)
            nodes[n_node][2], nodes[n_node][3] = first | 0x80000000, count
            return
        # TestTris (tree.cpp:24-43): centre from Min / Max of the corners' coordinates on the axis
        p1, p2, p3 = tri_corners(tris[sl])
        f1, f2, f3 = p1[:, axis], p2[:, axis], p3[:, axis]
        with np.errstate(all="ignore"):
            centre = ((vmin(f1, vmin(f2, f3)) + vmax(f1, vmax(f2, f3))).astype(F) * F(0.5)).astype(F)
        order = partition_loop(bin_index(centre, sub, mul) < min_idx)
        tris[sl] = tris[sl][order]
        perm[sl] = perm[sl][order]
        left = [l_lo[min_idx - 1], l_hi[min_idx - 1]]
        right = [r_lo[min_idx], r_hi[min_idx]]
        left_count, right_count = int(l_cnt[min_idx - 1]), int(r_cnt[min_idx])
        if left_count == 0 or right_count == 0:
            mid = count // 2
            tlo, thi = tri_boxes(tris[sl])
            left = [fold_min(tlo[0], tlo[1:mid]), fold_max(thi[0], thi[1:mid])]
            right = [fold_min(tlo[count - 1], tlo[mid:]), fold_max(thi[count - 1], thi[mid:])]
            left_count, right_count = mid, count - mid
        sub_node = len(nodes)
        first_node = (0 if left[1][axis] < right[1][axis] else 1) if left[0][axis] == right[0][axis] else 0
        nodes[n_node][2], nodes[n_node][3] = sub_node, axis | (first_node << 16)
        nodes.append([left[0], left[1], 0, 0])
        nodes.append([right[0], right[1], 0, 0])
        find_split(sub_node, first, left_count, sdepth + 1)
        find_split(sub_node + 1, first + left_count, right_count, sdepth + 1)

    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 4 * n + 1000))
    try:
        find_split(0, 0, n, 0)
    finally:
        sys.setrecursionlimit(old)
    arr = np.zeros(len(nodes), dtype=NODE_DTYPE)
    for i, (lo, hi, sub, aux) in enumerate(nodes):
        arr[i]["bmin"], arr[i]["bmax"], arr[i]["sub"], arr[i]["aux"] = lo, hi, sub, aux
    out.nodes, out.tris, out.perm = arr, tris, perm
    return out
