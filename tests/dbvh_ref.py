"""Test-side restatement of the reference's two-level tree (DBVH, src/dbvh/tree.cpp, src/dbvh/traverse.cpp, src/dbvh/tree.h): the
top-level build and walk written out literally in float32 numpy, the inner level through the oracle's pinned BVH walks
(orc_trace_rays / orc_trace_shadow with IN/OUT distance).  Test infrastructure only; the deviations it shares with the library are
the two defined in include/snail_instances.h (bins of a zero extent, barycentrics at the hit's own quad)."""
from __future__ import annotations

import numpy as np

from tests import oracle_lib as O

F = np.float32
NODE_DTYPE = np.dtype([("bmin", "<f4", 3), ("bmax", "<f4", 3), ("sub", "<u4"), ("aux", "<i4")])
INF = F(np.inf)


def fmin(a, b):
    return a if a < b else b    # veclib Min (vecbase.h:76), _mm_min_ps


def fmax(a, b):
    return a if a > b else b


# ---- build: ObjectInstance::ComputeBBox, DBVH::Construct / FindSplit ----------------------------------------------------------------
def instance_box(xf12, b6):
    r = [[F(xf12[3 * c + k]) for k in range(3)] for c in range(3)]
    t = [F(xf12[9 + c]) for c in range(3)]
    x0, x1 = F(b6[0]), F(b6[3])
    y = [F(b6[1]), F(b6[1]), F(b6[4]), F(b6[4])]
    z = [F(b6[2]), F(b6[5]), F(b6[2]), F(b6[5])]
    lo, hi = [], []
    for c in range(3):
        mn, mx = [], []
        for l in range(4):
            p0 = y[l] * r[c][1] + z[l] * r[c][2]
            p1 = x1 * r[c][0] + p0
            p0 = p0 + x0 * r[c][0]
            mn.append(fmin(p0, p1)); mx.append(fmax(p0, p1))
        lo.append(fmin(fmin(mn[0], mn[1]), fmin(mn[2], mn[3])) + t[c])
        hi.append(fmax(fmax(mx[0], mx[1]), fmax(mx[2], mx[3])) + t[c])
    return lo, hi


def box_add(a, b):
    return [fmin(a[0][k], b[0][k]) for k in range(3)], [fmax(a[1][k], b[1][k]) for k in range(3)]


def box_sa(b):
    w, h, d = b[1][0] - b[0][0], b[1][1] - b[0][1], b[1][2] - b[0][2]
    return (w * (d + h) + d * h) * F(2.0)


def bin_of(c, sub, mul, n_bins):
    with np.errstate(all="ignore"):
        v = (F(c) - sub) * mul
    if not (v >= 0):
        return 0            # deviation: NaN (0 * inf of a zero extent) -> bin 0
    if not (v < n_bins):
        return n_bins - 1
    return int(v)


def partition(items, lo, hi, pred):
    """libstdc++ std::__partition for bidirectional iterators (bits/stl_algo.h): in place on items[lo:hi]"""
    while True:
        while True:
            if lo == hi:
                return lo
            if pred(items[lo]):
                lo += 1
            else:
                break
        hi -= 1
        while True:
            if lo == hi:
                return lo
            if not pred(items[hi]):
                hi -= 1
            else:
                break
        items[lo], items[hi] = items[hi], items[lo]
        lo += 1


def build(xf12, blas_index, blas_bbox6):
    """-> (nodes NODE_DTYPE, depth, perm): what snail_instances_build returns."""
    xf = np.asarray(xf12, dtype=np.float32).reshape(-1, 12)
    bi = np.asarray(blas_index, dtype=np.int32).reshape(-1)
    bb = np.asarray(blas_bbox6, dtype=np.float32).reshape(-1, 6)
    n = len(xf)
    items = [(instance_box(xf[i], bb[bi[i]]), i) for i in range(n)]
    nodes = []
    depth = [0]

    def push(b):
        nodes.append([list(b[0]), list(b[1]), 0, 0])
        return len(nodes) - 1

    root = items[0][0]
    for i in range(1, n):
        root = box_add(root, items[i][0])
    push(root)

    def find_split(nn, first, count, sdepth):
        bbox = (nodes[nn][0], nodes[nn][1])
        leaf = count <= 1
        if not leaf:
            size = [bbox[1][k] - bbox[0][k] for k in range(3)]
            axis = (2 if size[2] > size[1] else 1) if size[1] > size[0] else (2 if size[2] > size[0] else 0)
            n_bins = 8 if count < 8 else 16
            with np.errstate(all="ignore"):
                mul = F(n_bins) * (F(1.0) - F(0.0001)) / (bbox[1][axis] - bbox[0][axis])
            sub = bbox[0][axis]
            bins = [([INF] * 3, [-INF] * 3) for _ in range(n_bins)]
            cnt = [0] * n_bins
            for i in range(count):
                b = items[first + i][0]
                c = (b[1][axis] + b[0][axis]) * F(0.5)
                k = bin_of(c, sub, mul, n_bins)
                cnt[k] += 1
                bins[k] = box_add(bins[k], b)
            lb, lc, rb, rc = [None] * n_bins, [0] * n_bins, [None] * n_bins, [0] * n_bins
            rb[-1], rc[-1], lb[0], lc[0] = bins[-1], cnt[-1], bins[0], cnt[0]
            for k in range(1, n_bins):
                lb[k] = box_add(lb[k - 1], bins[k]); lc[k] = lc[k - 1] + cnt[k]
            for k in range(n_bins - 2, -1, -1):
                rb[k] = box_add(rb[k + 1], bins[k]); rc[k] = rc[k + 1] + cnt[k]
            min_cost, min_idx = INF, 1
            no_split = F(1.0) * F(count) * box_sa(bbox)
            with np.errstate(all="ignore"):
                for k in range(1, n_bins):
                    cost = (box_sa(lb[k - 1]) * F(lc[k - 1]) if lc[k - 1] else F(0)) + (box_sa(rb[k]) * F(rc[k]) if rc[k] else F(0))
                    if cost < min_cost:
                        min_cost, min_idx = cost, k
            min_cost = F(0) + F(1) * min_cost
            leaf = bool(no_split < min_cost)
        if leaf:
            depth[0] = max(depth[0], sdepth)
            nodes[nn][2] = first | 0x80000000
            nodes[nn][3] = count
            return
        partition(items, first, first + count, lambda it: bin_of((it[0][0][axis] + it[0][1][axis]) * F(0.5), sub, mul, n_bins) < min_idx)
        left_box, right_box, left_count, right_count = lb[min_idx - 1], rb[min_idx], lc[min_idx - 1], rc[min_idx]
        if left_count == 0 or right_count == 0:
            mid = count // 2
            left_box, right_box = items[first][0], items[first + count - 1][0]
            for i in range(1, mid):
                left_box = box_add(left_box, items[first + i][0])
            for i in range(mid, count):
                right_box = box_add(right_box, items[first + i][0])
            left_count, right_count = mid, count - mid
        sub_node = len(nodes)
        first_node = (0 if left_box[1][axis] < right_box[1][axis] else 1) if left_box[0][axis] == right_box[0][axis] else 0
        nodes[nn][2] = sub_node
        nodes[nn][3] = axis | (first_node << 16)
        push(left_box); push(right_box)
        find_split(sub_node, first, left_count, sdepth + 1)
        find_split(sub_node + 1, first + left_count, right_count, sdepth + 1)

    find_split(0, 0, n, 0)
    out = np.zeros(len(nodes), dtype=NODE_DTYPE)
    for i, (lo, hi, s, a) in enumerate(nodes):
        out[i]["bmin"], out[i]["bmax"], out[i]["sub"], out[i]["aux"] = lo, hi, s, a
    return out, depth[0], np.array([it[1] for it in items], dtype=np.int32)


# ---- walk: DBVH::TraversePrimary0 / TraverseShadow0 --------------------------------------------------------------------------------
def inv(x, mode):
    """Inv of the given arithmetic, element-wise (veclib: 1 / x, or rcpps + one Newton step)"""
    x = np.asarray(x, dtype=np.float32)
    if mode == O.MODE_IEEE:
        with np.errstate(all="ignore"):
            return (F(1.0) / x).astype(np.float32)
    t = O.raw_approx(0, np.ascontiguousarray(x).view(np.uint32).reshape(-1), mode == O.MODE_TABLE).view(np.float32).reshape(x.shape)
    with np.errstate(all="ignore"):
        return ((t + t) - ((x * t) * t)).astype(np.float32)


def _minmax(v, act, masked):
    """ComputeMinMax (src/rtbase.cpp:61-121) as the device restates it: per SSE slot a sequential fold over the quads (masked lanes
    skipped, the fold seeded from the first active lane of the first quad with one), then Minimize / Maximize over the slots."""
    size = v.shape[0]
    q = 0
    while q < size and act[q] == 0:
        q += 1
    if q == size:
        return [F(0)] * 3, [F(0)] * 3
    k0 = (act[q] & -act[q]).bit_length() - 1
    lo, hi = [], []
    for c in range(3):
        mn_s, mx_s = [], []
        for l in range(4):
            mn = mx = v[q, c, k0] if masked else v[0, c, l]
            for qq in range(q if masked else 1, size):
                if not (act[qq] >> l) & 1:
                    continue
                x = v[qq, c, l]
                mn = mn if mn < x else x
                mx = mx if mx > x else x
            mn_s.append(mn); mx_s.append(mx)
        lo.append(fmin(fmin(mn_s[0], mn_s[1]), fmin(mn_s[2], mn_s[3])))
        hi.append(fmax(fmax(mx_s[0], mx_s[1]), fmax(mx_s[2], mx_s[3])))
    return lo, hi


def _test_interval(node, iv):
    with np.errstate(all="ignore"):
        lmin = lmax = F(0)
        for k in range(3):
            l1 = iv["minIDir"][k] * (node["bmin"][k] - iv["maxOrg"][k])
            l2 = iv["maxIDir"][k] * (node["bmin"][k] - iv["maxOrg"][k])
            l3 = iv["minIDir"][k] * (node["bmax"][k] - iv["minOrg"][k])
            l4 = iv["maxIDir"][k] * (node["bmax"][k] - iv["minOrg"][k])
            lo = fmin(fmin(l1, l2), fmin(l3, l4))
            hi = fmax(fmax(l1, l2), fmax(l3, l4))
            if k == 0:
                lmin, lmax = lo, hi
            else:
                lmin, lmax = fmax(lmin, lo), fmin(lmax, hi)
    return lmax >= 0 and lmin <= lmax


def _box_test(node, org, idir, dist, first, last, shared, shadow):
    """BBox::Test (src/bounding_box.cpp:61-200): the first / last quad of [first, last] with a passing lane, or None"""
    passing = []
    with np.errstate(all="ignore"):
        for q in range(first, last + 1):
            ok = False
            for l in range(4):
                lmin = lmax = F(0)
                for k in range(3):
                    o = org[0, k, 0] if shared else org[q, k, l]
                    l1 = idir[q, k, l] * (node["bmin"][k] - o)
                    l2 = idir[q, k, l] * (node["bmax"][k] - o)
                    lo, hi = fmin(l1, l2), fmax(l1, l2)
                    if k == 0:
                        lmin, lmax = lo, hi
                    elif shadow:
                        lmin, lmax = fmax(lo, lmin), fmin(hi, lmax)
                    else:
                        lmin, lmax = fmax(lmin, lo), fmin(lmax, hi)
                d = dist[q, l]
                ok |= (lmax >= 0 and lmin <= fmin(lmax, d)) if shadow else not (lmax < 0 or lmin > fmin(lmax, d))
            if ok:
                passing.append(q)
    return (passing[0], passing[-1]) if passing else None


class Ref:
    """The instanced scene for the restatement: BLAS oracle scenes, top-level nodes, xf12 / blas index in builder-slot order."""

    # instrumentation of traverse() for the tests (it enters no result): the longest top-level stack any packet has held, and the
    # (axis, firstNode, sign[axis]) triples met at inner nodes; a test resets them before the walks it wants to look at
    max_stack = 0
    orders_seen = set()

    def __init__(self, blas_oracles, nodes, xf12_slots, blas_index_slots):
        self.blas = list(blas_oracles)
        self.nodes = np.asarray(nodes).view(NODE_DTYPE)
        self.xf = np.asarray(xf12_slots, dtype=np.float32).reshape(-1, 12)
        self.bi = np.asarray(blas_index_slots, dtype=np.int32).reshape(-1)

    def _collide(self, slot, first, last, org, d, mask, dist, obj, elem, bary, shared, shadow, mode, stats):
        xf = self.xf[slot]
        R = xf[:9].reshape(3, 3)
        T = xf[9:12]
        cnt = last - first + 1
        sd = d[first:last + 1]                               # [cnt, 3, 4]
        nd = np.empty_like(sd)
        for c in range(3):                                   # ITransformVec (src/dbvh/tree.h:34-38)
            nd[:, c, :] = (sd[:, 0, :] * R[0, c] + sd[:, 1, :] * R[1, c]) + sd[:, 2, :] * R[2, c]
        nid = inv(nd + F(0.00000001), mode)                  # SafeInv
        if shared:
            p = org[0, :, 0] - T
            o = np.array([(p[0] * R[0, c] + p[1] * R[1, c]) + p[2] * R[2, c] for c in range(3)], dtype=np.float32)
            iorg = np.repeat(o.reshape(1, 3, 1), 4, axis=2).astype(np.float32)
            iorg3 = o.copy()
        else:
            p = org[first:last + 1] - T.reshape(1, 3, 1)
            iorg = np.empty_like(p)
            for c in range(3):
                iorg[:, c, :] = (p[:, 0, :] * R[0, c] + p[:, 1, :] * R[1, c]) + p[:, 2, :] * R[2, c]
        blas = self.blas[self.bi[slot]]
        idist = np.ascontiguousarray(dist[first:last + 1])
        nd, nid, iorg = (np.ascontiguousarray(a, dtype=np.float32) for a in (nd, nid, iorg))
        if shadow:
            st = blas.trace_shadow(np.ascontiguousarray(iorg3), nd, nid, idist, 1, cnt, mode)
            dist[first:last + 1] = idist
        else:
            iobj = np.full((cnt, 4), -1, dtype=np.int32)
            ibary = np.zeros((cnt, 8), dtype=np.float32)
            imask = None if mask is None else np.ascontiguousarray(mask[first:last + 1])
            st = blas.trace_rays(iorg, nd, nid, imask, idist, iobj, ibary, 1, cnt, shared, mode)
            dist[first:last + 1] = idist
            hit = iobj != -1
            o_, e_ = obj[first:last + 1], elem[first:last + 1]
            o_[hit] = slot
            e_[hit] = iobj[hit]
            if bary is not None:
                b_ = bary[first:last + 1]
                u, v = b_[:, :4], b_[:, 4:]
                u[hit] = ibary[:, :4][hit]
                v[hit] = ibary[:, 4:][hit]
        stats += st

    def traverse(self, org, d, idir, mask, dist, obj, elem, bary, shared, shadow=False, mode=O.MODE_IEEE):
        """One packet, in place.  org [1 or size, 3, 4], d / idir [size, 3, 4], mask uint8 [size] or None, dist [size, 4], obj / elem
        int32 [size, 4] (ignored for shadow), bary [size, 8] or None.  -> TreeStats uint64[4]."""
        size = d.shape[0]
        stats = np.zeros(4, dtype=np.uint64)
        act = [int(mask[q]) & 15 if mask is not None else 15 for q in range(size)]
        mnD, mxD = _minmax(d, act, mask is not None)
        mnI, mxI = _minmax(idir, act, mask is not None)
        if shared:
            mnO = mxO = [org[0, k, 0] for k in range(3)]
        else:
            mnO, mxO = _minmax(org, act, mask is not None)
        iv = {"minIDir": mnI, "maxIDir": mxI, "minOrg": mnO, "maxOrg": mxO, "minDir": mnD, "maxDir": mxD}
        sign = [int(d[0, k, 0] < 0) for k in range(3)]
        stack = [(0, 0, size - 1)]
        nodes = self.nodes
        while stack:
            nn, first, last = stack.pop()
            while True:
                stats[1] += 1                                   # LoopIteration
                node = nodes[nn]
                if not _test_interval(node, iv):
                    break
                r = _box_test(node, org, idir, dist, first, last, shared, shadow)
                if r is None:
                    break
                first, last = r
                sub, aux = int(node["sub"]), int(node["aux"])
                if sub & 0x80000000:
                    for k in range(aux):
                        self._collide((sub & 0x7fffffff) + k, first, last, org, d, mask, dist, obj, elem, bary, shared, shadow, mode, stats)
                        stats[0] += last - first + 1
                    break
                fn = ((aux >> 16) & 0xffff) ^ sign[aux & 0xffff]
                stack.append((sub + (fn ^ 1), first, last))
                Ref.max_stack = max(Ref.max_stack, len(stack))
                Ref.orders_seen.add((aux & 0xffff, (aux >> 16) & 0xffff, sign[aux & 0xffff]))
                nn = sub + fn
        return stats

    def _primary_packet(self, cam, resx, resy, px, py, mode):
        """The 16x16 primary packet at pixel origin (px, py): (dist [64,4], bary [64,8], obj [64,4], elem [64,4], TreeStats)."""
        org = np.repeat(cam[:3].reshape(1, 3, 1), 4, axis=2).astype(np.float32)
        dd, ii = O.gen_packet(cam, resx, resy, px, py, mode)
        d = dd.reshape(64, 3, 4).copy(); idir = ii.reshape(64, 3, 4).copy()
        dist = np.full((64, 4), np.inf, dtype=np.float32)
        obj = np.zeros((64, 4), dtype=np.int32); elem = np.zeros((64, 4), dtype=np.int32)
        bary = np.zeros((64, 8), dtype=np.float32)
        stats = self.traverse(org, d, idir, None, dist, obj, elem, bary, True, False, mode)
        stats[2] += 256
        return dist, bary, obj, elem, stats

    def render_primary(self, cam13, resx, resy, mode=O.MODE_IEEE, rect=None):
        """Frame layout (t, u, v, instance, tri, stats) of the whole image, as snail_instances_trace_primary_dev.  rect = (x0, y0, w, h):
        only the packets at (x0 + 16 i, y0 + 16 j), i < (w + 15) // 16, j < (h + 15) // 16, are traced (stats are theirs) and only the
        pixels x < min(resx, x0 + w), y < min(resy, y0 + h) are stored; every other pixel keeps the miss."""
        t = np.full((resy, resx), np.inf, dtype=np.float32)
        u = np.zeros((resy, resx), dtype=np.float32)
        v = np.zeros((resy, resx), dtype=np.float32)
        inst = np.zeros((resy, resx), dtype=np.int32)
        tri = np.zeros((resy, resx), dtype=np.int32)
        stats = np.zeros(4, dtype=np.uint64)
        cam = np.asarray(cam13, dtype=np.float32)
        x0, y0, w, h = rect if rect is not None else (0, 0, resx, resy)
        xlim, ylim = min(resx, x0 + w), min(resy, y0 + h)
        for py in range(y0, y0 + 16 * ((h + 15) // 16), 16):
            for px in range(x0, x0 + 16 * ((w + 15) // 16), 16):
                dist, bary, obj, elem, st = self._primary_packet(cam, resx, resy, px, py, mode)
                stats += st
                for q in range(64):
                    y = py + (q >> 2)
                    for l in range(4):
                        x = px + 4 * (q & 3) + l
                        if x < xlim and y < ylim:
                            t[y, x], u[y, x], v[y, x] = dist[q, l], bary[q, l], bary[q, 4 + l]
                            inst[y, x], tri[y, x] = obj[q, l], elem[q, l]
        return t, u, v, inst, tri, stats

    def render_packets(self, cam13, resx, resy, packet_xy, mode=O.MODE_IEEE):
        """Packet-major [n, 256] planes (t, u, v, instance, tri) and the summed stats of the packets at the pixel origins packet_xy [n, 2],
        as snail_instances_trace_packets_dev: entry 4 q + l of a packet is lane l of quad q (pixel (px + 4 (q & 3) + l, py + (q >> 2)), the
        order render_primary unpacks), all 256 written, rays beyond the frame's edge included."""
        xy = np.asarray(packet_xy, dtype=np.int64).reshape(-1, 2)
        n = len(xy)
        t = np.zeros((n, 256), dtype=np.float32); u = np.zeros((n, 256), dtype=np.float32); v = np.zeros((n, 256), dtype=np.float32)
        inst = np.zeros((n, 256), dtype=np.int32); tri = np.zeros((n, 256), dtype=np.int32)
        stats = np.zeros(4, dtype=np.uint64)
        cam = np.asarray(cam13, dtype=np.float32)
        for i in range(n):
            dist, bary, obj, elem, st = self._primary_packet(cam, resx, resy, int(xy[i, 0]), int(xy[i, 1]), mode)
            stats += st
            t[i], u[i], v[i] = dist.reshape(256), bary[:, :4].reshape(256), bary[:, 4:].reshape(256)
            inst[i], tri[i] = obj.reshape(256), elem.reshape(256)
        return t, u, v, inst, tri, stats
