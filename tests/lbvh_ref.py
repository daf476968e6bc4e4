"""The device LBVH builder (snail_scene_create_lbvh, snail_amd/csrc/lbvh.inc) restated in NumPy and plain Python: float32 rounded per
operation, nothing imported from the product library.  build(tv, max_leaf) gives the node array (all 2n - 1 slots), perm and depth the
device must produce byte for byte; check_tree is the validity walk of a tree in the reference's record formats; karras_topology is a
line-by-line port of k_topology, kept to show that the recursive form used here numbers its nodes as Karras' search does.

The small functions quant_scale / key_low / split_index / first_node are the four places a builder of this kind goes subtly wrong; the
host tests replace each in turn and require the byte comparison to notice."""
import numpy as np

F = np.float32
NODE_DTYPE = np.dtype([("bmin", "<f4", 3), ("bmax", "<f4", 3), ("sub", "<u4"), ("aux", "<i4")])
TRI_DTYPE = np.dtype([("a", "<f4", 3), ("ba", "<f4", 3), ("ca", "<f4", 3), ("t0", "<f4"), ("it0", "<f4"), ("pad", "<i4"), ("plane", "<f4", 4)])
LEAF = 0x80000000


def _verts(tv):
    return np.ascontiguousarray(tv, dtype=F).reshape(-1, 3, 3)


def tri_boxes(tv):
    """per-triangle boxes; fminf / fmaxf drop a NaN operand, as np.fmin / np.fmax do"""
    v = _verts(tv)
    return np.fmin(v[:, 0], np.fmin(v[:, 1], v[:, 2])), np.fmax(v[:, 0], np.fmax(v[:, 1], v[:, 2]))


def scene_bounds(tv):
    v = _verts(tv).reshape(-1, 3)
    return np.fmin.reduce(v, axis=0), np.fmax.reduce(v, axis=0)


def quant_scale():
    return F(1024.0)


def quantise(tv):
    """-> (q uint32 [n, 3], t float32 [n, 3] after the clamp to [0, 1]): 10 bits per axis of the box centre within the scene's bounds"""
    lo, hi = scene_bounds(tv)
    mn, mx = tri_boxes(tv)
    with np.errstate(all="ignore"):
        ext = (hi - lo).astype(F)
        t = ((((mn + mx).astype(F) * F(0.5)).astype(F) - lo).astype(F) / ext).astype(F)
        t = np.where(ext > 0, t, F(0.0)).astype(F)
        t = np.fmin(np.fmax(t, F(0.0)), F(1.0))
        q = np.fmin((t * quant_scale()).astype(F), F(1023.0)).astype(np.uint32)
    return q, t


def morton_codes(q):
    """30 bits: x at 3b + 2, y at 3b + 1, z at 3b"""
    code = np.zeros(len(q), dtype=np.uint64)
    for b in range(10):
        for k in range(3):
            code |= ((q[:, k].astype(np.uint64) >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + 2 - k)
    return code


def key_low(n):
    """the key's low word: the input index, which makes keys unique and decides everything below one Morton cell"""
    return np.arange(n, dtype=np.uint64)


def sorted_keys(tv):
    """-> (keys as Python ints, ascending; perm int32: sorted position -> input triangle)"""
    q, _ = quantise(tv)
    low = key_low(len(q))
    keys = (morton_codes(q) << np.uint64(32)) | low
    order = np.argsort(keys, kind="stable")
    return [int(k) for k in keys[order]], order.astype(np.int32)


def split_index(keys, lo, hi):
    """the last index of [lo, hi] whose key has the highest bit in which keys[lo] and keys[hi] differ clear"""
    bit = (keys[lo] ^ keys[hi]).bit_length() - 1
    a, b = lo, hi          # keys[a] has the bit clear, keys[b] has it set
    while b - a > 1:
        m = (a + b) // 2
        if (keys[m] >> bit) & 1:
            b = m
        else:
            a = m
    return a


def recursive_topology(keys):
    """-> (children [n - 1][2], ranges [n - 1][2]) in k_topology's conventions (child >= 0: internal node, < 0: leaf ~child): the root is
    internal node 0, an internal left child [lo, g] is node g, an internal right child [g + 1, hi] is node g + 1"""
    n = len(keys)
    children, ranges = [None] * (n - 1), [None] * (n - 1)
    todo = [(0, 0, n - 1)] if n > 1 else []
    while todo:
        i, lo, hi = todo.pop()
        g = split_index(keys, lo, hi)
        children[i] = (~g if lo == g else g, ~(g + 1) if hi == g + 1 else g + 1)
        ranges[i] = (lo, hi)
        if lo != g:
            todo.append((g, lo, g))
        if hi != g + 1:
            todo.append((g + 1, g + 1, hi))
    return children, ranges


def karras_topology(keys):
    """k_topology (Karras 2012, algorithm 1) line by line, one loop iteration per thread"""
    n = len(keys)

    def delta(i, j):
        if j < 0 or j >= n:
            return -1
        return 64 - (keys[i] ^ keys[j]).bit_length()

    children, ranges = [None] * (n - 1), [None] * (n - 1)
    for i in range(n - 1):
        d = 1 if delta(i, i + 1) - delta(i, i - 1) >= 0 else -1
        dmin = delta(i, i - d)
        lmax = 2
        while delta(i, i + lmax * d) > dmin:
            lmax *= 2
        l, t = 0, lmax // 2
        while t >= 1:
            if delta(i, i + (l + t) * d) > dmin:
                l += t
            t //= 2
        j = i + l * d
        dnode = delta(i, j)
        s, t = 0, (l + 1) // 2
        while True:
            if delta(i, i + (s + t) * d) > dnode:
                s += t
            if t <= 1:
                break
            t = (t + 1) // 2
        g = i + s * d + (-1 if d < 0 else 0)
        lo, hi = min(i, j), max(i, j)
        children[i] = (~g if lo == g else g, ~(g + 1) if hi == g + 1 else g + 1)
        ranges[i] = (lo, hi)
    return children, ranges


def first_node(sep_axis):
    return 0 if sep_axis >= 0 else 1


def empty_nodes(n_slots):
    """what k_fill_empty writes: zero box, a leaf of no triangles"""
    nodes = np.zeros(n_slots, dtype=NODE_DTYPE)
    nodes["sub"] = LEAF
    return nodes


def build(tv, max_leaf):
    """-> (nodes NODE_DTYPE [2n - 1], perm int32 [n], depth)"""
    tv = np.ascontiguousarray(tv, dtype=F).reshape(-1, 9)
    n = len(tv)
    keys, perm = sorted_keys(tv)
    mn, mx = tri_boxes(tv[perm])
    nodes = empty_nodes(2 * n - 1)
    depth = 0

    def box(lo, hi):
        return np.fmin.reduce(mn[lo:hi + 1], axis=0), np.fmax.reduce(mx[lo:hi + 1], axis=0)

    todo = [(0, 0, n - 1, 0, 0)]          # (internal node, lo, hi, slot, level)
    while todo:
        i, lo, hi, slot, level = todo.pop()
        b = box(lo, hi)
        nodes["bmin"][slot], nodes["bmax"][slot] = b
        if hi - lo + 1 <= max_leaf:
            nodes["sub"][slot], nodes["aux"][slot] = LEAF | lo, hi - lo + 1
            depth = max(depth, level)
            continue
        g = split_index(keys, lo, hi)
        bl, br = box(lo, g), box(g + 1, hi)
        with np.errstate(all="ignore"):
            sep = ((br[0] + br[1]).astype(F) - (bl[0] + bl[1]).astype(F)).astype(F)
        axis, best = 0, F(-1.0)
        for k in range(3):
            if np.abs(sep[k]) > best:
                best, axis = np.abs(sep[k]), k
        nodes["sub"][slot], nodes["aux"][slot] = 1 + 2 * i, axis | (first_node(sep[axis]) << 16)
        todo.append((g, lo, g, 1 + 2 * i, level + 1))
        todo.append((g + 1, g + 1, hi, 2 + 2 * i, level + 1))
    return nodes, perm, depth


def tri_records(tv):
    """Triangle::Triangle + ComputeData as triRecord of lbvh.inc computes them: no contraction, IEEE sqrt and divide"""
    v = _verts(tv)
    out = np.zeros(len(v), dtype=TRI_DTYPE)
    with np.errstate(all="ignore"):
        a, ba, ca = v[:, 0], (v[:, 1] - v[:, 0]).astype(F), (v[:, 2] - v[:, 0]).astype(F)
        nx = ba[:, 1] * ca[:, 2] - ba[:, 2] * ca[:, 1]
        ny = ba[:, 2] * ca[:, 0] - ba[:, 0] * ca[:, 2]
        nz = ba[:, 0] * ca[:, 1] - ba[:, 1] * ca[:, 0]
        ln = np.sqrt(nx * nx + ny * ny + nz * nz)
        inv = F(1.0) / ln
        nx, ny, nz = nx * inv, ny * inv, nz * inv
        out["a"], out["ba"], out["ca"], out["t0"], out["it0"] = a, ba, ca, ln, inv
        out["plane"] = np.stack([nx, ny, nz, nx * a[:, 0] + ny * a[:, 1] + nz * a[:, 2]], axis=1)
    return out


def fast_ok(nodes, tris):
    """the fastOK conditions of snail_scene_create over ALL node slots and triangle records"""
    t = np.ascontiguousarray(tris).view(F).reshape(-1, 16)
    with np.errstate(all="ignore"):
        ok = (np.abs(t[:, :9]) <= F(1.0e9)).all() and (t[:, 9] > 0).all() and (t[:, 10] <= F(1.0e12)).all() and (t[:, 10] > 0).all()
        ok = ok and (np.abs(t[:, 12:16]) <= F(1.0e18)).all()
        ok = ok and (np.abs(nodes["bmin"]) <= F(1.0e9)).all() and (np.abs(nodes["bmax"]) <= F(1.0e9)).all() and (nodes["bmin"] <= nodes["bmax"]).all()
    return bool(ok)


def _boxes_plus_zero(nodes):
    b = np.concatenate([nodes["bmin"], nodes["bmax"]], axis=1).astype(F)
    return (b + F(0.0)).astype(F)          # -0 + +0 = +0: the sign of a zero bound is not part of the contract


def assert_same_tree(got, want, what=""):
    """got, want = (nodes, perm, depth): boxes equal as bytes after + 0.0f on both sides, everything else as raw bytes"""
    gn, gp, gd = got
    wn, wp, wd = want
    gn, wn = np.ascontiguousarray(gn).view(NODE_DTYPE).reshape(-1), np.ascontiguousarray(wn).view(NODE_DTYPE).reshape(-1)
    assert len(gn) == len(wn), (what, len(gn), len(wn))
    assert int(gd) == int(wd), (what, "depth", gd, wd)
    assert np.asarray(gp, np.int32).tobytes() == np.asarray(wp, np.int32).tobytes(), (what, "perm")
    for f in ("sub", "aux"):
        ne = np.nonzero(gn[f] != wn[f])[0]
        assert not len(ne), (what, f, "slot %d: %#x vs %#x (%d slots differ)" % (ne[0], gn[f][ne[0]], wn[f][ne[0]], len(ne)))
    gb, wb = _boxes_plus_zero(gn), _boxes_plus_zero(wn)
    ne = np.nonzero((gb.view(np.uint32) != wb.view(np.uint32)).any(axis=1))[0]
    assert not len(ne), (what, "box", "slot %d: %r vs %r (%d slots differ)" % (ne[0], gb[ne[0]], wb[ne[0]], len(ne)))


def same_tree(got, want):
    try:
        assert_same_tree(got, want)
    except AssertionError:
        return False
    return True


def check_tree(nodes, tris, perm, tv, max_leaf, depth):
    """A valid BVH in the reference's record formats: perm a permutation, 2n - 1 slots, triangle records those of the permuted input,
    children adjacent and inside their parent, every leaf of 1..max_leaf triangles bounding them, the leaves a partition of the triangle
    array, the deepest leaf at `depth`."""
    tv = _verts(tv)
    n = len(tv)
    perm = np.asarray(perm)
    assert sorted(perm.tolist()) == list(range(n)) and len(nodes) == 2 * n - 1
    want_tris = tri_records(tv[perm])
    for f in ("a", "ba", "ca", "t0", "it0", "plane"):
        assert np.ascontiguousarray(tris[f]).view(np.uint32).tobytes() == np.ascontiguousarray(want_tris[f]).view(np.uint32).tobytes(), "triangle record field " + f
    covered = np.zeros(n, dtype=np.int32)
    stack, max_depth, n_leaves = [(0, 0)], 0, 0
    while stack:
        i, d = stack.pop()
        nd = nodes[i]
        if nd["sub"] & 0x80000000:
            first, count = int(nd["sub"] & 0x7fffffff), int(nd["aux"])
            assert 1 <= count <= max_leaf and first + count <= n
            covered[first:first + count] += 1
            tb = tv[perm[first:first + count]].reshape(-1, 3)
            assert (tb.min(axis=0) >= nd["bmin"]).all() and (tb.max(axis=0) <= nd["bmax"]).all()
            max_depth = max(max_depth, d); n_leaves += 1
        else:
            c = int(nd["sub"])
            assert 0 < c and c + 1 < len(nodes) and (nd["aux"] & 0xffff) <= 2 and (nd["aux"] >> 16) <= 1
            for k in (0, 1):
                assert (nodes[c + k]["bmin"] >= nd["bmin"]).all() and (nodes[c + k]["bmax"] <= nd["bmax"]).all()
                stack.append((c + k, d + 1))
    assert (covered == 1).all() and max_depth == depth
    return n_leaves
