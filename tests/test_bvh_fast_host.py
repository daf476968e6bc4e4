"""The reference's fast builder on the host (snail_bvh_build_fast, include/snail_bvh_fast.h) against tests/bvh_fast_ref.py, an independent
numpy restatement of BVH::FindSplit (src/bvh/tree.cpp:161-287): byte-equal nodes, permuted triangle records, perm, nNodes and depth; the
edge cases of the defined deviation; the structure of the tree; the oracle's walk over it; the C-ABI.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import bvh_fast_ref as R
from tests import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "snail_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def fixture(name):
    return np.load(os.path.join(GOLDEN, name + "_tris.npz"))["tris"].reshape(-1, 9).astype(np.float32)


def soup(n, seed, spread=10.0, size=1.0):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-spread, spread, (n, 1, 3))
    return (c + rng.uniform(-size, size, (n, 3, 3))).reshape(n, 9).astype(np.float32)


# ---- the edge cases (shared with tests/test_gpu_bvh_fast.py) ----
def identical_tris(n=37):
    """every box equal: extent 0 on every axis, 0 * inf = NaN -> bin 0 -> one side empty -> the median split, all the way down"""
    return np.tile(np.array([[0, 0, 0, 0, 0, 0, 0, 0, 0]], np.float32) + np.array([1, 2, 3, 2, 2, 3, 1, 3, 3], np.float32), (n, 1))


def empty_side_field():
    """a field whose best SAH plane leaves one side empty: the node's box is far wider than where its triangles' CENTRES lie (one long
    sliver spans it, everything sits at one end), so the cheapest of the 15 planes has all centres... in bins 0 and the sliver's -- and a
    cluster of 40 coincident-centre triangles that splits into (40, 0)"""
    t = np.array([0, 0, 0, 1, 0, 0, 0, 1, 0], np.float32)
    same = np.tile(t, (40, 1))
    same[:, 1::3] += np.linspace(0, 0, 40, dtype=np.float32)[:, None]
    sliver = np.array([[0, 0, 0, 100, 0, 0, 0, 0.5, 0]], np.float32)
    return np.concatenate([same, sliver, same[:10] * np.float32(0.5)])


def signed_zero_tris():
    """vertices with +0 and -0 coordinates: Min / Max keep the LATER of two equal operands, so the box bytes depend on the fold order"""
    pz, nz = np.float32(0.0), np.float32(-0.0)
    rows = []
    for i in range(24):
        # (a box bound is -0 only through the first corner: ba + a and ca + a never give -0 from a finite edge)
        z0, z1 = (pz, nz) if i % 2 else (nz, pz)
        x = np.float32(i % 6)
        rows.append([x, z0, z1, x + 1, 1, 1, x, 1, 2])
    return np.array(rows, np.float32)


def big_leaf_soup():
    """large, heavily overlapping triangles around small offsets: every plane's cost comes within rounding of count * BoxSA(node)"""
    rng = np.random.default_rng(5)
    base = np.array([-50, -50, 0, 50, -50, 1, 0, 60, -1], np.float32)
    return (base + rng.uniform(-0.5, 0.5, (12, 9))).astype(np.float32)


def deep_line():
    """triangles of unit size at +-3^k along x over fp32's whole exponent range: one or two leave per level, 60 levels deep (the unit size
    swallows every offset below about 1e-7, which is what ends it there)"""
    tri = np.array([0, 0, 0, 1, 0, 0, 0, 1, 1], np.float64)
    rows = []
    for k in range(-84, 81):
        for s in (1, -1):
            t = tri.copy()
            t[0::3] += s * 3.0 ** k
            rows.append(t)
    return np.array(rows).astype(np.float32)


def deep_chain(ks=range(-68, 68), ratio=2.0):
    """A chain of shrinking triangles at x = +-ratio^k, each scaled with its position (size 1e-3 |x|): every binned split takes the
    outermost one or two off, so the depth grows with the number of binades the chain spans.  Depths of the cases used here (asserted
    where they are used): 272 triangles, ratio 2, k in [-68 + d, 68 + d): d = 0 -> 65, d = -6 -> 64, d = -5 -> 63; ratio 1.9, d = 0 ->
    50; k in [-126, 126) (504 triangles, all of fp32's normal range) -> 181."""
    rows = []
    for k in ks:
        for sg in (1.0, -1.0):
            x = sg * float(ratio) ** k
            s = 1e-3 * abs(x)
            rows.append([x, 0, 0, x + s, 0, 0, x, s, s])
    return np.array(rows, np.float64).astype(np.float32)


# depth -> a chain of 272 triangles that deep (SNAIL_MAX_DEPTH = 64; the shallow traversal stack takes 62)
CHAINS = {50: lambda: deep_chain(ratio=1.9), 63: lambda: deep_chain(range(-73, 63)), 64: lambda: deep_chain(range(-74, 62)), 65: lambda: deep_chain()}


def raw_build_fast(tv):
    """snail_bvh_build_fast's own return code (HostBVH.build_fast raises on it) -> (rc, nNodes, depth)"""
    import ctypes as C
    from snail_amd import HostBVH, _lib
    from snail_amd.bvh import NODE_DTYPE
    tris = HostBVH.triangles(tv)
    nodes = np.zeros(2 * len(tris) + 2, dtype=NODE_DTYPE)
    perm = np.zeros(len(tris), np.int32)
    nn, depth = C.c_int(0), C.c_int(0)
    rc = _lib.lib().snail_bvh_build_fast(_lib.ptr(tris), len(tris), _lib.ptr(nodes), C.addressof(nn), C.addressof(depth), _lib.ptr(perm))
    return rc, nn.value, depth.value


def host_build(tv):
    from snail_amd import HostBVH
    return HostBVH.build_fast(tv)


def ref_build(tv):
    from snail_amd import HostBVH
    return R.build_fast(HostBVH.triangles(tv))


def assert_same_tree(hb, rt, what=""):
    assert len(hb.nodes) == len(rt.nodes), (what, len(hb.nodes), len(rt.nodes))
    assert hb.depth == rt.depth, (what, hb.depth, rt.depth)
    assert np.array_equal(hb.perm, rt.perm), what
    assert hb.nodes.tobytes() == rt.nodes.tobytes(), what
    assert hb.tris.tobytes() == rt.tris.tobytes(), what


_cache = {}


def built(name):
    if name not in _cache:
        tv = {"box": lambda: fixture("box"), "lancia": lambda: fixture("lancia"), "identical": identical_tris, "empty_side": empty_side_field,
              "signed_zero": signed_zero_tris, "big_leaf": big_leaf_soup}[name]()
        _cache[name] = (tv, host_build(tv), ref_build(tv))
    return _cache[name]


@pytest.mark.parametrize("name", ["box", "lancia"])
def test_fixture_trees_match_the_restatement(name):
    tv, hb, rt = built(name)
    assert_same_tree(hb, rt, name)


@pytest.mark.parametrize("n", [1, 4, 5, 6, 16, 17, 100, 1000])
def test_random_soups_match_the_restatement(n):
    tv = soup(n, 100 + n)
    assert_same_tree(host_build(tv), ref_build(tv), n)


def leaves(nodes):
    return [i for i in range(len(nodes)) if nodes[i]["sub"] & 0x80000000]


def reachable(nodes):
    seen, todo = [], [(0, 0)]
    while todo:
        i, d = todo.pop()
        seen.append((i, d))
        if not nodes[i]["sub"] & 0x80000000:
            todo += [(int(nodes[i]["sub"]) + 1, d + 1), (int(nodes[i]["sub"]), d + 1)]
    return seen


def test_identical_triangles_take_the_median_split_all_the_way_down():
    tv, hb, rt = built("identical")
    assert_same_tree(hb, rt)
    n = len(tv)
    # the median split halves: every leaf holds <= 4 and the tree is as deep as halving n down to <= 4 makes it
    counts = sorted(int(hb.nodes[i]["aux"]) for i in leaves(hb.nodes))
    assert sum(counts) == n and counts[-1] <= 4
    depth, c = 0, n
    while c > 4:
        c, depth = c - c // 2, depth + 1
    assert hb.depth == depth
    assert np.array_equal(hb.perm, np.arange(n))      # nothing moves: one side of every partition is empty


def test_a_split_with_an_empty_side_falls_back_to_the_median():
    tv, hb, rt = built("empty_side")
    assert_same_tree(hb, rt)
    # some inner node's children hold count / 2 and the rest although their centres coincide (the binned counts were (count, 0))
    lo, hi = R.tri_boxes(hb.tris)
    found = False
    for i, _ in reachable(hb.nodes):
        if hb.nodes[i]["sub"] & 0x80000000:
            continue
        ch = int(hb.nodes[i]["sub"])
        spans = []
        for c in (ch, ch + 1):
            stack, first, cnt = [c], None, 0
            while stack:
                k = stack.pop()
                if hb.nodes[k]["sub"] & 0x80000000:
                    f = int(hb.nodes[k]["sub"] & 0x7fffffff)
                    first = f if first is None else min(first, f)
                    cnt += int(hb.nodes[k]["aux"])
                else:
                    stack += [int(hb.nodes[k]["sub"]), int(hb.nodes[k]["sub"]) + 1]
            spans.append((first, cnt))
        (f0, c0), (f1, c1) = spans
        axis = int(hb.nodes[i]["aux"]) & 0xffff
        centres = (lo[f0:f1 + c1, axis] + hi[f0:f1 + c1, axis]) * np.float32(0.5)
        if c0 + c1 > 4 and c0 == (c0 + c1) // 2 and np.all(centres == centres[0]):
            found = True
    assert found


def test_signed_zeros_keep_the_sign_the_ordered_fold_keeps():
    tv, hb, rt = built("signed_zero")
    assert_same_tree(hb, rt)
    bits = hb.nodes["bmin"].view(np.uint32), hb.nodes["bmax"].view(np.uint32)
    assert any((b == 0x80000000).any() for b in bits) and any((b == 0).any() for b in bits)
    # the root is the literal fold, in triangle order
    lo, hi = R.tri_boxes(R_tris(tv))
    assert R.fold_min_loop(lo[0], lo[1:]).tobytes() == hb.nodes[0]["bmin"].tobytes()


def R_tris(tv):
    from snail_amd import HostBVH
    return HostBVH.triangles(tv)


def test_overlapping_triangles_match_the_restatement():
    """The leaf rule count * BoxSA(node) < minCost next to costs that all but tie with it.  NOT asserted: that a leaf of more than 4
    triangles occurs, because none can.  A plane that leaves one side empty costs exactly count * BoxSA(node): the other side's box is
    the in-order fold of all the node's triangles, which is the node's box, bit for bit.  So minCost <= noSplitCost whenever such a plane
    exists, and the strict < does not fire.  When no such plane exists, bins 0 and 15 are both occupied.  Plane 1's left box then holds
    centres in the first sixteenth of the longest extent w and starts no lower than the node, so it is at most w / 8 long: its area is
    below half the node's (w (d + h) is at least two thirds of w (d + h) + d h, and seven eighths of it go), while the right box is no
    larger than the node's.  Plane 1 is cheaper than count * BoxSA(node) by a margin no rounding closes (areas of 0 or inf give equal
    costs, and < is strict).  For boxes without NaN the rule therefore never ends a node; the comparison itself is pinned, byte for
    byte, by every tree of this file."""
    tv, hb, rt = built("big_leaf")
    assert_same_tree(hb, rt)
    assert max(int(hb.nodes[i]["aux"]) for i in leaves(hb.nodes)) <= 4


@pytest.mark.parametrize("name", ["box", "lancia", "signed_zero", "empty_side"])
def test_structure(name):
    tv, hb, _ = built(name)
    assert sorted(hb.perm.tolist()) == list(range(len(tv)))
    assert hb.tris.tobytes() == R_tris(tv)[hb.perm].tobytes()
    lo, hi = R.tri_boxes(hb.tris)
    nodes = hb.nodes
    seen = reachable(nodes)
    assert sorted(i for i, _ in seen) == list(range(len(nodes)))
    assert max(d for i, d in seen if nodes[i]["sub"] & 0x80000000) == hb.depth
    span = {}
    for i, _ in sorted(seen, reverse=True):      # children have larger indices than their parent
        if nodes[i]["sub"] & 0x80000000:
            f, c = int(nodes[i]["sub"] & 0x7fffffff), int(nodes[i]["aux"])
            assert np.all(lo[f:f + c] >= nodes[i]["bmin"]) and np.all(hi[f:f + c] <= nodes[i]["bmax"])
            span[i] = (f, c)
        else:
            a, b = span[int(nodes[i]["sub"])], span[int(nodes[i]["sub"]) + 1]
            assert a[0] + a[1] == b[0]
            span[i] = (a[0], a[1] + b[1])
    covered = sorted(span[i] for i, _ in seen if nodes[i]["sub"] & 0x80000000)
    assert covered[0][0] == 0 and all(covered[k][0] + covered[k][1] == covered[k + 1][0] for k in range(len(covered) - 1))
    # every child box is the union of its triangles' boxes (numerically: the bytes are pinned by the restatement)
    for i in range(1, len(nodes)):
        f, c = span[i]
        assert np.array_equal(lo[f:f + c].min(axis=0), nodes[i]["bmin"]) and np.array_equal(hi[f:f + c].max(axis=0), nodes[i]["bmax"])


def test_partition_closed_form_is_libstdcxx_order():
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 7, 64, 65, 300):
        for p in (0.0, 0.2, 0.5, 0.9, 1.0):
            pred = rng.uniform(size=n) < p
            assert np.array_equal(R.partition_loop(pred), R.partition_order(pred)), (n, p)
    x = rng.integers(0, 3, (50, 3)).astype(np.float32) * np.float32(0.0) + rng.integers(-1, 2, (50, 3)).astype(np.float32)
    assert R.fold_min(x[0], x[1:]).tobytes() == R.fold_min_loop(x[0], x[1:]).tobytes()


def test_deep_tree_matches_the_restatement():
    tv = deep_line()
    hb, rt = host_build(tv), ref_build(tv)
    assert_same_tree(hb, rt)
    assert hb.depth == 60


@pytest.mark.parametrize("depth", [50, 63, 64])
def test_chains_up_to_the_depth_limit_match_the_restatement(depth):
    tv = CHAINS[depth]()
    hb, rt = host_build(tv), ref_build(tv)
    assert_same_tree(hb, rt)
    assert hb.depth == depth and len(tv) == 272


@pytest.mark.parametrize("make,depth", [(CHAINS[65], 65), (lambda: deep_chain(range(-126, 126)), 181)], ids=["one_level_too_deep", "whole_exponent_range"])
def test_a_chain_deeper_than_the_limit_is_error_2(make, depth):
    """the reference asserts depth <= BVH::maxDepth; here the build returns 2 and the message names the depth the restatement finds"""
    from snail_amd import HostBVH, _lib
    tv = make()
    assert ref_build(tv).depth == depth > 64
    rc, _, got = raw_build_fast(tv)
    assert rc == 2 and got == depth
    assert ("depth %d exceeds 64" % depth) in _lib.lib().snail_last_error().decode()
    with pytest.raises(_lib.SnailError):
        HostBVH.build_fast(tv)


def test_oracle_walks_the_fast_tree():
    """box scene, 256 x 256: the hit triangle agrees with the sweep tree's frame through perm on >= 99 % of the hit pixels, and t is
    bit-equal wherever it does (elsewhere the order-dependent packet culls pick another of two exact ties)"""
    from snail_amd import HostBVH, survey_camera
    tv, hb, _ = built("box")
    cam = survey_camera(tv).as_array13()
    sweep = O.OracleScene(tv)
    fast = O.OracleScene.from_arrays(hb.tris, hb.nodes, hb.depth, hb.perm)
    t0, _, _, id0, _ = sweep.render_primary(cam, 256, 256, threads=2)
    t1, _, _, id1, _ = fast.render_primary(cam, 256, 256, threads=2)
    hit = np.isfinite(t0)
    assert np.array_equal(hit, np.isfinite(t1)) and hit.sum() > 10000
    same = hit & (np.asarray(sweep.perm)[np.where(hit, id0, 0)] == hb.perm[np.where(hit, id1, 0)])
    print("agreeing hit pixels: %d of %d" % (same.sum(), hit.sum()))
    assert np.array_equal(t0[same].view(np.uint32), t1[same].view(np.uint32))
    assert same.sum() >= 0.99 * hit.sum()


# ---- ABI ----
def test_signatures_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "snail_bvh_fast.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|SnailScene \*)\s*(snail_[a-z_0-9]+)\s*\(", hdr, flags=re.M)))
    from snail_amd._lib import BVH_FAST_SIGNATURES, lib
    assert sorted(BVH_FAST_SIGNATURES) == declared == ["snail_bvh_build_fast", "snail_scene_create_fast_dev", "snail_scene_rebuild_fast_dev"]
    for name in declared:
        params = re.search(name + r"\s*\(([^;]*)\);", hdr).group(1)
        assert len(params.split(",")) == len(BVH_FAST_SIGNATURES[name][1]), name
    assert '#include "snail_hip.h"' in hdr
    L = lib()
    for name in declared:
        assert hasattr(L, name), "libsnailhip.so does not export " + name


def test_header_is_a_c_header(tmp_path):
    exe = str(tmp_path / "bvh_fast_c")
    src = os.path.join(ROOT, "tests", "c", "bvh_fast_c.c")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", src, "-o", exe, "-L" + LIBDIR, "-lsnailhip", "-Wl,-rpath," + LIBDIR])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "C bvh fast ABI ok: 3 symbols" in r.stdout, (r.returncode, r.stdout, r.stderr)
    from snail_amd._lib import BVH_FAST_SIGNATURES
    assert set(re.findall(r"ADDR\((snail_[a-z0-9_]+)\)", open(src).read())) == set(BVH_FAST_SIGNATURES)
