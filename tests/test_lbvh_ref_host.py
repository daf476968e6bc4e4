"""tests/lbvh_ref.py, the NumPy restatement of the device LBVH builder (snail_scene_create_lbvh), and the cases of tests/lbvh_cases.py, on
the CPU: every case reaches what it was built for, every restated tree is a valid BVH, the byte comparison notices each of four subtle
mutations of the builder, Karras' search equals the recursive split it is restated as, and the entry point's refusals run before any
device work.  tests/test_gpu_lbvh.py holds the device to the same trees byte for byte.  No GPU."""
import numpy as np
import pytest

from tests import lbvh_cases as K
from tests import lbvh_ref as R
from tests import oracle_lib as O

ONE_BIT = sorted(1 << b for b in range(30))


def codes_of(name):
    q, t = R.quantise(K.verts(name))
    return R.morton_codes(q), q, t


def records_of(name, perm):
    return R.tri_records(K.verts(name)[perm])


# ---- (a) every restated tree is a valid BVH, and every case is what it says ----
@pytest.mark.parametrize("name,max_leaf", K.ALL)
def test_restated_tree_is_a_valid_bvh(name, max_leaf):
    nodes, perm, depth = K.ref(name, max_leaf)
    n = len(K.verts(name))
    R.check_tree(nodes, records_of(name, perm), perm, K.verts(name), max_leaf, depth)
    if n <= max_leaf:          # the root leaf: one record, everything else stays the empty leaf
        assert depth == 0 and nodes["sub"][0] == R.LEAF and nodes["aux"][0] == n
        assert nodes[1:].tobytes() == R.empty_nodes(2 * n - 2).tobytes()
    else:
        assert depth >= 1 and not nodes["sub"][0] & R.LEAF and nodes["sub"][0] == 1
    # slots below a collapsed subtree are the empty leaf of k_fill_empty
    seen, todo = set(), [0]
    while todo:
        i = todo.pop()
        seen.add(i)
        if not nodes["sub"][i] & R.LEAF:
            todo += [int(nodes["sub"][i]), int(nodes["sub"][i]) + 1]
    unused = np.array(sorted(set(range(len(nodes))) - seen), dtype=np.int64)
    assert nodes[unused].tobytes() == R.empty_nodes(len(unused)).tobytes()
    assert (max_leaf == 1 or n == 1) == (len(unused) == 0)


def test_records_restated_equal_the_host_records():
    """check_tree compares triangle records with tri_records: that restatement is snail_tris_from_verts' bytes on every case"""
    from snail_amd import HostBVH
    for name in K.NAMES:
        assert R.tri_records(K.verts(name)).tobytes() == HostBVH.triangles(K.verts(name)).tobytes(), name


def test_soup_sizes_cover_the_root_leaf_and_two_collapsed_children():
    for n in K.SOUP_SIZES:
        for m in K.MAX_LEAF:
            nodes, _, depth = K.ref("soup%d" % n, m)
            assert (depth == 0) == (n <= m)
    nodes, _, depth = K.ref("soup65", 64)
    assert depth == 1 and nodes["sub"][1] & R.LEAF and nodes["sub"][2] & R.LEAF and nodes["aux"][1] + nodes["aux"][2] == 65
    assert R.check_tree(nodes, records_of("soup65", K.ref("soup65", 64)[1]), K.ref("soup65", 64)[1], K.verts("soup65"), 64, 1) == 2
    leaves = K.ref("soup1025", 64)[0]
    assert 8 < leaves["aux"][(leaves["sub"] & R.LEAF) != 0].max() <= 64          # leaves larger than anything tested before


def test_identical_triangles_have_one_code_and_keep_their_order():
    codes, _, _ = codes_of("identical300")
    assert len(set(codes.tolist())) == 1
    for m in K.MAX_LEAF:
        assert np.array_equal(K.ref("identical300", m)[1], np.arange(300))


def test_clusters_are_eight_cells_of_forty():
    codes, _, _ = codes_of("clusters")
    vals, counts = np.unique(codes, return_counts=True)
    assert len(vals) == 8 and (counts == 40).all()
    mn, mx = R.tri_boxes(K.verts("clusters"))
    assert len(np.unique((mx - mn)[:, 0])) == 40


def test_flat_scene_has_zero_extent_and_zero_quanta_on_z():
    lo, hi = R.scene_bounds(K.verts("flat"))
    _, q, _ = codes_of("flat")
    assert hi[2] - lo[2] == 0 and (q[:, 2] == 0).all() and len(np.unique(q[:, 0])) > 50


def test_comb_holds_the_one_bit_codes_and_is_deep():
    codes, _, _ = codes_of("comb")
    lo, hi = R.scene_bounds(K.verts("comb"))
    assert (lo == 0).all() and (hi == 1).all() and len(K.verts("comb")) == 288
    assert sorted(codes[:30].tolist()) == ONE_BIT
    assert (codes[K.COMB_CELL0] == 0).all() and codes[286] == 0 and codes[287] == (1 << 30) - 1
    assert len(set(codes.tolist())) == 32
    depths = [K.ref("comb", m)[2] for m in K.MAX_LEAF]
    print("comb: restated depth at max_leaf 1 / 4 / 64 = %d / %d / %d" % tuple(depths))
    assert depths[0] >= 36 and depths[0] <= 64
    # Karras' search runs long here: some internal node's range is one-sided over more than 256 keys
    keys, _ = R.sorted_keys(K.verts("comb"))
    ch, rg = R.karras_topology(keys)
    assert sum(hi - lo > 256 and (c[0] < 0 or c[1] < 0) for c, (lo, hi) in zip(ch, rg)) >= 28


def test_walls_reach_cell_0_the_clamp_and_exact_boundaries():
    _, q, t = codes_of("walls")
    lo, hi = R.scene_bounds(K.verts("walls"))
    assert np.array_equal(lo, K.WALLS_LO.astype(np.float32)) and np.array_equal(hi, (K.WALLS_LO + K.WALLS_EXT).astype(np.float32))
    for k in range(3):
        on_min, on_max = t[:, k] == 0, t[:, k] == 1
        assert on_min.sum() >= 6 and on_max.sum() >= 6
        assert (q[on_min, k] == 0).all() and (q[on_max, k] == 1023).all()          # t * 1024 = 1024 only comes back through the clamp
        rows = np.arange(K.WALLS_BOUNDARY.start, K.WALLS_BOUNDARY.stop)[k * len(K.WALLS_CELLS):(k + 1) * len(K.WALLS_CELLS)]
        assert q[rows, k].tolist() == list(K.WALLS_CELLS)
        assert (t[rows, k] * np.float32(1024) == np.array(K.WALLS_CELLS, np.float32)).all()


def test_scaling_by_a_power_of_two_keeps_the_keys():
    """the quantisation is relative to the bounds: a scene times 2^+-20 has the same codes, the same perm and the same topology; 1e6 away
    from the origin the vertices round to 1/16 and the codes are others, still spread over the cells"""
    base = codes_of("scaled_up")[0]
    assert np.array_equal(base, codes_of("scaled_down")[0]) and len(set(base.tolist())) == 257
    for m in K.MAX_LEAF:
        up, down = K.ref("scaled_up", m), K.ref("scaled_down", m)
        assert np.array_equal(up[1], down[1]) and up[2] == down[2]
        assert up[0]["sub"].tobytes() == down[0]["sub"].tobytes() and up[0]["aux"].tobytes() == down[0]["aux"].tobytes()
    shifted = codes_of("shifted")[0]
    assert len(set(shifted.tolist())) > 200 and not np.array_equal(shifted, base)
    assert np.abs(K.verts("shifted")).min() > 9.9e5


def test_every_axis_and_both_orders_occur():
    seen = set()
    for name, m in K.ALL:
        nodes = K.ref(name, m)[0]
        inner = nodes[(nodes["sub"] & R.LEAF) == 0]
        seen |= set(zip((inner["aux"] & 0xffff).tolist(), (inner["aux"] >> 16).tolist()))
    assert seen == {(a, f) for a in (0, 1, 2) for f in (0, 1)}


# ---- (b) the byte comparison notices what a valid-BVH check cannot ----
def _reversed_ties(n):
    return np.arange(n, dtype=np.uint64)[::-1].copy()


_split = R.split_index
_first = R.first_node
MUTATIONS = {
    "ties_by_reversed_index": ("key_low", _reversed_ties),
    "quantise_by_1023": ("quant_scale", lambda: np.float32(1023.0)),
    "first_node_inverted": ("first_node", lambda s: 1 - _first(s)),
    "split_one_index_late": ("split_index", lambda keys, lo, hi: min(_split(keys, lo, hi) + 1, hi - 1)),
}


@pytest.mark.parametrize("which", list(MUTATIONS))
def test_byte_comparison_catches_the_mutation(monkeypatch, which):
    """Each mutant still builds a VALID tree (check_tree passes: that walk is why the earlier tests could not tell), and the byte comparison
    against the true restatement fails on at least one listed case."""
    attr, fn = MUTATIONS[which]
    want = {(name, m): K.ref(name, m) for name, m in K.ALL}
    monkeypatch.setattr(R, attr, fn)
    caught = []
    for name, m in K.ALL:
        if len(K.verts(name)) > 1100:
            continue
        got = R.build(K.verts(name), m)
        R.check_tree(got[0], records_of(name, got[1]), got[1], K.verts(name), m, got[2])
        if not R.same_tree(got, want[(name, m)]):
            caught.append((name, m))
    print("%s: caught on %d case(s), e.g. %s" % (which, len(caught), caught[:4]))
    assert caught
    if which == "ties_by_reversed_index":
        assert ("identical300", 1) in caught and ("clusters", 4) in caught
    if which == "quantise_by_1023":
        assert ("walls", 1) in caught
    monkeypatch.undo()
    assert R.same_tree(R.build(K.verts("walls"), 4), want[("walls", 4)])


def test_signed_zero_boxes_compare_equal_and_nothing_else_does():
    nodes, perm, depth = (x.copy() if hasattr(x, "copy") else x for x in K.ref("flat", 4))
    other = nodes.copy()
    other["bmin"][0][0] = np.float32(0.0); nodes["bmin"][0][0] = np.float32(-0.0)
    assert R.same_tree((nodes, perm, depth), (other, perm, depth))
    other["bmin"][0][0] = np.float32(1e-45)
    assert not R.same_tree((nodes, perm, depth), (other, perm, depth))
    assert not R.same_tree((nodes, perm, depth + 1), (nodes, perm, depth))
    unused = nodes.copy(); unused["aux"][-1] ^= 1
    assert not R.same_tree((unused, perm, depth), (nodes, perm, depth))


# ---- (c) Karras' search and the recursive split are one topology ----
@pytest.mark.parametrize("name", [n for n in K.NAMES if n != "soup1"])
def test_karras_search_equals_the_recursive_split(name):
    keys, _ = R.sorted_keys(K.verts(name))
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert R.karras_topology(keys) == R.recursive_topology(keys)


# ---- (d) refusals come before any device work ----
def raw_create_lbvh(tv, n, max_leaf, perm=None, ms=None):
    from snail_amd import _lib
    L = _lib.lib()
    h = L.snail_scene_create_lbvh(_lib.ptr(tv), n, 0, max_leaf, _lib.ptr(perm), ms)
    return h, L.snail_last_error().decode()


@pytest.mark.parametrize("what,n,max_leaf", [("null", 4, 4), ("verts", 0, 4), ("verts", -1, 4), ("verts", 4, 0), ("verts", 4, 65)],
                         ids=["null_vertices", "no_triangles", "negative_count", "max_leaf_0", "max_leaf_65"])
def test_refusals_need_no_device(what, n, max_leaf):
    tv = None if what == "null" else np.ascontiguousarray(K.verts("soup4"))
    perm = np.full(4, -7, np.int32)
    h, msg = raw_create_lbvh(tv, n, max_leaf, perm)
    assert not h
    assert "snail_scene_create_lbvh" in msg and "bad arguments" in msg and "1 <= maxLeafTris <= 64" in msg, msg
    assert (perm == -7).all()


# ---- non-finite vertices: what the device is expected to build, and whether the oracle can walk it ----
@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
def test_oracle_walks_the_expected_tree_of_a_non_finite_vertex(value):
    """fminf / fmaxf drop the NaN from every box and bound (the triangle's record keeps it); an infinite vertex makes the scene's extent on
    that axis infinite, every centre quantises to cell 0 there, and the boxes above that triangle reach +inf.  Either way the expected tree
    is a tree the oracle renders, so tests/test_gpu_lbvh.py compares frames for both inputs."""
    from snail_amd import survey_camera
    tv = K.nonfinite_soup(value)
    nodes, perm, depth = R.build(tv, 4)
    tris = R.tri_records(tv[perm])
    assert not R.fast_ok(nodes, tris)
    assert np.isfinite(nodes["bmin"]).all() and not np.isnan(nodes["bmax"]).any()
    assert np.isinf(nodes["bmax"][0][1]) == np.isinf(value)
    if np.isinf(value):
        assert (R.quantise(tv)[0][:, 1] == 0).all()
    slot = int(np.nonzero(perm == 123)[0][0])
    assert not np.isfinite(np.ascontiguousarray(tris[slot:slot + 1]).view(np.float32)).all()
    good = K.nonfinite_soup(np.float32(0.0))
    cam = survey_camera(good)
    osc = O.OracleScene.from_arrays(tris, nodes, depth, perm)
    for mode in (O.MODE_IEEE, O.MODE_SSE):
        t, u, v, tid, st = osc.render_primary(cam.as_array13(), 128, 96, mode=mode, threads=2)
        assert np.isfinite(t).sum() > 200 and not np.isnan(t).any() and st[0] > 0
