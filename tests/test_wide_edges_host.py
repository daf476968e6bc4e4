"""The cases of tests/wide_edge_cases.py reach the edges they are named for, shown on the NumPy restatement (tests/wide_ref.py) alone:
denormal intermediates that a flushing kernel would lose, a stack as full as the handle's slots, NaN / -inf / negative distances, index
lists with duplicates in and across waves, leaves as start nodes, and photon blocks with 0, 1, 6, 128 and 256 survivors.  No GPU.
Each test prints the counts it asserts (pytest -s shows them)."""
import os
import re

import numpy as np
import pytest

from snail_amd import photons
from tests import wide_edge_cases as EC
from tests import wide_ref as WR

F = np.float32


def differs(a, b):
    return not (EC.same_floats(a[0], b[0]) and np.array_equal(a[1], b[1]))


def test_the_float_comparison():
    nan2 = np.asarray([0x7fc00000, 0xffc00001], dtype=np.uint32).view(F)
    assert EC.same_floats(nan2, nan2[::-1])                                            # any NaN for a NaN
    assert EC.float_mismatches([0.0, 1.0, np.nan], [-0.0, 1.0, 1.0]).tolist() == [0, 2]   # +-0 told apart; a NaN for a number is wrong
    assert EC.float_mismatches([1.0], [np.nan]).tolist() == [0]
    assert WR.flush(np.asarray([2.0 ** -127, -2.0 ** -149, 2.0 ** -126, np.nan, -0.0], dtype=F)).view(np.uint32).tolist()[:3] == [0, 0x80000000, 0x00800000]


@pytest.mark.parametrize("k", [-33, -35, -38])
def test_scaled_boxes_with_denormal_squares_keep_their_hits(k):
    c = EC.case(EC.scale_name(k))
    b = EC.bvh(c["scene"])
    den = EC.denormal_squares(b.tris)
    want = EC.expected(c)
    finite = int(np.isfinite(want[0]).sum())
    print("%s: %d denormal n[c] * n[c] in %d triangles, %d of %d rays end finite" % (c["name"], den, len(b.tris), finite, len(want[0])))
    assert den >= 1 and finite >= 200
    flushed = EC.expected(c, "flush_denormals")
    assert differs(flushed, want)
    began = c["dist"] == np.inf
    assert (flushed[0][began] == np.inf).all()           # t0 = 0: a flushing kernel loses every hit


@pytest.mark.parametrize("k", EC.DEAD_SCALES)
def test_scaled_boxes_whose_squares_leave_the_range_lose_every_hit(k):
    c = EC.case(EC.scale_name(k))
    d, v = EC.expected(c)
    began = c["dist"] == np.inf
    print("%s: %d rays began at +inf, %d of them end at +inf; %d box tests, %d triangle tests" % (c["name"], began.sum(), (d[began] == np.inf).sum(), v[:, 0].sum(), v[:, 1].sum()))
    assert began.sum() == 128 and (d[began] == np.inf).all() and np.array_equal(d[~began].view(np.uint32), c["dist"][~began].view(np.uint32))
    assert v[:, 0].sum() > 0 and v[:, 1].sum() > 0


def test_an_ordinary_scale_has_nothing_to_flush():
    c = EC.case("scaled_+20")
    assert EC.denormal_squares(EC.bvh(c["scene"]).tris) == 0 and not differs(EC.expected(c, "flush_denormals"), EC.expected(c))


def test_tiny_rays():
    c = EC.case("tiny_rays")
    d, v = EC.expected(c)
    tiny = lambda a: (a != 0) & (np.abs(a) < WR.TINY)      # noqa: E731
    print("tiny_rays: %d denormal origin components, initial distances denormal %d, -0.0 %d, -inf %d; %d end finite" %
          (tiny(c["origin"]).sum(), tiny(c["dist"]).sum(), (c["dist"].view(np.uint32) == 0x80000000).sum(), (c["dist"] == -np.inf).sum(), np.isfinite(d).sum()))
    assert tiny(c["origin"]).all() and tiny(c["dist"]).sum() >= 2 and (c["dist"].view(np.uint32) == 0x80000000).any() and (c["dist"] == -np.inf).any()
    assert differs(EC.expected(c, "flush_denormals"), (d, v))
    assert (d[c["dist"] == -np.inf] == -np.inf).all() and (v[c["dist"] == -np.inf] == [2, 0]).all()      # -inf fails both boxes under the root


@pytest.mark.parametrize("scene", EC.CHAIN_SCENES)
def test_deep_chains(scene):
    c = [c for c in EC.walk_cases() if c["scene"] == scene][0]
    b = EC.bvh(scene)
    diag = {}
    d, v = EC.expected(c, diag=diag)
    path, (most, _) = EC.inner_nodes_on_the_longest_path(b.nodes), EC.most_stacked(b.nodes)
    fin = np.isfinite(d)
    print("%s: %d rays, depth %d, %d inner nodes on the longest path, most stacked %d, max_sp %d; NaN %d, finite > 0 %d, finite < 0 %d; "
          "hits in %d binades" % (c["name"], len(d), b.depth, path, most, diag["max_sp"].max(), np.isnan(d).sum(), (fin & (d > 0)).sum(),
                                  (fin & (d < 0)).sum(), len(set(np.frexp(d[fin])[1].tolist()))))
    assert 190 <= len(d) <= 220 and b.depth == int(scene[5:7]) == path
    # a ray reaches the leaf that takes the most stack the tree can ask for, and a stack of exactly that size is enough
    assert diag["max_sp"].max() == most
    assert not differs(EC.expected(c, slots=most), (d, v))
    assert differs(EC.expected(c, "stack_short", slots=most), (d, v))
    # (every eighth triangle of each sign is aimed at, in turn from in front and from behind; those of 2^-27 < |x| < 2^41 can be hit:
    # 68 binades, 8 or 9 rays of each sign and side)
    assert np.isnan(d).any() and (fin & (d > 0)).sum() >= 16 and (fin & (d < 0)).sum() >= 16 and len(set(np.frexp(d[fin])[1].tolist())) >= 16
    assert differs(EC.expected(c, "flush_denormals"), (d, v))       # the chain spans 2^-74 .. 2^62: Collide0 under- and overflows
    if scene == "chain64_left":
        # every turn on the longest path is a left turn: the stack holds as many entries as that path has inner nodes, all 64 slots of
        # a 64-level handle, and the kernel's test off by one ends a ray early
        assert most == path == 64
        assert not differs(EC.expected(c, slots=64), (d, v)) and differs(EC.expected(c, "stack_short", slots=64), (d, v))
    else:
        # the builders' chains peel triangles off BOTH ends: the walk pops a right sibling before it enters it, so the deep path of
        # the tree as built stacks far fewer entries than it has levels
        assert most < path and not differs(EC.expected(c, "stack_short", slots=64), (d, v))


def test_the_left_leaning_tree_is_the_same_tree():
    a, b = EC.bvh("chain64"), EC.bvh("chain64_left")
    assert a.tris.tobytes() == b.tris.tobytes() and len(a.nodes) == len(b.nodes)
    assert a.nodes[0].tobytes() == b.nodes[0].tobytes() and a.nodes.tobytes() != b.nodes.tobytes()
    for c in a.nodes["sub"][~EC.is_leaf(a.nodes)].astype(np.int64):      # the same records, the two of a child pair swapped or not
        assert sorted(a.nodes[c:c + 2].tobytes()[k:k + 32] for k in (0, 32)) == sorted(b.nodes[c:c + 2].tobytes()[k:k + 32] for k in (0, 32))


def test_the_duplicate_list():
    c, distinct = EC.dups()
    idx = c["indices"].astype(np.int64)
    ok = (idx >= 0) & (idx < 130)
    assert len(idx) == 200 and len(distinct) == 130 and not ok[[0, 63, 64, 127]].any() and not ok[192:].any() and ok[:192].sum() == 188
    assert sorted(idx[~ok].tolist())[0] == -2 ** 31 and max(idx[~ok].tolist()) == 2 ** 31 - 1 and {-1, 130} <= set(idx[~ok].tolist())
    pos = {}
    for p in np.flatnonzero(ok):
        pos.setdefault(int(idx[p]), []).append(int(p) // 64)
    same = sum(1 for w in pos.values() if len(w) != len(set(w)))
    cross = sum(1 for w in pos.values() if len(set(w)) > 1)
    print("dups: %d entries, %d valid, %d rays listed twice in one wave, %d in different waves; initial distances: %d inf, %d finite" %
          (len(idx), ok.sum(), same, cross, np.isinf(c["dist"]).sum(), np.isfinite(c["dist"]).sum()))
    assert same >= 1 and cross >= 1 and np.isinf(c["dist"]).any() and np.isfinite(c["dist"]).any()
    h = EC.case("half_outside")["indices"].astype(np.int64)
    assert len(h) == 128 and len(set(h[:64].tolist())) == 64 and ((h[:64] >= 0) & (h[:64] < 130)).all() and not ((h[64:] >= 0) & (h[64:] < 130)).any()


def test_the_start_nodes():
    cases = EC.start_cases()
    for scene in ("box", "two"):
        nodes = EC.bvh(scene).nodes
        assert sorted(c["start"] for c in cases if c["scene"] == scene) == list(range(len(nodes)))
    nodes = EC.bvh("box").nodes
    leaves = [c["start"] for c in cases if c["scene"] == "box" and EC.is_leaf(nodes)[c["start"]]]
    print("start nodes: %d of the box's %d nodes are leaves (%s); two has %d node" % (len(leaves), len(nodes), leaves, len(EC.bvh("two").nodes)))
    assert leaves and (~EC.is_leaf(nodes)).any() and all(len(c["dist"]) == 65 for c in cases)
    c = EC.a_leaf_start()
    d, v = EC.expected(c)
    assert (v[:, 0] == 0).all() and (v[:, 1] == nodes["aux"][c["start"]]).all() and np.isfinite(d).any()     # the leaf alone, its box not tested


def test_the_photon_patterns():
    for name, (lights, count) in EC.PHOTON_SIZES.items():
        n = lights * count
        hit = EC.photon_pattern(name)
        per_block = np.bincount(np.flatnonzero(hit) // 256, minlength=(n + 255) // 256)
        print("%s: %d rays, %d blocks, %d scan rounds, %d kept; survivors per block %s ..." %
              (name, n, len(per_block), (len(per_block) + 1023) // 1024, hit.sum(), sorted(set(per_block.tolist()))[:6]))
        assert {0, 1, 6, 128, 256} <= set(per_block[:-1].tolist())
    blocks = lambda name: (EC.PHOTON_SIZES[name][0] * EC.PHOTON_SIZES[name][1] + 255) // 256      # noqa: E731
    assert blocks("one_round") == 1024 and blocks("one_block_more") == 1025 and blocks("three_rounds") == 2050 and blocks("odd_one_light") == 2051
    z = EC.photon_pattern("a_round_of_zeros")
    assert not z[1024 * 256:2048 * 256].any() and z[:1024 * 256].any() and z[2048 * 256:].any()


def test_the_odd_photon_distances():
    o, d = EC.odd_photon_rays()
    dist = EC.odd_photon_distances()
    fin = np.isfinite(dist)
    print("odd photons: %d rays; NaN %d, -inf %d, +inf %d, finite < 0 %d, finite > 0 %d" %
          (len(dist), np.isnan(dist).sum(), (dist == -np.inf).sum(), (dist == np.inf).sum(), (fin & (dist < 0)).sum(), (fin & (dist > 0)).sum()))
    assert len(dist) == 67
    for what in (np.isnan(dist), dist == -np.inf, dist == np.inf, fin & (dist < 0), fin & (dist > 0)):
        assert what.sum() >= 10
    l7 = [[0.0, 0.0, 0.0, 1.0, 0.5, 0.25, 1.0]]
    want = WR.photons(o, d, dist, l7, 67, photons.PHOTON)
    assert len(want) == 67 - (dist == np.inf).sum()
    less, finite = (WR.photons(o, d, dist, l7, 67, photons.PHOTON, mutation=m) for m in WR.PHOTON_MUTATIONS)
    assert len(less) == len(want) - np.isnan(dist).sum() and len(finite) == fin.sum() and len({len(want), len(less), len(finite)}) == 3
    # a NaN or -inf distance leaves a record with a NaN position; a negative one a position behind the origin
    kept = np.flatnonzero(~(dist == np.inf))
    assert np.isnan(want["position"][np.isnan(dist[kept]) | (dist[kept] == -np.inf)]).any(axis=1).all()
    neg = fin[kept] & (dist[kept] < 0)
    assert (want["position"][neg][:, 2] < o[kept][neg][:, 2]).all()


def test_the_scratch_plan_takes_slots_round_across_streams_and_grows_used_ones():
    """from i alone: which slot sees which counts on which streams"""
    seen = {}
    for i in range(EC.SLOT_CALLS):
        seen.setdefault(i % EC.SLOTS, []).append(EC.slot_plan(i))
    grows = [s for s, v in seen.items() if any(b[0] > a[0] for a, b in zip(v, v[1:]))]           # a larger launch after the slot was used
    shrinks = [s for s, v in seen.items() if any(b[0] < a[0] for a, b in zip(v, v[1:]))]         # a smaller one in a buffer that stays
    crosses = [s for s, v in seen.items() if any(b[1] != a[1] for a, b in zip(v, v[1:]))]        # the next user is on the other stream
    print("scratch plan: %d calls on %d slots; slots that grow after use %s, that take a smaller launch %s, whose next user is on the "
          "other stream %s" % (EC.SLOT_CALLS, len(seen), grows, shrinks, crosses))
    assert len(seen) == EC.SLOTS and all(len(v) >= 2 for v in seen.values())
    assert len(grows) >= 4 and len(shrinks) >= 2 and len(crosses) == EC.SLOTS
    assert {EC.slot_plan(i)[0] for i in range(EC.SLOT_CALLS)} == set(EC.SLOT_COUNTS)
    # consecutive calls alternate between the streams, except where a turn round the slots begins
    assert all(EC.slot_plan(i)[1] != EC.slot_plan(i + 1)[1] for i in range(EC.SLOT_CALLS - 1) if (i + 1) % EC.SLOTS)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "snail_amd", "csrc", "snail_hip.hip")).read()
    assert re.search(r"#define SNAIL_DEFER_SLOTS (\d+)", src).group(1) == str(EC.SLOTS)
