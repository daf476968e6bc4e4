"""BVH::WideTrace with one ray per lane (include/snail_wide.h) at its edges, against the NumPy restatement (tests/wide_ref.py) on the cases
of tests/wide_edge_cases.py (tests/test_wide_edges_host.py shows what each of them reaches): denormal intermediates, trees that fill the
per-lane stack, index lists with duplicates and numbers that name no ray, every node as start node, the counters' optional halves and
the host forms.  Distances: a NaN where the restatement has one, the same bits everywhere else; counters and their sums: equal."""
import numpy as np
import pytest
import torch

from snail_amd import _lib
from snail_amd.scene import Scene
from tests import wide_cases as WC
from tests import wide_edge_cases as EC

pytestmark = pytest.mark.gpu

SENTINEL = -7
FAST_DEV = ("chain64", "chain63", "chain50")       # walked on snail_scene_create_fast_dev handles, built on the device

_scenes = {}


def dev_scene(name):
    if name not in _scenes:
        _scenes[name] = Scene(EC.bvh(name), 0)
    return _scenes[name]


@pytest.fixture(scope="module", autouse=True)
def close_the_scenes():
    yield
    for sc in _scenes.values():
        sc.close()
    _scenes.clear()


def run(sc, case, visits=True, stats=(0, 0)):
    """-> (dist, visits, stats) of one device call; visits / stats = None: the call gets no such buffer.  The visits of rays that are not
    listed keep SENTINEL; stats = the words the accumulator holds before the call."""
    dev = sc._dev()
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    dist = up(case["dist"])
    d_visits = torch.full((len(case["dist"]), 2), SENTINEL, dtype=torch.int32, device=dev) if visits else None
    d_stats = torch.tensor(list(stats), dtype=torch.int64, device=dev) if stats is not None else None
    sc.wide_trace(up(case["origin"]), up(case["dir"]), dist, idir=up(case["idir"]), indices=up(case["indices"]), start_node=case["start"],
                  visits=d_visits, stats=d_stats)
    torch.cuda.synchronize()
    return dist.cpu().numpy(), None if d_visits is None else d_visits.cpu().numpy(), None if d_stats is None else d_stats.cpu().numpy()


def listed_rays(case):
    n = len(case["dist"])
    return np.arange(n) if case["indices"] is None else EC.valid_entries(case["indices"], n).astype(np.int64)


def check(case, got, want, counters=True, preset=(0, 0)):
    (d, v, st), (wd, wv) = got, want
    listed = listed_rays(case)
    rest = np.setdiff1d(np.arange(len(wd)), listed)
    bad = EC.float_mismatches(d, wd)
    assert len(bad) == 0, (case["name"], len(bad), bad[:8], d[bad[:8]], wd[bad[:8]])
    assert np.array_equal(d[rest].view(np.uint32), case["dist"][rest].view(np.uint32))       # untouched rays keep their bytes
    if v is not None:
        assert (v[rest] == SENTINEL).all(), case["name"]
        if counters:
            assert np.array_equal(v[listed], wv[listed]), (case["name"], np.flatnonzero((v[listed] != wv[listed]).any(axis=1))[:8])
    if st is not None and counters:
        sums = wv[listed].astype(np.int64).sum(axis=0)
        assert st.tolist() == [preset[0] + int(sums[0]), preset[1] + int(sums[1])], case["name"]


@pytest.mark.parametrize("name", [c["name"] for c in EC.walk_cases() if c["scene"] not in FAST_DEV])
def test_walk_cases(name):
    case = EC.case(name)
    got = run(dev_scene(case["scene"]), case)
    check(case, got, EC.expected(case))
    if name in ("scaled_-40", "scaled_+60"):
        began = case["dist"] == np.inf
        assert (got[0][began] == np.inf).all() and got[2][1] > 0
    if name in ("scaled_-33", "scaled_-35", "scaled_-38"):
        assert np.isfinite(got[0]).sum() >= 200           # a kernel that flushes denormals has t0 = 0 and loses every hit


@pytest.mark.parametrize("scene", FAST_DEV)
def test_deep_chains_on_fast_dev_handles(scene):
    """the committed tree of snail_scene_create_fast_dev; the expected values from the tree read back.  These handles size the stack by
    the builder's depth limit, which no binding reports and which is therefore not asserted; the chains stack 24, 24 and 14 entries,
    far fewer than either limit.  The stack is filled to its last slot in test_a_full_stack, on a snail_scene_create handle."""
    case = [c for c in EC.walk_cases() if c["scene"] == scene][0]
    sc = Scene.from_fast_dev(torch.from_numpy(np.ascontiguousarray(EC.verts(scene).reshape(-1, 9))).cuda(), 0)
    try:
        got = run(sc, case)
        b = sc.bvh
        assert b.depth == int(scene[5:7]) and int(sc.d_info.cpu()[0]) == 0
        check(case, got, EC.expected(case, tree=b))
        d = got[0]
        assert np.isnan(d).any() and (np.isfinite(d) & (d > 0)).any() and (np.isfinite(d) & (d < 0)).any()
    finally:
        sc.close()


def test_a_full_stack():
    """chain64_left: a 64-level handle whose longest path stacks 64 entries, one in every slot the launch reserves; a ray ended one
    slot early would lose the hit in the deepest leaf"""
    case = EC.case("chain64_left")
    b = EC.bvh("chain64_left")
    assert EC.most_stacked(b.nodes)[0] == 64 == b.depth
    got = run(dev_scene("chain64_left"), case)
    want, short = EC.expected(case, slots=64), EC.expected(case, "stack_short", slots=64)
    check(case, got, want)
    assert not (EC.same_floats(got[0], short[0]) and np.array_equal(got[1], short[1]))


def test_duplicates_and_numbers_that_name_no_ray():
    case, distinct = EC.dups()
    sc = dev_scene("box")
    plain = dict(case, indices=distinct)
    want = EC.expected(plain)
    # (with duplicates the counters are undefined: distances only, and the rays that are not listed -- there are none -- untouched)
    check(case, run(sc, case), want, counters=False)
    check(plain, run(sc, plain), want)


def test_the_counters_optional_halves_and_a_preset_accumulator():
    case = EC.case("scaled_-35")
    sc = dev_scene(case["scene"])
    want = EC.expected(case)
    d, v, st = run(sc, case, visits=False)
    assert v is None
    check(case, (d, v, st), want)
    d, v, st = run(sc, case, stats=None)
    assert st is None
    check(case, (d, v, st), want)
    preset = (2 ** 40 + 5, 7)
    check(case, run(sc, case, stats=preset), want, preset=preset)
    check(case, run(sc, case, visits=False, stats=None), want)


@pytest.mark.parametrize("name", ["box_subset", "box_idir_skew", "start_leaf"])
def test_the_host_form(name):
    case = EC.a_leaf_start() if name == "start_leaf" else [c for c in WC.small_cases() if c["name"] == name][0]
    sc = dev_scene(case["scene"])
    d, v, st = run(sc, case)
    dist = case["dist"].copy()
    visits = np.full((len(dist), 2), SENTINEL, dtype=np.int32)
    hs = sc.wide_trace_host(case["origin"], case["dir"], dist, idir=case["idir"], indices=case["indices"], start_node=case["start"], visits=visits)
    assert np.array_equal(dist.view(np.uint32), d.view(np.uint32)) and np.array_equal(visits, v) and hs.tolist() == st.tolist()
    rest = np.setdiff1d(np.arange(len(dist)), listed_rays(case))
    assert (visits[rest] == SENTINEL).all() and (name != "box_subset" or len(rest) == 53)
    check(case, (dist, visits, hs.astype(np.int64)), EC.expected(case))
    # stats2 is ADDED to; visits NULL with stats given and the reverse
    dist2 = case["dist"].copy()
    stats2 = np.asarray([2 ** 40 + 5, 7], dtype=np.uint64)
    ptr = _lib.ptr
    rc = _lib.lib().snail_wide_trace(sc._h, len(dist2), ptr(case["origin"]), ptr(case["dir"]), ptr(case["idir"]), ptr(case["indices"]),
                                     0 if case["indices"] is None else len(case["indices"]), ptr(dist2), int(case["start"]), None, ptr(stats2))
    _lib.check(rc, "snail_wide_trace")
    assert stats2.tolist() == [2 ** 40 + 5 + int(st[0]), 7 + int(st[1])] and np.array_equal(dist2.view(np.uint32), d.view(np.uint32))
    dist3 = case["dist"].copy()
    visits3 = np.full((len(dist3), 2), SENTINEL, dtype=np.int32)
    rc = _lib.lib().snail_wide_trace(sc._h, len(dist3), ptr(case["origin"]), ptr(case["dir"]), ptr(case["idir"]), ptr(case["indices"]),
                                     0 if case["indices"] is None else len(case["indices"]), ptr(dist3), int(case["start"]), ptr(visits3), None)
    _lib.check(rc, "snail_wide_trace")
    assert np.array_equal(visits3, v) and np.array_equal(dist3.view(np.uint32), d.view(np.uint32))


def test_the_host_form_with_more_entries_than_rays():
    """nIndices > nRays on host pointers: the staging buffers are sized by the list, not by the rays"""
    case, distinct = EC.dups()
    sc = dev_scene("box")
    dist = case["dist"].copy()
    sc.wide_trace_host(case["origin"], case["dir"], dist, indices=case["indices"])
    assert EC.same_floats(dist, EC.expected(dict(case, indices=distinct))[0])


@pytest.mark.parametrize("arith", ["ieee", "host_sse"])
def test_in_both_arithmetics(arith):
    """the walk is compiled once, outside the arithmetic namespaces: the scene's mode changes nothing"""
    for name in ("scaled_-38", "tiny_rays", "chain64_left", "half_outside"):
        case = EC.case(name)
        sc = dev_scene(case["scene"])
        sc.set_arith(arith)
        try:
            got = run(sc, case)
        finally:
            sc.set_arith("ieee")
        check(case, got, EC.expected(case))
