"""BVH::WideTrace with one ray per lane (include/snail_wide.h) against its NumPy restatement (tests/wide_ref.py) on the cases of
tests/wide_cases.py: distances equal on bits, per-ray visit counters equal, their sums in d_stats."""
import numpy as np
import pytest
import torch

from snail_amd import _lib, scenes
from snail_amd.scene import Scene
from tests import wide_cases as WC
from tests import wide_ref as WR

pytestmark = pytest.mark.gpu

SENTINEL = -7


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


_scenes = {}


def dev_scene(name):
    if name not in _scenes:
        _scenes[name] = Scene(WC.bvh(name), 0)
    return _scenes[name]


def run(sc, case, stream=None):
    """-> (dist, visits, stats) of one device call; the visits of rays that are not listed keep SENTINEL"""
    dev = sc._dev()
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    dist = up(case["dist"])
    visits = torch.full((len(case["dist"]), 2), SENTINEL, dtype=torch.int32, device=dev)
    stats = torch.zeros(2, dtype=torch.int64, device=dev)
    sc.wide_trace(up(case["origin"]), up(case["dir"]), dist, idir=up(case["idir"]), indices=up(case["indices"]), start_node=case["start"],
                  visits=visits, stats=stats, stream=stream)
    torch.cuda.synchronize()
    return dist.cpu().numpy(), visits.cpu().numpy(), stats.cpu().numpy()


def check(case, got, want):
    (d, v, st), (wd, wv) = got, want
    n = len(wd)
    listed = np.arange(n) if case["indices"] is None else np.asarray(case["indices"], dtype=np.int64)
    rest = np.setdiff1d(np.arange(n), listed)
    bad = np.flatnonzero(_bits(d) != _bits(wd))
    assert len(bad) == 0, (case["name"], bad[:8], d[bad[:8]], wd[bad[:8]])
    assert np.array_equal(v[listed], wv[listed]), (case["name"], np.flatnonzero((v[listed] != wv[listed]).any(axis=1))[:8])
    assert (v[rest] == SENTINEL).all() and np.array_equal(_bits(d[rest]), _bits(case["dist"][rest]))    # untouched rays keep their bytes
    assert st.tolist() == wv[listed].astype(np.int64).sum(axis=0).tolist(), case["name"]


@pytest.mark.parametrize("name", [c["name"] for c in WC.small_cases()])
def test_small_cases(name):
    case = [c for c in WC.small_cases() if c["name"] == name][0]
    check(case, run(dev_scene(case["scene"]), case), WC.expected(case))


def test_root_leaf_returns_negative_distances():
    case = WC.root_leaf()
    d, v, st = run(dev_scene("two"), case)
    assert (d < 0).sum() >= 2 and (v[:, 0] == 0).all() and st.tolist() == [0, 2 * len(d)]


def test_given_idir_equal_to_the_computed_one_gives_the_same_bytes():
    same, skew = WC.box_idir()
    null = dict(same, idir=None)
    a, b, c = run(dev_scene("box"), same), run(dev_scene("box"), null), run(dev_scene("box"), skew)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and not np.array_equal(a[1], c[1])


@pytest.fixture(scope="module")
def fuzz_ref():
    case = WC.fuzz()
    return case, WC.expected(case)


def test_fuzz_in_both_arithmetics(fuzz_ref):
    case, want = fuzz_ref
    sc = dev_scene("offgrid")
    got = run(sc, case)
    check(case, got, want)
    sc.set_arith("host_sse")
    try:
        sse = run(sc, case)
    finally:
        sc.set_arith("ieee")
    assert np.array_equal(_bits(got[0]), _bits(sse[0])) and np.array_equal(got[1], sse[1]) and np.array_equal(got[2], sse[2])
    # on a stream of its own, and the host form: the same bytes
    s = torch.cuda.Stream()
    again = run(sc, case, stream=s)
    assert np.array_equal(_bits(got[0]), _bits(again[0])) and np.array_equal(got[1], again[1])
    dist = case["dist"].copy()
    visits = np.full((len(dist), 2), SENTINEL, dtype=np.int32)
    st = sc.wide_trace_host(case["origin"], case["dir"], dist, visits=visits)
    assert np.array_equal(_bits(dist), _bits(want[0])) and np.array_equal(visits, want[1]) and st.tolist() == got[2].tolist()


def test_fuzz_on_a_fast_dev_handle_after_a_rebuild():
    """the committed tree of snail_scene_create_fast_dev: built, rebuilt from moved vertices, then walked; expected from the tree read back"""
    case = WC.fuzz()
    tv = WC.verts("offgrid").reshape(-1, 9)
    d_verts = torch.from_numpy(tv).cuda()
    sc = Scene.from_fast_dev(d_verts, 0)
    moved = torch.from_numpy((tv + np.float32(0.125)).astype(np.float32)).cuda()
    info = sc.rebuild_fast_dev(moved)
    got = run(sc, case)
    assert info.cpu().numpy()[0] == 0
    b = sc.bvh
    want = WR.wide_trace(b.nodes, b.tris, case["origin"], case["dir"], case["dist"])
    check(case, got, want)
    assert np.isfinite(got[0]).sum() > 100
    sc.close()


def test_lbvh_handle():
    case = WC.box_sizes()[4]
    sc = Scene.from_lbvh(scenes.box_scene(), 0)
    b = sc.bvh
    check(case, run(sc, case), WR.wide_trace(b.nodes, b.tris, case["origin"], case["dir"], case["dist"]))
    sc.close()


def test_refusals_that_need_the_handle():
    sc = dev_scene("box")
    dev = sc._dev()
    o = torch.zeros((4, 3), dtype=torch.float32, device=dev)
    dist = torch.full((4,), 3.5, dtype=torch.float32, device=dev)
    with pytest.raises(_lib.SnailError, match="startNode 9 outside the tree"):
        sc.wide_trace(o, o, dist, start_node=len(WC.bvh("box").nodes))
    with pytest.raises(_lib.SnailError, match="startNode -1 outside the tree"):
        sc.wide_trace(o, o, dist, start_node=-1)
    with pytest.raises(ValueError, match="3 values per ray"):
        sc.wide_trace(o[:3], o, dist)
    # ray numbers outside the arrays name no ray; an empty list does nothing
    idx = torch.tensor([7, -1, 2], dtype=torch.int32, device=dev)
    d = torch.ones((4, 3), dtype=torch.float32, device=dev)
    sc.wide_trace(o, d, dist, indices=idx)
    sc.wide_trace(o, d, dist, indices=idx[:0])
    torch.cuda.synchronize()
    got = dist.cpu().numpy()
    assert (got[[0, 1, 3]] == 3.5).all()
