"""Two-level instanced scenes on the host: the library's top-level builder (snail_instances_build) against the test-side restatement
(tests/dbvh_ref.py), the validation of snail_instances_create / _build, and a self-check of the restatement's walk against the oracle."""
import ctypes as C

import numpy as np
import pytest

from snail_amd import _lib, scenes
from snail_amd.instances import build_instances
from tests import dbvh_ref as R
from tests import oracle_lib as O


def _field(n, seed, n_blas=1, bbox=((-1.0, -2.0, -0.5), (3.0, 1.0, 2.5))):
    rot, tr, bi = scenes.instance_field(bbox[0], bbox[1], n, seed=seed, n_blas=n_blas)
    xf = np.concatenate([rot.reshape(-1, 9), tr], axis=1).astype(np.float32)
    return xf, bi


def _boxes(n_blas, seed=3):
    rng = np.random.default_rng(seed)
    lo = rng.uniform(-3, 0, (n_blas, 3))
    return np.concatenate([lo, lo + rng.uniform(0.5, 4, (n_blas, 3))], axis=1).astype(np.float32)


def _check(xf, bi, bb):
    nodes, depth, perm = build_instances(xf, bi, bb)
    rn, rd, rp = R.build(xf, bi, bb)
    assert nodes.tobytes() == rn.tobytes()
    assert depth == rd
    assert np.array_equal(perm, rp)
    assert sorted(perm.tolist()) == list(range(len(xf)))
    return nodes, depth, perm


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 17, 1000])
def test_builder_matches_restatement(n):
    xf, bi = _field(n, seed=n)
    _check(xf, bi, _boxes(1))


def test_builder_several_blas_and_multi_instance_leaves():
    xf, bi = _field(300, seed=11, n_blas=3)
    _, _, _ = _check(xf, bi, _boxes(3))
    # the binned SAH never prefers a leaf of several instances (a split costs at most the leaf); such leaves come from a caller's tree
    # (the reference's own DBVH::nodes): one leaf holding every instance passes the validation
    one = np.zeros(1, dtype=R.NODE_DTYPE)
    one["sub"], one["aux"] = 0x80000000, 5
    assert "invalid scene handle" in _create(one, np.ascontiguousarray(xf[:5]), np.zeros(5, np.int32))


def test_builder_coincident_centres_take_the_median_split():
    xf = np.tile(np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1, 5, 5, 5]], np.float32), (13, 1))
    nodes, depth, perm = _check(xf, np.zeros(13, np.int32), _boxes(1))
    assert depth >= 3 and np.array_equal(perm, np.arange(13))


def test_builder_non_orthonormal_rotations():
    rng = np.random.default_rng(9)
    xf = rng.uniform(-3, 3, (64, 12)).astype(np.float32)
    _check(xf, (np.arange(64) % 2).astype(np.int32), _boxes(2))


def test_builder_rejects_bad_input():
    xf, bi = _field(10, seed=1)
    bad = xf.copy(); bad[3, 4] = np.nan
    with pytest.raises(_lib.SnailError):
        build_instances(bad, bi, _boxes(1))
    bad = xf.copy(); bad[0, 9] = np.inf
    with pytest.raises(_lib.SnailError):
        build_instances(bad, bi, _boxes(1))
    with pytest.raises(_lib.SnailError):
        build_instances(xf, np.full(10, 1, np.int32), _boxes(1))


def _create(nodes, xf, bi, depth=0):
    """snail_instances_create with no BLAS scene: validation of the tree comes first and needs no device; a tree that passes it
    fails later for the missing BLAS.  -> the error text."""
    L = _lib.lib()
    blas = (C.c_void_p * 1)(None)
    h = L.snail_instances_create(blas, 1, _lib.ptr(nodes), len(nodes), _lib.ptr(xf), _lib.ptr(bi), len(xf), depth)
    assert not h
    return L.snail_last_error().decode()


def test_create_rejects_malformed_trees():
    """snail_instances_create validates the tree before it looks at the BLAS handles (no device needed): a well-formed tree gets as far
    as the (here null) BLAS handle, every malformed one is refused for what is wrong with it."""
    xf, bi = _field(9, seed=4)
    nodes, depth, perm = build_instances(xf, bi, _boxes(1))
    xs, bs = np.ascontiguousarray(xf[perm]), np.ascontiguousarray(bi[perm])
    assert "invalid scene handle" in _create(nodes, xs, bs, depth)
    inner = np.nonzero((nodes["sub"] & 0x80000000) == 0)[0]
    leaf = np.nonzero((nodes["sub"] & 0x80000000) != 0)[0]
    bad = nodes.copy(); bad[inner[0]]["sub"] = len(nodes) - 1          # second child outside the array
    assert "children" in _create(bad, xs, bs)
    bad = nodes.copy(); bad[inner[-1]]["sub"] = 0                      # a child before its parent (a cycle)
    assert "children" in _create(bad, xs, bs)
    bad = nodes.copy(); bad[leaf[0]]["aux"] = 10                       # leaf range past the instances
    assert "leaf" in _create(bad, xs, bs)
    bad = nodes.copy(); bad[leaf[0]]["sub"] = 0x80000000 | 8; bad[leaf[0]]["aux"] = 2
    assert "leaf" in _create(bad, xs, bs)
    b2 = bs.copy(); b2[0] = 1
    assert "names BLAS" in _create(nodes, xs, b2)
    x2 = xs.copy(); x2[1, 2] = np.inf
    assert "non-finite" in _create(nodes, x2, bs)
    # a chain 65 levels deep: node 2k has children 2k+1 (a leaf) and 2k+2
    levels = 65
    chain = np.zeros(2 * levels + 1, dtype=nodes.dtype)
    chain["bmin"], chain["bmax"] = -1.0, 1.0
    for k in range(levels):
        chain[2 * k]["sub"] = 2 * k + 1
        chain[2 * k + 1]["sub"] = 0x80000000; chain[2 * k + 1]["aux"] = 1
    chain[2 * levels]["sub"] = 0x80000000; chain[2 * levels]["aux"] = 1
    one_x, one_b = np.ascontiguousarray(xs[:1]), np.zeros(1, np.int32)
    assert "deeper than 64" in _create(chain, one_x, one_b)


def test_restatement_identity_instance_equals_the_oracle():
    """dbvh_ref over ONE identity instance: hits (t, u, v, tri) bit-equal to OracleScene.render_primary; TreeStats = the oracle's plus
    exactly the top-level counts (one loop iteration per packet for the single leaf, Intersection(64) per packet whose box test passed)."""
    tv = scenes.box_scene()
    osc = O.OracleScene(tv)
    cam = np.asarray(__import__("snail_amd").survey_camera(tv).as_array13(), dtype=np.float32)
    ident = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]], np.float32)
    bb = np.concatenate([osc.nodes[0]["bmin"], osc.nodes[0]["bmax"]]).astype(np.float32).reshape(1, 6)
    nodes, depth, perm = R.build(ident, np.zeros(1, np.int32), bb)
    ref = R.Ref([osc], nodes, ident, np.zeros(1, np.int32))
    for mode in (O.MODE_IEEE, O.MODE_SSE):
        t, u, v, inst, tri, st = ref.render_primary(cam, 64, 48, mode=mode)
        ot, ou, ov, otid, ost = osc.render_primary(cam, 64, 48, mode=mode, threads=2)
        for a, b in ((t, ot), (u, ou), (v, ov)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert np.array_equal(tri, otid) and not inst.any()
        n_packets = 4 * 3
        extra = st - ost
        assert extra[1] == n_packets and extra[2] == 0 and extra[3] == 0
        assert 0 < extra[0] <= 64 * n_packets
        # per packet, exactly: the root leaf's BBox::Test (RayInterval first, src/dbvh/traverse.cpp:40-47) leaves a range [first, last];
        # when it is the whole packet, the inner walk is the oracle's own 64-quad walk, so the packet's TreeStats are the oracle's plus
        # LoopIteration 1 and Intersection 64; when the box is missed, the top level's one iteration stands for the BVH root's; a narrowed
        # range makes the inner RayGroup a count-quad packet (tree.h:62-63), whose counts are its own -- those packets are checked above only
        org = np.repeat(cam[:3].reshape(1, 3, 1), 4, axis=2).astype(np.float32)
        inf = np.full((64, 4), np.inf, dtype=np.float32)
        full = missed = 0
        for py in range(0, 48, 16):
            for px in range(0, 64, 16):
                dd, ii = O.gen_packet(cam, 64, 48, px, py, mode)
                d, idir = dd.reshape(64, 3, 4).copy(), ii.reshape(64, 3, 4).copy()
                mnD, mxD = R._minmax(d, [15] * 64, False)
                mnI, mxI = R._minmax(idir, [15] * 64, False)
                iv = {"minIDir": mnI, "maxIDir": mxI, "minOrg": list(cam[:3]), "maxOrg": list(cam[:3]), "minDir": mnD, "maxDir": mxD}
                r = R._box_test(nodes[0], org, idir, inf, 0, 63, True, False) if R._test_interval(nodes[0], iv) else None
                dist = inf.copy()
                pst = ref.traverse(org, d, idir, None, dist, np.zeros((64, 4), np.int32), np.zeros((64, 4), np.int32), np.zeros((64, 8), np.float32),
                                   True, False, mode)
                ost1 = osc.render_primary(cam, 64, 48, rect=(px, py, 16, 16), mode=mode, threads=1)[4]
                if r is None:
                    missed += 1
                    assert pst.tolist() == [0, 1, 0, ost1[3]] and ost1[0] == 0 and ost1[1] == 1
                elif r == (0, 63):
                    full += 1
                    assert pst.tolist() == [ost1[0] + 64, ost1[1] + 1, 0, ost1[3]]
        assert full > 0
