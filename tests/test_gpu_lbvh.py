"""The device LBVH builder (snail_scene_create_lbvh, snail_amd/csrc/lbvh.inc) held to tests/lbvh_ref.py byte for byte -- every node slot,
unused ones included, perm, depth, triangle records -- on the cases of tests/lbvh_cases.py (tests/test_lbvh_ref_host.py shows what each is
for); its flags held to what snail_scene_create reports for the same arrays; and every walk the product has, in both arithmetics, over LBVH
trees with unused slots, leaves of up to 64 triangles, 39 levels and a single Morton cell, against the oracle over the downloaded tree.
All comparisons are bitwise."""
import ctypes as C

import numpy as np
import pytest

from tests import dbvh_ref as D
from tests import lbvh_cases as K
from tests import lbvh_ref as R
from tests import oracle_lib as O
from tests import util as U

pytestmark = pytest.mark.gpu
ARITH = [("ieee", O.MODE_IEEE), ("host_sse", O.MODE_SSE)]
RES = (128, 96)


def lbvh_scene(tv, max_leaf):
    from snail_amd.scene import Scene
    return Scene.from_lbvh(np.ascontiguousarray(tv, np.float32), 0, max_leaf_tris=max_leaf)


def scene_info(sc):
    """(nNodes, nTris, depth) as the handle reports them"""
    from snail_amd import _lib
    nn, nt, depth, dev = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
    _lib.check(_lib.lib().snail_scene_info(sc._h, C.addressof(nn), C.addressof(nt), C.addressof(depth), C.addressof(dev)), "snail_scene_info")
    return nn.value, nt.value, depth.value


def assert_flags_equal_the_reuploads(sc, what=""):
    """the download, re-uploaded through snail_scene_create, is a scene with the same flags and the same depth"""
    from snail_amd.scene import Scene
    again = Scene(sc.bvh, 0)
    try:
        assert sc.flags() == again.flags(), (what, "flags", sc.flags(), again.flags())
        assert sc.depth == scene_info(sc)[2] == scene_info(again)[2], (what, "depth", sc.depth, scene_info(again))
    finally:
        again.close()
    return sc.flags()


def assert_is_the_restatement(sc, tv, max_leaf, want, what=""):
    from snail_amd import HostBVH
    tv = np.ascontiguousarray(tv, np.float32).reshape(-1, 9)
    R.assert_same_tree((sc.bvh.nodes, sc.perm, sc.depth), want, what)
    assert sc.bvh.tris.tobytes() == HostBVH.triangles(tv[sc.perm]).tobytes(), (what, "triangle records")
    R.check_tree(sc.bvh.nodes, sc.bvh.tris, sc.perm, tv, max_leaf, sc.depth)


# ---- 1 + 5: byte equality and flags ----
@pytest.mark.parametrize("name,max_leaf", K.ALL)
def test_device_tree_is_byte_equal_to_the_restatement(name, max_leaf):
    tv = K.verts(name)
    sc = lbvh_scene(tv, max_leaf)
    try:
        if name == "comb":
            print("comb at max_leaf %d: device depth %d, restated depth %d" % (max_leaf, sc.depth, K.ref(name, max_leaf)[2]))
        assert_is_the_restatement(sc, tv, max_leaf, K.ref(name, max_leaf), "%s/%d" % (name, max_leaf))
        nodes, perm, _ = K.ref(name, max_leaf)
        fast_ok, nested_ok = assert_flags_equal_the_reuploads(sc, name)
        assert nested_ok and fast_ok == R.fast_ok(nodes, R.tri_records(tv[perm]))
        assert sc.build_ms > 0.0
    finally:
        sc.close()


# ---- 2: determinism ----
@pytest.mark.parametrize("name,max_leaf", [("soup5003", 4), ("comb", 1)])
def test_two_builds_are_byte_equal(name, max_leaf):
    a, b = lbvh_scene(K.verts(name), max_leaf), lbvh_scene(K.verts(name), max_leaf)
    try:
        assert a.bvh.nodes.tobytes() == b.bvh.nodes.tobytes() and a.bvh.tris.tobytes() == b.bvh.tris.tobytes()
        assert np.array_equal(a.perm, b.perm) and a.depth == b.depth and a.flags() == b.flags()
    finally:
        a.close(); b.close()


# ---- 3: the optional outputs ----
def test_perm_and_build_ms_are_optional():
    from snail_amd import _lib
    from snail_amd.bvh import NODE_DTYPE, TRI_DTYPE
    L = _lib.lib()
    tv = np.ascontiguousarray(K.verts("soup257"))
    got = []
    for with_outputs in (False, True):
        perm, ms = np.full(len(tv), -7, np.int32), C.c_float(-1.0)
        h = L.snail_scene_create_lbvh(_lib.ptr(tv), len(tv), 0, 4, _lib.ptr(perm) if with_outputs else None, C.addressof(ms) if with_outputs else None)
        assert h, L.snail_last_error().decode()
        h = C.c_void_p(h)
        try:
            nn, nt, depth, dev = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
            _lib.check(L.snail_scene_info(h, C.addressof(nn), C.addressof(nt), C.addressof(depth), C.addressof(dev)), "snail_scene_info")
            nodes, tris = np.zeros(nn.value, NODE_DTYPE), np.zeros(nt.value, TRI_DTYPE)
            _lib.check(L.snail_scene_download(h, _lib.ptr(nodes), _lib.ptr(tris)), "snail_scene_download")
            got.append((nodes.tobytes(), tris.tobytes(), depth.value, nn.value, nt.value))
        finally:
            L.snail_scene_destroy(h)
        if with_outputs:
            assert np.array_equal(perm, K.ref("soup257", 4)[1]) and ms.value > 0.0
        else:
            assert (perm == -7).all() and ms.value == -1.0
    assert got[0] == got[1] and got[0][3:] == (2 * len(tv) - 1, len(tv))


# ---- 4: the walks ----
_walk = {}


def walk_scene(name, max_leaf):
    if (name, max_leaf) not in _walk:
        sc = lbvh_scene(K.verts(name), max_leaf)
        hb = sc.bvh
        _walk[(name, max_leaf)] = dict(sc=sc, osc=O.OracleScene.from_arrays(hb.tris, hb.nodes, hb.depth, sc.perm), region=K.Region(name))
    return _walk[(name, max_leaf)]


def test_walk_trees_are_the_restatement_and_what_they_are_for():
    for name, max_leaf in K.WALK_TREES:
        W = walk_scene(name, max_leaf)
        assert_is_the_restatement(W["sc"], K.verts(name), max_leaf, K.ref(name, max_leaf), name)
        assert_flags_equal_the_reuploads(W["sc"], name)
    nodes = walk_scene("soup1025", 64)["sc"].bvh.nodes
    leaf = (nodes["sub"] & 0x80000000) != 0
    assert 32 < nodes["aux"][leaf].max() <= 64 and (leaf & (nodes["aux"] == 0)).sum() > 1000          # big leaves, unused slots
    assert walk_scene("comb", 1)["sc"].depth >= 36


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("name,max_leaf", K.WALK_TREES)
def test_primary_frame_equals_the_oracle(name, max_leaf, arith, mode):
    import torch
    W = walk_scene(name, max_leaf)
    sc, osc, cam = W["sc"], W["osc"], W["region"].camera()
    sc.set_arith(arith)
    try:
        stats = sc.new_stats()
        f = sc.trace_primary(cam, *RES, stats=stats)
        torch.cuda.synchronize()
        t, u, v, tid, ost = osc.render_primary(cam.as_array13(), *RES, mode=mode, threads=4)
        for a, b, n in ((f.t, t, "t"), (f.u, u, "u"), (f.v, v, "v"), (f.tri_id, tid, "triId")):
            U.assert_bit_equal(a.cpu().numpy(), b, n)
        assert np.array_equal(stats.cpu().numpy().astype(np.uint64), ost), "TreeStats"
        assert np.isfinite(t).sum() > 100 and np.isinf(t).sum() > 100          # hits and misses both occur
    finally:
        sc.set_arith("ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("name,max_leaf", K.WALK_TREES)
def test_shadow_packets_and_the_lit_frame_equal_the_oracle(name, max_leaf, arith, mode):
    import torch
    W = walk_scene(name, max_leaf)
    sc, osc, rg = W["sc"], W["osc"], W["region"]
    cam = rg.camera()
    sc.set_arith(arith)
    try:
        npk = 16
        origin, dirs, idir, dist = U.shadow_packets(rg, npk, seed=5, size=64)
        want = dist.copy()
        wst = osc.trace_shadow(origin, dirs, idir, want, npk, 64, mode=mode)
        got = dist.copy()
        st = np.asarray(sc.trace_shadow_host(origin, dirs, idir, got, npk, 64)).astype(np.uint64)
        U.assert_bit_equal(got, want, "shadow distance")
        assert st[0] == wst[0] and st[1] == wst[1] and st[3] == wst[3], (st, wst)      # intersects, iters, skips (rays are counted by the caller)
        assert (np.isneginf(want) & ~np.isneginf(dist)).any() and (~np.isneginf(want)).any()      # occluded and lit rays both occur
        lights = rg.light()
        wimg, wst = osc.render_whitted(cam.as_array13(), *RES, lights, mode=mode, threads=4)
        stats = sc.new_stats()
        img = sc.render_whitted(cam, *RES, lights, stats=stats).cpu().numpy()
        torch.cuda.synchronize()
        assert np.array_equal(img, wimg), int((img != wimg).sum())
        assert np.array_equal(stats.cpu().numpy().astype(np.uint64), wst), "TreeStats"
        assert len(np.unique(wimg.reshape(-1, 3), axis=0)) >= 3          # background, shaded and lit pixels
    finally:
        sc.set_arith("ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("shared", [True, False], ids=["shared_origin", "per_ray_origins"])
@pytest.mark.parametrize("name,max_leaf", K.WALK_TREES)
def test_generic_packets_equal_the_oracle(name, max_leaf, shared, arith, mode):
    W = walk_scene(name, max_leaf)
    sc, osc, rg = W["sc"], W["osc"], W["region"]
    sc.set_arith(arith)
    try:
        npk = 16
        origin, dirs, idir, mask, dist, obj, bary = U.secondary_packets(rg, rg.camera(), *RES, npk, seed=21, shared=shared, masked=not shared, size=64)
        d2, o2, b2 = dist.copy(), obj.copy(), bary.copy()
        wst = osc.trace_rays(origin, dirs, idir, mask, d2, o2, b2, npk, 64, shared, mode=mode)
        d3, o3, b3 = dist.copy(), obj.copy(), bary.copy()
        st = np.asarray(sc.trace_rays_host(origin, dirs, idir, mask, d3, o3, b3, npk, 64, shared)).astype(np.uint64)
        U.assert_bit_equal(d3, d2, "t"); U.assert_bit_equal(o3, o2, "triId"); U.assert_bit_equal(b3, b2, "barycentric")
        assert st[0] == wst[0] and st[1] == wst[1], (st, wst)
        # hits occur (triId 0 is a hit's id too where every triangle is the same one: the distance tells) and so do misses
        assert np.isfinite(d2).any() and np.isposinf(d2).any() and wst[0] > 0
        assert name == "identical300" or (o2 != 0).any()
    finally:
        sc.set_arith("ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
def test_instanced_frame_over_an_lbvh_blas_equals_the_restatement(arith, mode):
    """one instanced frame whose first BLAS is the LBVH handle of soup1025 at 64 triangles per leaf, beside a host-built box, against
    tests/dbvh_ref.py over the downloaded tree"""
    import torch
    from snail_amd import HostBVH, scenes, survey_camera
    from snail_amd.instances import InstancedScene
    from snail_amd.scene import Scene
    from tests.test_bvh_fast_host import fixture
    W = walk_scene("soup1025", 64)
    lb = W["sc"]
    box_tv = fixture("box")
    box = Scene(HostBVH.build(box_tv), 0)
    osc = [W["osc"], O.OracleScene(box_tv)]
    lo = np.minimum(osc[0].nodes[0]["bmin"], osc[1].nodes[0]["bmin"])
    hi = np.maximum(osc[0].nodes[0]["bmax"], osc[1].nodes[0]["bmax"])
    rot, tr, bi = scenes.instance_field(lo, hi, 12, seed=3, n_blas=2)
    tr = (tr * np.float32(0.1)).astype(np.float32)
    isc = InstancedScene([lb, box], rot, tr, bi)
    for s in isc.blas:
        s.set_arith(arith)
    try:
        xs, bs = isc.slot_transforms()
        ref = D.Ref(osc, isc.nodes(), xs, bs)
        nd = isc.nodes()[0]
        cam = survey_camera(np.concatenate([nd["bmin"], nd["bmax"], nd["bmin"]]).reshape(1, 9))
        st = isc.new_stats()
        t, u, v, inst, tri = isc.trace_primary(cam, 96, 64, stats=st)
        rt, ru, rv, rinst, rtri, rst = ref.render_primary(cam.as_array13(), 96, 64, mode=mode)
        torch.cuda.synchronize()
        for a, b, what in ((t, rt, "t"), (u, ru, "u"), (v, rv, "v")):
            U.assert_bit_equal(a.cpu().numpy(), b, what)
        assert np.array_equal(inst.cpu().numpy(), rinst) and np.array_equal(tri.cpu().numpy(), rtri)
        assert np.array_equal(st.cpu().numpy().astype(np.uint64), rst), (st.cpu().numpy(), rst)
        hit = np.isfinite(rt)
        assert hit.sum() > 20 and (np.asarray(bs)[rinst[hit]] == 0).any()      # the LBVH BLAS is hit
    finally:
        for s in isc.blas:
            s.set_arith("ieee")
        isc.close(); box.close()


# ---- 5: flags ----
@pytest.mark.parametrize("copies,max_leaf", [(1, 4), (2, 4), (5, 1)], ids=["single_triangle", "root_leaf", "inner_nodes"])
def test_a_box_beyond_1e9_clears_fastok_on_every_path(copies, max_leaf):
    """Every field of the triangle's record is within the limits the fast arithmetic modes need, its box maximum (1.7e9) is not.
    snail_scene_create refuses fastOK for such a node; the builder must say the same whether the box is written by the single-triangle
    path, the root-leaf path or the inner branch of k_emit."""
    tv = np.tile(K.magnitude_tri(), (copies, 1))
    rec = R.tri_records(tv).view(np.float32).reshape(-1, 16)
    assert (np.abs(rec[:, :9]) <= 1e9).all() and (rec[:, 9] > 0).all() and tv.max() > 1e9
    sc = lbvh_scene(tv, max_leaf)
    try:
        assert_is_the_restatement(sc, tv, max_leaf, R.build(tv, max_leaf), "magnitude x%d" % copies)
        flags = sc.flags()
        print("magnitude case, %d triangle(s), max_leaf %d: fastOK = %d" % (copies, max_leaf, flags[0]))
        assert assert_flags_equal_the_reuploads(sc) == (False, True) and flags == (False, True)
    finally:
        sc.close()


def frame_equals_the_oracle(sc, cam, mode=O.MODE_IEEE):
    import torch
    osc = O.OracleScene.from_arrays(sc.bvh.tris, sc.bvh.nodes, sc.depth, sc.perm)
    stats = sc.new_stats()
    f = sc.trace_primary(cam, *RES, stats=stats)
    torch.cuda.synchronize()
    t, u, v, tid, ost = osc.render_primary(cam.as_array13(), *RES, mode=mode, threads=4)
    for a, b, n in ((f.t, t, "t"), (f.u, u, "u"), (f.v, v, "v"), (f.tri_id, tid, "triId")):
        U.assert_bit_equal(a.cpu().numpy(), b, n)
    assert np.array_equal(stats.cpu().numpy().astype(np.uint64), ost), "TreeStats"
    assert np.isfinite(t).sum() > 200


def test_a_zero_area_triangle_clears_fastok_and_the_frame_is_the_oracles():
    from snail_amd import survey_camera
    tv = K.zero_area_soup()
    sc = lbvh_scene(tv, 4)
    try:
        assert_is_the_restatement(sc, tv, 4, R.build(tv, 4), "zero area")
        assert assert_flags_equal_the_reuploads(sc) == (False, True)
        frame_equals_the_oracle(sc, survey_camera(tv))
    finally:
        sc.close()


# ---- 6: non-finite vertices ----
@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_non_finite_vertex_gives_a_handle_without_fastok(value):
    """fminf / fmaxf drop a NaN from boxes and bounds, an infinite coordinate makes one axis of the scene infinite (every centre in cell
    0 there): either way a handle comes back, it is the restated tree, fastOK is 0 as after a re-upload, and the frame is the oracle's walk
    of the downloaded tree (tests/test_lbvh_ref_host.py shows the oracle renders such a tree)."""
    from snail_amd import survey_camera
    tv = K.nonfinite_soup(value)
    sc = lbvh_scene(tv, 4)
    try:
        R.assert_same_tree((sc.bvh.nodes, sc.perm, sc.depth), R.build(tv, 4), "non-finite")
        got, want = (np.ascontiguousarray(x).view(np.uint32).reshape(-1, 16) for x in (sc.bvh.tris, R.tri_records(tv[sc.perm])))
        nan = np.isnan(want.view(np.float32))          # (which NaN an invalid operation gives is the processor's choice)
        assert np.array_equal(np.isnan(got.view(np.float32)), nan) and np.array_equal(got[~nan], want[~nan]) and nan.any(axis=1).sum() == 1
        flags = sc.flags()
        print("non-finite vertex %r: flags %r" % (value, flags))
        assert assert_flags_equal_the_reuploads(sc) == (False, True)
        frame_equals_the_oracle(sc, survey_camera(K.nonfinite_soup(np.float32(0.0))))
    finally:
        sc.close()

