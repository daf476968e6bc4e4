"""The top-level tree rebuilt on the device (snail_instances_rebuild_dev / InstancedScene.update_dev, include/snail_instances_build.h)
against the HOST builder on the same inputs (snail_instances_build, pinned to tests/dbvh_ref.py by tests/test_instances_host.py): node
bytes, node count, depth, element order and slot records equal, and the frames rendered after it equal the host-updated scene's.

Size classes of the kernels (snail_amd/csrc/instances_build.inc): n == 1 (the root is a leaf), 2..64 (the root goes straight to the
one-wave subtree kernel), > 64 (workgroup-per-node levels first; 65 is the smallest, 5003 takes six such levels and hundreds of small
subtrees)."""
import ctypes as C

import numpy as np
import pytest

from snail_amd import HostBVH, _lib, scenes, survey_camera
from snail_amd.instances import InstancedScene, build_instances
from snail_amd.scene import Scene

pytestmark = pytest.mark.gpu

UNIT = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 1], [1, 1, 1, 0, 1, 0, 1, 0, 1]], np.float32)      # a BLAS whose root box is exactly [0, 1]^3


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_cache = {}


def blas_list(kind):
    """device Scenes: "box" = the box scene alone; "three" = it and two scaled / shifted copies (three different root boxes);
    "unit" = two triangles spanning [0, 1]^3"""
    if kind not in _cache:
        tv = scenes.box_scene()
        if kind == "box":
            tvs = [tv]
        elif kind == "three":
            tvs = [tv, (tv * np.float32(0.5) + np.float32(1.25)).astype(np.float32), (tv * np.float32(1.75) - np.float32(0.5)).astype(np.float32)]
        else:
            tvs = [UNIT]
        _cache[kind] = [Scene(HostBVH.build(t), 0) for t in tvs]
    return _cache[kind]


def bboxes(blas):
    return np.stack([np.concatenate(s.get_bbox()) for s in blas]).astype(np.float32)


def field(blas, n, seed):
    bb = bboxes(blas)
    rot, tr, bi = scenes.instance_field(bb[:, :3].min(axis=0), bb[:, 3:].max(axis=0), n, seed=seed, n_blas=len(blas))
    return np.ascontiguousarray(np.concatenate([rot.reshape(-1, 9), tr], axis=1), dtype=np.float32), bi


_seed_scene = {}


def scene_of(kind):
    """one handle per BLAS list, reused by the cases (every case rebuilds it)"""
    if kind not in _seed_scene:
        blas = blas_list(kind)
        xf, bi = field(blas, 5, seed=77)
        _seed_scene[kind] = InstancedScene(blas, xf[:, :9], xf[:, 9:], bi)
    return _seed_scene[kind]


def read_tree(isc):
    L = _lib.lib()
    nn, n = C.c_int(0), C.c_int(0)
    _lib.check(L.snail_instances_read_tree(isc._h, None, 0, C.addressof(nn), None, None, 0, C.addressof(n)), "snail_instances_read_tree")
    nodes = np.zeros(nn.value, dtype=isc._nodes.dtype)
    xf = np.zeros((n.value, 12), np.float32)
    bi = np.zeros(n.value, np.int32)
    _lib.check(L.snail_instances_read_tree(isc._h, _lib.ptr(nodes), len(nodes), None, _lib.ptr(xf), _lib.ptr(bi), len(xf), None), "snail_instances_read_tree")
    return nodes, xf, bi


def check_rebuild(torch, isc, xf, bi):
    """update_dev on (xf, bi) against snail_instances_build on the same arrays"""
    xf = np.ascontiguousarray(xf, dtype=np.float32)
    bi = np.ascontiguousarray(bi, dtype=np.int32)
    want_nodes, want_depth, want_perm = build_instances(xf, bi, bboxes(isc.blas))
    d = torch.device("cuda", isc.device)
    perm, info = isc.update_dev(torch.from_numpy(xf).to(d), torch.from_numpy(bi).to(d))
    nodes, xs, bs = read_tree(isc)
    info = info.cpu().numpy()
    assert info[0] == 0, info
    assert info[1] == len(want_nodes) and len(nodes) == len(want_nodes), (info, len(want_nodes))
    assert info[2] == want_depth and info[3] == len(xf), (info, want_depth)
    assert nodes.tobytes() == want_nodes.tobytes(), "node %d differs" % int(np.nonzero(nodes != want_nodes)[0][0])
    assert np.array_equal(perm.cpu().numpy(), want_perm)
    assert xs.tobytes() == xf[want_perm].tobytes() and bs.tobytes() == bi[want_perm].tobytes()
    # the Python object serves the same, refreshed
    assert isc.nodes().tobytes() == want_nodes.tobytes() and isc.depth == want_depth and np.array_equal(isc.perm(), want_perm)
    assert isc.slot_transforms()[0].tobytes() == xf[want_perm].tobytes()
    return want_nodes, want_depth, want_perm


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 17, 63, 64, 65, 1000, 5003])
def test_plain_fields(torch_mod, n):
    blas = blas_list("box")
    xf, bi = field(blas, n, seed=n)
    check_rebuild(torch_mod, scene_of("box"), xf, bi)


def test_three_blas_field(torch_mod):
    blas = blas_list("three")
    xf, bi = field(blas, 300, seed=11)
    assert len(set(bi.tolist())) == 3
    check_rebuild(torch_mod, scene_of("three"), xf, bi)


def test_blas_index_none_is_all_zero(torch_mod):
    isc = scene_of("three")
    xf, _ = field(isc.blas, 40, seed=5)
    want_nodes, _, want_perm = build_instances(xf, np.zeros(40, np.int32), bboxes(isc.blas))
    perm, info = isc.update_dev(torch_mod.from_numpy(xf).cuda())
    nodes, xs, bs = read_tree(isc)
    assert info.cpu().numpy()[0] == 0 and nodes.tobytes() == want_nodes.tobytes() and np.array_equal(perm.cpu().numpy(), want_perm) and not bs.any()


def test_coincident_centres_and_non_orthonormal(torch_mod):
    xf = np.tile(np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1, 5, 5, 5]], np.float32), (13, 1))
    _, depth, perm = check_rebuild(torch_mod, scene_of("box"), xf, np.zeros(13, np.int32))
    assert depth >= 3 and np.array_equal(perm, np.arange(13))       # median splits, nothing moved
    rng = np.random.default_rng(9)
    xf = rng.uniform(-3, 3, (64, 12)).astype(np.float32)
    check_rebuild(torch_mod, scene_of("three"), xf, (np.arange(64) % 2).astype(np.int32))


def signed_zero_field(n=24, seed=21):
    """axis-aligned rotations whose entries are +-1 and +-0, translations +-0, over the [0, 1]^3 BLAS: products and sums give +0 and -0
    bounds on the faces where the instances meet"""
    rng = np.random.default_rng(seed)
    xf = np.zeros((n, 12), np.float32)
    for i in range(n):
        p = rng.permutation(3)
        for r in range(3):
            row = np.where(rng.random(3) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
            row[p[r]] = rng.choice([-1.0, 1.0])
            xf[i, r * 3:r * 3 + 3] = row
        xf[i, 9:] = np.where(rng.random(3) < 0.5, np.float32(0.0), np.float32(-0.0))
    return xf


def test_signed_zeros(torch_mod):
    isc = scene_of("unit")
    assert np.array_equal(bboxes(isc.blas), np.array([[0, 0, 0, 1, 1, 1]], np.float32))
    xf = signed_zero_field()
    bi = np.zeros(len(xf), np.int32)
    nodes, _, _ = build_instances(xf, bi, bboxes(isc.blas))
    bits = np.concatenate([nodes["bmin"].ravel(), nodes["bmax"].ravel()]).view(np.uint32)
    assert (bits == 0x80000000).any() and (bits == 0).any(), "the case must hold -0 and +0 bounds to prove anything"
    check_rebuild(torch_mod, isc, xf, bi)
    check_rebuild(torch_mod, isc, xf[::-1].copy(), bi)


def box_sa(nodes):
    F = np.float32
    w, h, d = ((nodes["bmax"][:, k] - nodes["bmin"][:, k]).astype(F) for k in range(3))
    return ((w * (d + h)).astype(F) + (d * h).astype(F)).astype(F) * F(2.0)


def test_denormal_areas(torch_mod):
    isc = scene_of("box")
    xf, bi = field(isc.blas, 200, seed=31)
    xf = (xf * np.float32(1e-20)).astype(np.float32)
    nodes, _, _ = build_instances(xf, bi, bboxes(isc.blas))
    with np.errstate(all="ignore"):
        sa = box_sa(nodes)
    assert ((sa > 0) & (sa < np.float32(1.1754944e-38))).any(), "no BoxSA of the host computation is denormal"
    check_rebuild(torch_mod, isc, xf, bi)


def test_shrink_and_grow(torch_mod):
    blas = blas_list("box")
    xf0, bi0 = field(blas, 5, seed=1)
    isc = InstancedScene(blas, xf0[:, :9], xf0[:, 9:], bi0)      # a handle of its own: its buffers grow from 5 instances
    for n in (300, 17, 1000):
        xf, bi = field(blas, n, seed=100 + n)
        check_rebuild(torch_mod, isc, xf, bi)
    isc.close()


def frames_equal(a, b):
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


@pytest.mark.parametrize("second_stream", [False, True])
def test_ordering_without_host_waits(torch_mod, second_stream):
    torch = torch_mod
    blas = blas_list("box")
    xf1, bi1 = field(blas, 40, seed=3)
    xf2, bi2 = field(blas, 90, seed=4)
    host1 = InstancedScene(blas, xf1[:, :9], xf1[:, 9:], bi1)
    host2 = InstancedScene(blas, xf2[:, :9], xf2[:, 9:], bi2)
    isc = InstancedScene(blas, xf1[:, :9], xf1[:, 9:], bi1)
    # warm the handle: its buffers and the builder's scratch grow (and wait for the device) on the first rebuild of this size only, and
    # the first update_dev after an update() seeds the scene's device copy of perm; then back to the 40-instance tree
    warm, _ = field(blas, 90, seed=5)
    isc.update_dev(torch.from_numpy(warm).cuda())
    isc.update(xf1[:, :9], xf1[:, 9:], bi1)
    isc.update_dev(torch.from_numpy(xf1).cuda(), torch.from_numpy(bi1).cuda())
    assert isc.nodes().tobytes() == host1.nodes().tobytes()
    nd = host1.nodes()[0]
    cam = survey_camera(np.concatenate([nd["bmin"], nd["bmax"], nd["bmin"]]).reshape(1, 9))
    d_xf, d_bi = torch.from_numpy(xf2).cuda(), torch.from_numpy(bi2).cuda()
    side = torch.cuda.Stream() if second_stream else None
    torch.cuda.synchronize()
    st_a, st_b = isc.new_stats(), isc.new_stats()
    torch.cuda.synchronize()
    a = isc.trace_primary(cam, 64, 48, stats=st_a)
    isc.update_dev(d_xf, d_bi, stream=side)
    b = isc.trace_primary(cam, 64, 48, stats=st_b)
    torch.cuda.synchronize()
    w_a, w_b = host1.new_stats(), host2.new_stats()
    frames_equal(a, host1.trace_primary(cam, 64, 48, stats=w_a))
    frames_equal(b, host2.trace_primary(cam, 64, 48, stats=w_b))
    torch.cuda.synchronize()
    assert np.array_equal(st_a.cpu().numpy(), w_a.cpu().numpy()) and np.array_equal(st_b.cpu().numpy(), w_b.cpu().numpy())
    assert np.isfinite(b[0].cpu().numpy()).sum() > 20 and a[0].cpu().numpy().tobytes() != b[0].cpu().numpy().tobytes()
    if not second_stream:
        nd2 = host2.nodes()[0]
        c, ext = (nd2["bmin"] + nd2["bmax"]) * 0.5, nd2["bmax"] - nd2["bmin"]
        light = np.array([[c[0], c[1] + 0.3 * ext[1], c[2], 1.0, 1.0, 1.0, float(np.linalg.norm(ext))]], dtype=np.float32)
        lit, want = isc.render_whitted(cam, 64, 48, light), host2.render_whitted(cam, 64, 48, light)
        torch.cuda.synchronize()
        assert lit.cpu().numpy().tobytes() == want.cpu().numpy().tobytes() and lit.cpu().numpy().any()
        tiles = np.array([[0, 0, 16, 48], [16, 0, 48, 32]], np.int32)
        got_t, want_t = isc.render_tiles_host(cam, 64, 48, tiles, light), host2.render_tiles_host(cam, 64, 48, tiles, light)
        assert np.asarray(got_t[0]).tobytes() == np.asarray(want_t[0]).tobytes()
    for s in (isc, host1, host2):
        s.close()


def test_status_1_leaves_the_handle_untouched(torch_mod):
    torch = torch_mod
    blas = blas_list("three")
    xf, bi = field(blas, 30, seed=8)
    isc = InstancedScene(blas, xf[:, :9], xf[:, 9:], bi)
    nd = isc.nodes()[0]
    cam = survey_camera(np.concatenate([nd["bmin"], nd["bmax"], nd["bmin"]]).reshape(1, 9))
    before = read_tree(isc)
    frame = [x.cpu().numpy().copy() for x in isc.trace_primary(cam, 64, 48)]
    depth, perm0 = isc.depth, isc.perm()
    xf2, bi2 = field(blas, 50, seed=9)
    bad_nan = xf2.copy(); bad_nan[7, 4] = np.nan
    bad_inf = xf2.copy(); bad_inf[49, 11] = -np.inf
    bi_hi = bi2.copy(); bi_hi[3] = len(blas)
    bi_lo = bi2.copy(); bi_lo[20] = -1
    bi_far = bi2.copy(); bi_far[0] = 0x7fffffff
    for x, b in ((bad_nan, bi2), (bad_inf, bi2), (xf2, bi_hi), (xf2, bi_lo), (xf2, bi_far)):
        _, info = isc.update_dev(torch.from_numpy(x).cuda(), torch.from_numpy(b).cuda())
        assert info.cpu().numpy()[0] == 1, info
        after = read_tree(isc)
        assert all(p.tobytes() == q.tobytes() for p, q in zip(before, after))
        again = isc.trace_primary(cam, 64, 48)
        assert all(p.tobytes() == q.cpu().numpy().tobytes() for p, q in zip(frame, again))
        assert isc.depth == depth and np.array_equal(isc.perm(), perm0) and isc.nodes().tobytes() == before[0].tobytes()
    check_rebuild(torch, isc, xf2, bi2)         # and the handle still rebuilds
    isc.close()


def test_a_refused_rebuild_behind_a_good_one_with_one_info_tensor(torch_mod):
    """the caller reuses one info tensor: after good, refused the scene describes the good tree, not the one before both"""
    torch = torch_mod
    isc = scene_of("box")
    xf, bi = field(isc.blas, 70, seed=41)
    bad = xf.copy(); bad[5, 0] = np.inf
    want_nodes, want_depth, want_perm = build_instances(xf, bi, bboxes(isc.blas))
    info = torch.zeros(4, dtype=torch.int32, device="cuda")
    d_bi = torch.from_numpy(bi).cuda()
    good_x, bad_x = torch.from_numpy(xf).cuda(), torch.from_numpy(bad).cuda()
    isc.update_dev(good_x, d_bi, info=info)
    for _ in range(3):
        isc.update_dev(bad_x, d_bi, info=info)
    assert info.cpu().numpy()[0] == 1
    assert isc.nodes().tobytes() == want_nodes.tobytes() and isc.depth == want_depth and np.array_equal(isc.perm(), want_perm)
    assert isc.slot_transforms()[0].tobytes() == xf[want_perm].tobytes()
    # a caller's perm tensor receives the copy
    mine = torch.full((70,), -1, dtype=torch.int32, device="cuda")
    got, _ = isc.update_dev(good_x, d_bi, perm=mine)
    torch.cuda.synchronize()
    assert got is mine and np.array_equal(mine.cpu().numpy(), want_perm)


def deep_chain(k):
    """k point instances (zero rotation) at 2^(-149 + 4 i) on x: every split leaves the largest alone in the last bin, one level each"""
    xf = np.zeros((k, 12), np.float32)
    xf[:, 9] = np.ldexp(np.float32(1.0), (-149 + 4 * np.arange(k)).astype(np.int32)).astype(np.float32)
    return xf


def test_status_2_and_the_deepest_tree(torch_mod):
    torch = torch_mod
    isc = scene_of("unit")
    bb = bboxes(isc.blas)
    # 65 instances: depth 64, the deepest tree the host accepts -- byte-equal
    _, depth, _ = check_rebuild(torch, isc, deep_chain(65), np.zeros(65, np.int32))
    assert depth == 64
    before = read_tree(isc)
    for k in (66, 70):
        xf = deep_chain(k)
        nodes = np.zeros(2 * k, dtype=before[0].dtype)
        nn, dd = C.c_int(0), C.c_int(0)
        rc = _lib.lib().snail_instances_build(_lib.ptr(xf), _lib.ptr(np.zeros(k, np.int32)), k, _lib.ptr(bb), 1, _lib.ptr(nodes), C.addressof(nn), C.addressof(dd), None)
        assert rc == 2, "the host builder must refuse this input as too deep (returned %d)" % rc
        _, info = isc.update_dev(torch.from_numpy(xf).cuda())
        assert info.cpu().numpy()[0] == 2, info
        after = read_tree(isc)
        assert all(p.tobytes() == q.tobytes() for p, q in zip(before, after))
        assert isc.depth == 64


def test_host_side_argument_errors(torch_mod):
    torch = torch_mod
    isc = scene_of("box")
    L = _lib.lib()
    xf = torch.zeros((4, 12), dtype=torch.float32, device="cuda")
    before = read_tree(isc)
    for args, word in (((isc._h, _lib.ptr(xf), None, 0, None, None, None), "instances"),
                       ((isc._h, _lib.ptr(xf), None, -3, None, None, None), "instances"),
                       ((isc._h, _lib.ptr(xf), None, (1 << 30) + 1, None, None, None), "instances"),
                       ((isc._h, None, None, 4, None, None, None), "null transforms"),
                       ((None, _lib.ptr(xf), None, 4, None, None, None), "handle")):
        assert L.snail_instances_rebuild_dev(*args) != 0
        msg = L.snail_last_error().decode()
        assert "snail_instances_rebuild_dev" in msg and word in msg, msg
    assert L.snail_instances_read_tree(isc._h, _lib.ptr(np.zeros(1, before[0].dtype)), 0, None, None, None, 0, None) != 0
    assert "room for 0 nodes" in L.snail_last_error().decode()
    with pytest.raises(ValueError):
        isc.update_dev(torch.zeros((4, 12), dtype=torch.float32))            # a host tensor
    with pytest.raises(ValueError):
        isc.update_dev(torch.zeros((4, 9), dtype=torch.float32, device="cuda"))
    after = read_tree(isc)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(before, after))
