"""The sample stage of instanced full shading on the MI355X -- k_imat_sample (snail_amd/csrc/instances_materials.inc) -- on the SYNTHETIC hit
records of tests/instances_materials_synth.py, bit for bit against the restatement (tests/instances_materials_ref.py behind the clamp rule
of the header) in both arithmetics.  Every other GPU test of this kernel feeds it what a traversal of three procedural cases produced: six
instances of two BLASes, two textures.  Here it meets three BLASes of 291, 12 and 1 triangles behind maps of their own, 13 instances
addressed by builder slot, blocks of every (slot, triId) equality built on purpose, the (slot 0, triId 0) quirk beside its two
neighbours, slots and ids outside the scene, ids valid in one BLAS and out of range in another, normals of length 0, 1e-20 and 1e3 under
general rotations, and the texture shapes of tests/materials_synth.py through this kernel's own copy of the sampling code.  Independent
of the restatement: the same records with the slots of identity instances collapsed, exact rotations against the identity, and the plain
scenes' k_mat_sample on the same records.  What the list must exercise is asserted on the restatement's diagnostics here and, without a
GPU, by tests/test_instances_materials_synth_host.py.  All comparisons are by bit pattern.  Nothing here reads outside the repository.

Left out (tests/instances_materials_synth.py says why): non-finite barycentrics and t = NaN, slots at or above the count on a handle that
shrank, subnormal products, non-rigid matrices, k_imat_light on synthetic samples, texDiff products at or above 2^32."""
import functools

import numpy as np
import pytest

from snail_amd import HostBVH
from snail_amd import instances_materials as IP
from snail_amd import materials as P
from snail_amd.instances import InstancedScene
from snail_amd.scene import Scene
from tests import instances_materials_synth as Z
from tests import materials_synth as Y
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu
ARITH = [("ieee", O.MODE_IEEE), ("host_sse", O.MODE_SSE)]
INF = np.float32(np.inf)
RESX, RESY = Y.FRAME
CAM = Y.Cam()
PLANES = ["normal x", "normal y", "normal z", "diffuse r", "diffuse g", "diffuse b", "specular r", "specular g", "specular b"]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def product_materials():
    mats = [P.Material.simple(d[1], d[2]) if d[0] == "simple" else P.Material.textured(d[1], d[2]) if d[0] == "tex" else P.Material.uber(d[1], d[2], d[3])
            for d in Y.material_descs()]
    return mats, [P.Texture(t) for t in Y.synth().textures]


@functools.lru_cache(maxsize=None)
def blas_scenes():
    """the device Scene of every BLAS, built once; the product builder's tree is the oracle's, so the generator's triIds are the product's"""
    out = []
    for b in Z.blases():
        hb = HostBVH.build(b.tv)
        assert np.array_equal(hb.perm, b.osc.perm) and hb.nodes.tobytes() == b.osc.nodes.tobytes()
        out.append(Scene(hb, 0))
    return out


def check_tree(isc, ref):
    xs, bs = isc.slot_transforms()
    assert isc.nodes().tobytes() == ref.nodes.tobytes() and np.array_equal(xs, ref.xf) and np.array_equal(bs, ref.bi)


def new_set(key="main"):
    """(InstancedScene, InstancedMaterialSet) of an arrangement on a freshly created handle (capacity = count); the handle's tree and slot
    order are the restated ones"""
    a = Z.arrangement(key)
    isc = InstancedScene(blas_scenes(), a.rot, a.tr, a.bi_input)
    check_tree(isc, a.ref)
    mats, texs = product_materials()
    return isc, IP.InstancedMaterialSet(isc, [b.per_blas for b in Z.blases()], mats, texs)


@functools.lru_cache(maxsize=None)
def device_set():
    return new_set()


def set_arith(arith):
    for s in blas_scenes():
        s.set_arith(arith)


def dev(torch, a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")      # (a copy: the shared inputs are read-only)


def hits_of(torch, r):
    n = len(r["t"])
    return (dev(torch, r["t"].reshape(n, 256)), dev(torch, r["bary"][:, :, 0:4].reshape(n, 256)), dev(torch, r["bary"][:, :, 4:8].reshape(n, 256)),
            dev(torch, r["slot"].reshape(n, 256)), dev(torch, r["tri"].reshape(n, 256)))


def shade(torch, ms, r):
    return ms.shade_packets(CAM, RESX, RESY, dev(torch, Z.packet_xy(len(r["t"]))), hits_of(torch, r)).cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def compare_planes(what, got, want):
    """all planes given (nine, or the three of the normal) by bit pattern; prints the number of differing words per plane before it asserts"""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (got.shape, want.shape)
    ne = bits(got) != bits(want)
    print("%s: %d differing words of %d; per plane %s" % (what, int(ne.sum()), ne.size, {PLANES[c]: int(ne[:, c].sum()) for c in range(ne.shape[1]) if ne[:, c].any()}))
    if ne.any():
        at = tuple(np.argwhere(ne)[0])
        raise AssertionError("%s: %d words differ; first at (packet, plane, quad, lane) %s: %r / %r; packets %s" % (
            what, int(ne.sum()), at, got[at], want[at], sorted(set(np.argwhere(ne)[:, 0].tolist()))[:16]))


def recipe_of(r, at):
    return r["info"][at[0]][at[2] // 4]


# ---- 1. the list against the restatement ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_the_list_equals_the_restatement(torch_mod, arith, mode):
    _, ms = device_set()
    r = Z.records()
    want, d = Z.expected(mode)
    set_arith(arith)
    try:
        got = shade(torch_mod, ms, r)
    finally:
        set_arith("ieee")
    print(Z.describe(d))
    ne = bits(got) != bits(want)
    if ne.any():
        print("recipes of the differing blocks: %s" % sorted({recipe_of(r, at)["recipe"] for at in np.argwhere(ne).tolist()}))
    compare_planes("the list, %s" % arith, got, want)
    Z.check_conditions(d)


# ---- 2. device against device: the slots of identity instances collapsed ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_collapsed_identity_slots_change_the_branch_and_nothing_else(torch_mod, arith, mode):
    """same_tri_two_slots blocks whose slots are all identity instances of one BLAS: the records of the slots are equal, so replacing every slot
    by the block's first changes only the branch, (b) -> (a).  The two device runs differ exactly where the restatement's two runs differ,
    and every block that was left alone -- (b) in both runs among them -- is bit-equal between the runs."""
    _, ms = device_set()
    r = Z.records()
    col, which = Z.collapse_identity_blocks(r)
    w1, _ = Z.expected(mode)
    w2, _ = Z.expected_of(col, mode)
    set_arith(arith)
    try:
        g1, g2 = shade(torch_mod, ms, r), shade(torch_mod, ms, col)
    finally:
        set_arith("ieee")
    dev_ne, ref_ne = bits(g1) != bits(g2), bits(w1) != bits(w2)
    print("collapsed %d blocks, %s: %d words differ between the device runs, %d between the restatement's" % (int(which.sum()), arith, int(dev_ne.sum()), int(ref_ne.sum())))
    assert which.sum() >= 8 and np.array_equal(dev_ne, ref_ne)
    blocks = dev_ne.any(axis=1).reshape(len(g1), 16, 16).any(axis=2)
    assert blocks[which].all() and not blocks[~which].any()
    others_b = sum(1 for p, infos in enumerate(r["info"]) for b, i in enumerate(infos) if i["recipe"] == "same_tri_two_slots" and not which[p, b])
    assert others_b >= 16


# ---- 3. exact rotations ----
def signed_permutation_of(planes, rot):
    out = np.zeros_like(planes)
    for k in range(3):
        j = int(np.flatnonzero(rot[k])[0])
        out[:, k] = planes[:, j] * rot[k, j]
    return out


@pytest.mark.parametrize("arith,mode", ARITH)
def test_exact_rotations_permute_dyadic_normals(torch_mod, arith, mode):
    """single-pair blocks on the dyadic-normal triangles WITHOUT a zero component, in an identity slot of "big" and in each signed-permutation
    slot: every step of Transform is exact, so the rotated run's normal planes are the signed permutation of the identity run's by bits (no
    zero sums arise), and a TEX material without N.R has bit-equal diffuse and specular planes.  For the variant WITH an exact-zero component
    the sign of a zero sum depends on the order of the additions: only the comparison with the restatement (test 1) covers it."""
    _, ms = device_set()
    a, big = Z.arrangement(), Z.blases()[Z.BIG]
    runs = {name: Z.dyadic_records(a.slots(Z.BIG, [name])[0], (0,)) for name in ("identity",) + Z.EXACT}
    set_arith(arith)
    try:
        got = {name: shade(torch_mod, ms, r) for name, r in runs.items()}
    finally:
        set_arith("ieee")
    base = got["identity"]
    assert base[:, 0:3].all()
    mat = big.material[runs["identity"]["tri"]]                                          # [n, 64, 4]
    plain_tex = np.isin(mat, [m for m, d in enumerate(Y.material_descs()) if d[0] == "tex" and not d[2]])
    assert plain_tex.sum() >= 128                                                        # (two of the six triangles, five blocks each at the least)
    for name in Z.EXACT:
        compare_planes("normals under %s, %s" % (name, arith), np.ascontiguousarray(got[name][:, 0:3]), signed_permutation_of(base[:, 0:3], Z.ROTATIONS[name]))
        assert not np.array_equal(bits(got[name][:, 0:3]), bits(base[:, 0:3]))
        for c in range(3, 9):
            assert np.array_equal(bits(got[name][:, c])[plain_tex], bits(base[:, c])[plain_tex]), (name, PLANES[c])
    assert base[:, 3:6].transpose(0, 2, 3, 1)[plain_tex].any()


# ---- 4. the twin, device against device ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_an_identity_slot_equals_the_plain_scenes_kernel(torch_mod, arith, mode):
    """one identity slot of "big", dyadic-normal triangles (Transform's round trip is exact there: tests/test_instances_materials_synth_host.py):
    k_imat_sample's samples are k_mat_sample's over "big" as a plain scene with the same data and the same t, u, v, tri.  No restatement."""
    torch = torch_mod
    _, ms = device_set()
    a, big = Z.arrangement(), Z.blases()[Z.BIG]
    mats, texs = product_materials()
    plain = P.MaterialSet(blas_scenes()[Z.BIG], big.uv, big.nrm, big.mat_index, big.flat, big.map, mats, texs)
    r = Z.dyadic_records(a.slots(Z.BIG, ["identity"])[1], mixed=True)
    h = hits_of(torch, r)
    set_arith(arith)
    try:
        got = shade(torch, ms, r)
        want = plain.shade_packets(CAM, RESX, RESY, dev(torch, Z.packet_xy(len(r["t"]))), (h[0], h[1], h[2], h[4])).cpu().numpy()
    finally:
        set_arith("ieee")
    compare_planes("identity slot against the plain kernel, %s" % arith, got, want)
    assert got[:, 0:3].any() and got[:, 3:].any() and (r["t"] == INF).any()


# ---- 5. the same set after update and update_dev ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_the_same_set_follows_updates(torch_mod, arith, mode):
    """the SAME records under new transforms: every rotation replaced, the translations mirrored (so the slots are other instances, slot 0 a
    box, and an id valid in a slot's old BLAS may be out of range in its new one), the instance count and BLAS indices kept (capacity stays
    the count)"""
    torch = torch_mod
    a, u = Z.arrangement(), Z.arrangement("updated")
    r = Z.records()
    old, _ = Z.expected(mode)
    new, _ = Z.expected_of(r, mode, "updated")
    assert int((bits(old) != bits(new)).sum()) >= 10000
    isc, ms = new_set()                                               # (a handle of this test's own: the cached one keeps its transforms)
    set_arith(arith)
    try:
        compare_planes("before the update, %s" % arith, shade(torch, ms, r), old)
        isc.update(u.rot, u.tr, u.bi_input)
        check_tree(isc, u.ref)
        compare_planes("after update, %s" % arith, shade(torch, ms, r), new)
        isc.update_dev(dev(torch, a.xf_input), dev(torch, a.bi_input))
        got = shade(torch, ms, r)
        check_tree(isc, a.ref)
        compare_planes("after update_dev, %s" % arith, got, old)
    finally:
        set_arith("ieee")
        ms.close()
        isc.close()


# ---- 6. the edges of the call ----
def test_an_empty_list_and_a_longer_buffer(torch_mod):
    torch = torch_mod
    _, ms = device_set()
    r = Z.records()
    n = 3
    sub = {k: v[:n] for k, v in r.items()}
    want, _ = Z.expected(O.MODE_IEEE)
    poison = np.float32(-12345.5)
    buf = torch.full((n + 1, 9, 64, 4), float(poison), dtype=torch.float32, device="cuda:0")
    xy, h = dev(torch, Z.packet_xy(n)), hits_of(torch, sub)
    # nPackets = 0: success, nothing written
    ms.shade_packets(CAM, RESX, RESY, xy[:0], tuple(x[:0] for x in h), out=buf)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == poison).all()
    # a buffer one packet longer than the list keeps its poison past the list's end
    ms.shade_packets(CAM, RESX, RESY, xy, h, out=buf)
    got = buf.cpu().numpy()
    compare_planes("the first %d packets into a longer buffer" % n, np.ascontiguousarray(got[:n]), np.ascontiguousarray(want[:n]))
    assert (got[n] == poison).all()
