"""The synthetic hit records of tests/instances_materials_synth.py, the parts that need no GPU: the list exercises what
tests/test_gpu_instances_materials_synth.py rests on (conditions that keep those comparisons from passing vacuously, asserted on the
restatement's diagnostics), the list is ABLE to fail (three mutated restatements differ from the real one on a stated share of lanes), the clamp
rule, and the exactness argument behind the device-against-device tests."""
import numpy as np

from snail_amd import materials as P
from tests import instances_materials_ref as IM
from tests import instances_materials_synth as Z
from tests import materials_cases as MK
from tests import materials_ref as M
from tests import materials_synth as Y
from tests import oracle_lib as O

F = np.float32
INF = F(np.inf)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def block_differs(a, b):
    """bool [n, 16]: some word of the block differs between two sample buffers [n, 9, 64, 4]"""
    ne = (bits(a) != bits(b)).any(axis=1)                                # [n, 64, 4]
    return ne.reshape(len(a), 16, 16).any(axis=2)


# ---- the generator ----
def test_the_shading_data_and_the_instances():
    big, box, tiny = Z.blases()
    s = Y.synth()
    assert big.n == s.n + 2 * len(Z.DYADIC_ENTRIES) and box.n == 12 and tiny.n == 1
    assert np.array_equal(big.uv[:s.n], s.uv) and np.array_equal(big.nrm[:s.n], s.nrm) and big.map == Y.MAP
    # the product's own validation accepts every BLAS's data, and its records are the restatement's
    for b in (big, box, tiny):
        got = P.pack_shtris(b.uv, b.nrm, b.mat_index, b.flat, b.osc.perm)
        assert np.array_equal(got, M.shtris_bytes(*M.pack_shtris(b.uv, b.nrm, b.mat_index, b.flat, b.osc.perm)))
    # the dyadic normals: multiples of 1/64 up to 4, one sign per component; a variant without a zero and one with an exact-zero component
    for v in (0, 1):
        tris = Z.dyadic_tris((v,))
        assert len(tris) == len(Z.DYADIC_ENTRIES)
        n = big.nrm[big.input_of[tris]]
        assert np.array_equal(n * 64, np.round(n * 64)) and (np.abs(n) <= 4).all()
        assert ((n == 0).all(axis=1).sum(axis=1) == v).all() and ((n > 0).all(axis=1) | (n < 0).all(axis=1) | (n == 0).all(axis=1)).all()
    # the maps: another shuffle of another length; one class index, two materials; one material, two indices; materials that several maps name
    assert len(Z.BOX_MAP) != len(Y.MAP) and Z.BOX_MAP[0] != Y.MAP[0] and Z.BOX_MAP[0] == Z.BOX_MAP[4] == Z.UBER_SHARED
    assert Z.UBER_SHARED in Y.MAP and Z.UBER_SHARED in Z.TINY_MAP and Z.TEX_SHARED in Y.MAP and Z.TEX_SHARED in Z.BOX_MAP and -1 in Z.TINY_MAP
    assert Y.material_descs()[Z.UBER_SHARED][0] == "uber" and Y.material_descs()[Z.TEX_SHARED] == ("tex", 3, False)
    assert set(box.mat_index.tolist()) == set(range(len(Z.BOX_MAP)))
    # the instances: every BLAS under the identity and a general rotation, "big" under every exact one; slots are NOT the input order
    a = Z.arrangement()
    assert a.n >= 12 and len(a.slots(Z.BIG, ["identity"])) == 2
    for b in range(3):
        assert a.slots(b, ["identity"]) and a.slots(b, ["general0", "general1", "general2"])
    assert all(a.slots(Z.BIG, [r]) for r in Z.EXACT)
    for r in Z.EXACT:
        m = Z.ROTATIONS[r]
        assert np.array_equal(np.abs(m).sum(axis=0), [1, 1, 1]) and np.array_equal(np.abs(m).sum(axis=1), [1, 1, 1]) and np.linalg.det(m) == 1.0
    assert (Z.PERM3.min(axis=1) < 0).all()
    assert not np.array_equal(a.perm, np.arange(a.n)) and a.bi[0] == Z.BIG and a.name[0] == "general0"
    u = Z.arrangement("updated")
    assert np.array_equal(u.bi_input, a.bi_input) and not np.array_equal(u.perm, a.perm) and u.bi[0] == Z.BOX      # the second arrangement: slot 0 is a box


def test_the_packets_are_inside_the_documented_domain():
    r, a = Z.records(), Z.arrangement()
    B = Z.blases()
    assert r["t"].shape == (Z.N_PACKETS, 64, 4) and r["t"].dtype == np.float32 and r["slot"].dtype == r["tri"].dtype == np.int32 and r["bary"].shape == (48, 64, 8)
    assert not np.isnan(r["t"]).any() and (r["t"] > 0).all() and np.isfinite(r["bary"]).all()
    bx, by = r["bary"][:, :, 0:4], r["bary"][:, :, 4:8]
    assert (bx >= 0).all() and (by >= 0).all() and (bx.astype(np.float64) + by <= 1.0 + 1e-6).all()
    recipes = {i["recipe"] for infos in r["info"] for i in infos}
    assert recipes == {"one", "same_tri_two_slots", "same_tri_two_blas", "shared_material", "materials", "partial_one_material", "odd_lane", "none", "lane0_missed",
                       "garbage_misses", "outside_hits"}
    # the covering part: every triangle of every BLAS in a full block under an identity slot and under a rotated one
    seen = set()
    for p, infos in enumerate(r["info"]):
        for b, i in enumerate(infos):
            if i["recipe"] == "one":
                qs = slice(4 * b, 4 * b + 4)
                s, t = int(r["slot"][p, 4 * b, 0]), int(r["tri"][p, 4 * b, 0])
                assert (r["slot"][p, qs] == s).all() and (r["tri"][p, qs] == t).all() and (r["t"][p, qs] < INF).all()
                seen.add((int(a.bi[s]), t, a.name[s] == "identity"))
    for b in range(3):
        for t in range(B[b].n):
            assert (b, t, True) in seen and (b, t, False) in seen, (b, t)
    # hit lanes outside the scene carry the slots -3 and nInst + 5 alone (outside_hits, lane0_missed); garbage slots only on lanes that missed
    hit = r["t"] < INF
    out_slot = hit & ((r["slot"] < 0) | (r["slot"] >= a.n))
    assert set(r["slot"][out_slot].tolist()) == {-3, a.n + 5}
    assert int((~hit & ((r["slot"] < 0) | (r["slot"] >= a.n))).sum()) >= 32


def test_conditions_of_the_list():
    smp, d = Z.expected(O.MODE_IEEE)
    print(Z.describe(d))
    Z.check_conditions(d)
    assert np.isfinite(smp).all()


def test_clamp_records():
    a = Z.arrangement()
    n = a.n
    big_slot, box_slot, tiny_slot = a.slots_of_blas[0][0], a.slots_of_blas[1][0], a.slots_of_blas[2][0]
    nb = Z.blases()[0].n
    slot = np.array([-3, -1, 0, n - 1, n, n + 5, big_slot, big_slot, box_slot, box_slot, tiny_slot, tiny_slot, box_slot])
    tri = np.array([5, 5, -5, 0, 0, 0, nb + 7, nb + 9, 19, 21, 3, -2**31, 11])
    s, key, rec = Z.clamp_records(slot, tri)
    assert s.tolist() == [0, 0, 0, n - 1, n - 1, n - 1, big_slot, big_slot, box_slot, box_slot, tiny_slot, tiny_slot, box_slot]
    assert key.tolist() == [5, 5, 0, 0, 0, 0, nb + 7, nb + 9, 19, 21, 3, 0, 11]            # the keys of n + 7 and n + 9 differ ...
    assert rec[6] == rec[7] == nb - 1 and rec[8] == rec[9] == 11 and rec[10] == rec[11] == 0 and rec[12] == 11      # ... their records do not
    # in-range records are untouched, and the rule is idempotent
    rng = np.random.RandomState(3)
    sl = rng.randint(0, n, size=500)
    tr = (rng.rand(500) * a.n_tris[sl]).astype(np.int64)
    s2, k2, r2 = Z.clamp_records(sl, tr)
    assert np.array_equal(s2, sl) and np.array_equal(k2, tr) and np.array_equal(r2, tr)
    r = Z.records()
    s1, k1, r1 = Z.clamp_records(r["slot"], r["tri"])
    for again in (Z.clamp_records(s1, k1), Z.clamp_records(s1, r1)):
        assert np.array_equal(again[0], s1) and np.array_equal(again[2], r1)
    assert np.array_equal(Z.clamp_records(s1, k1)[1], k1)


# ---- the list is able to fail ----
def test_skipping_transform_shows_on_the_rotated_lanes():
    r, a = Z.records(), Z.arrangement()
    want, _ = Z.expected(O.MODE_IEEE)
    got, _ = Z.expected_of(r, O.MODE_IEEE, ref=Z.reference(transform=False))
    s, _, _ = Z.clamp_records(r["slot"], r["tri"])
    rotated = (r["t"] < INF) & np.array([n != "identity" for n in a.name])[s]
    ne = (bits(got[:, 0:3]) != bits(want[:, 0:3])).any(axis=1)
    print("transform skipped: %d of %d rotated hit lanes differ in their normals" % (int((ne & rotated).sum()), int(rotated.sum())))
    assert int((ne & rotated).sum()) * 4 >= int(rotated.sum()) and rotated.sum() >= 2000      # (nothing is claimed for identity slots: their round trip is not exact either)


def test_comparing_triids_alone_shows_on_every_block_of_one_triid_in_several_slots():
    r = Z.records()
    want, _ = Z.expected(O.MODE_IEEE)
    got, _ = Z.expected_of(Z.collapse_slots_by_tri(r), O.MODE_IEEE)
    diff = block_differs(got, want)
    n = seen = 0
    for p, infos in enumerate(r["info"]):
        for b, i in enumerate(infos):
            if i["recipe"] == "same_tri_two_slots":
                n += 1
                if i["kind"] == "tex" or not i["flat"]:
                    seen += 1
                    assert diff[p, b], (p, b, i)
    print("slots ignored: %d blocks differ; %d of the %d same_tri_two_slots blocks are TEX or not flat" % (int(diff.sum()), seen, n))
    assert seen >= 20 and n >= 29


def test_reading_slots_as_input_order_shows():
    want, _ = Z.expected(O.MODE_IEEE)
    got, _ = Z.expected_of(Z.records(), O.MODE_IEEE, ref=Z.reference(input_order=True))
    ne = (bits(got) != bits(want)).any(axis=1)
    print("slots read as input order: %d lanes differ" % int(ne.sum()))
    assert int(ne.sum()) >= 2000


def test_the_collapsed_identity_blocks_change_branch_and_nothing_else():
    """what test 2 of the GPU file rests on: collapsing the slots of the identity-only blocks turns (b) into (a) there, which shows in every
    such block, and leaves every other block as it was"""
    r = Z.records()
    want, d = Z.expected(O.MODE_IEEE)
    col, which = Z.collapse_identity_blocks(r)
    d2 = IM.Diag()
    got, _ = Z.expected_of(col, O.MODE_IEEE, diag=d2)
    diff = block_differs(got, want)
    assert which.sum() >= 8 and d2.blocks_a - d.blocks_a == which.sum() == d.blocks_b - d2.blocks_b
    assert not diff[~which].any() and diff[which].all(), (int(diff[which].sum()), int(which.sum()))


# ---- the exactness arguments behind the device-against-device tests ----
def test_an_identity_slot_with_dyadic_normals_equals_the_plain_restatement():
    """every step of Transform is exact for dyadic normals under the identity (a zero component included: +0 stays +0), so
    InstMaterialsRef.samples in an identity slot of "big" is MaterialsRef.samples of "big" as a plain scene, bit for bit"""
    a, big = Z.arrangement(), Z.blases()[Z.BIG]
    plain = M.MaterialsRef(big.osc, big.uv, big.nrm, big.mat_index, big.flat, big.map, MK.ref_materials(Y.material_descs()), Y.ref_textures())
    slot = a.slots(Z.BIG, ["identity"])[0]
    r = Z.dyadic_records(slot, mixed=True)
    xy = Z.packet_xy(len(r["t"]))
    di, dp = IM.Diag(), M.Diag()
    for p in range(len(r["t"])):
        d = Y.primary_dirs(int(xy[p, 0]), int(xy[p, 1]), O.MODE_IEEE)
        x = Z.reference().samples(d, r["t"][p], r["slot"][p], r["tri"][p], r["bary"][p], di)
        y = plain.samples(d, r["t"][p], r["tri"][p], r["bary"][p], dp)
        for u, v in zip(x, y):
            assert u.tobytes() == v.tobytes()
    assert min(dp.blocks_a, dp.blocks_b + dp.blocks_masked_one, dp.blocks_c) >= 4 and (di.blocks_a, di.blocks_b, di.blocks_c) == (dp.blocks_a, dp.blocks_b, dp.blocks_c)


def signed_permutation_of(planes, rot):
    """normal planes [n, 3, 64, 4] of an identity slot -> those of a slot whose rotation is the signed permutation rot, by bits"""
    out = np.zeros_like(planes)
    for k in range(3):
        j = int(np.flatnonzero(rot[k])[0])
        out[:, k] = planes[:, j] * rot[k, j]
    return out


def test_exact_rotations_permute_the_dyadic_normals():
    """what test 3 of the GPU file rests on, on the restatement: with no zero component the rotated run's normals are the signed permutation of
    the identity run's, and a TEX material without N.R samples to the same bits"""
    a = Z.arrangement()
    ident = a.slots(Z.BIG, ["identity"])[0]
    base, _ = Z.expected_of(Z.dyadic_records(ident, (0,)), O.MODE_IEEE)
    assert base[:, 0:3].all()                                             # no zero in any normal plane
    for name in Z.EXACT:
        got, _ = Z.expected_of(Z.dyadic_records(a.slots(Z.BIG, [name])[0], (0,)), O.MODE_IEEE)
        assert np.array_equal(bits(got[:, 0:3]), bits(signed_permutation_of(base[:, 0:3], Z.ROTATIONS[name]))), name
        assert not np.array_equal(bits(got[:, 0:3]), bits(base[:, 0:3]))
