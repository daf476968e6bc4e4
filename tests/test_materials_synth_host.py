"""The synthetic hit records of tests/materials_synth.py, the parts that need no GPU: the generator stays inside the documented domain of
include/snail_materials.h, the restatements (tests/materials_ref.py, tests/materials_bounce_ref.py) reach on the generated lists every branch,
kind and (texture, level) pair that tests/test_gpu_materials_synth.py rests on -- conditions that keep those comparisons from passing
vacuously, not measurements -- and pins of RefTexture.sample that do not rest on the restatement's own arithmetic."""
import numpy as np
import pytest

from snail_amd import materials as P
from tests import materials_ref as M
from tests import materials_synth as Y
from tests import oracle_lib as O

F = np.float32
INF = F(np.inf)


# ---- the generator ----
def test_the_set_is_inside_the_documented_domain():
    s = Y.synth()
    assert 200 <= s.n <= 400 and Y.N_PACKETS <= 64
    assert [t.shape[:2] for t in s.textures] == [(h, w) for w, h in Y.SHAPES] == [t.shape[:2] for t in s.textures_grey]
    assert len(set(Y.GREYS)) == len(Y.SHAPES) and all((t == g).all() for t, g in zip(s.textures_grey, Y.GREYS))
    # the product's own validation: finite, |uv| < 2^20 -- and its records are the restatement's
    got = P.pack_shtris(s.uv, s.nrm, s.mat_index, s.flat, s.osc.perm)
    assert np.array_equal(got, M.shtris_bytes(*M.pack_shtris(s.uv, s.nrm, s.mat_index, s.flat, s.osc.perm)))
    assert np.abs(s.uv).max() == F(1048575.9375)
    # every map entry crossed with every class and with flat / not flat
    seen = {(m["cls"], int(e), bool(f)) for m, e, f in zip(s.meta, s.mat_index, s.flat)}
    for cls in Y.UV_CLASSES + ["partner"]:
        for e in range(len(Y.MAP)):
            assert (cls, e, False) in seen and (cls, e, True) in seen, (cls, e)
    assert sorted(Y.MAP) == list(range(-1, 14)) and all(m != i for i, m in enumerate(Y.MAP))
    kinds = [d[0] for d in s.descs]
    assert kinds == ["tex"] * 10 + ["simple"] * 2 + ["uber"] * 2 and [d[1] for d in s.descs[:10]] == list(range(10))
    assert [d[2] for d in s.descs[:10]] == [True, False] * 5 and [d[2] for d in s.descs[10:12]] == [True, False] and [d[3] for d in s.descs[12:]] == [0.0, 1.0]
    # normals: exact zeros, tiny, about 1, long -- finite, not normalised
    ln = np.sqrt((s.nrm.astype(np.float64) ** 2).sum(axis=2))
    assert (ln == 0).sum() >= 30 and ((ln > 0) & (ln < 2e-20)).sum() >= 30 and ((ln > 0.7) & (ln < 1.3)).sum() >= 30 and (ln > 700).sum() >= 30
    assert ((ln > 0.7) & (ln < 1.3) & (np.abs(ln - 1) > 1e-3)).sum() >= 30
    # partners: the same triangle shifted by exact integers
    for i, m in enumerate(s.meta):
        if "partner" in m:
            j = m["partner"]
            sh = s.uv[j].astype(np.float64) - s.uv[i].astype(np.float64)
            assert (sh == sh[0]).all() and (sh == np.round(sh)).all() and (sh != 0).all() and np.abs(sh).max() <= 8000
            assert np.array_equal(s.nrm[i], s.nrm[j]) and s.mat_index[i] == s.mat_index[j] and s.flat[i] == s.flat[j]
            assert (np.abs(s.uv[i]) < 8).all() and np.array_equal(s.uv[i] * 64, np.round(s.uv[i] * 64))
    assert max(np.abs(s.uv[m["partner"]] - s.uv[i]).max() for i, m in enumerate(s.meta) if "partner" in m) > 4000


@pytest.mark.parametrize("generic", [False, True])
def test_the_packets_are_inside_the_documented_domain(generic):
    s = Y.synth()
    recipes, covered = set(), set()
    outside_hit = garbage_missed = n_masked = n_unmasked = 0
    for p in range(Y.N_PACKETS):
        pk = s.packet(p, generic)
        t, tri, bary = pk["t"], pk["tri"], pk["bary"]
        assert t.shape == (64, 4) and t.dtype == np.float32 and tri.shape == (64, 4) and tri.dtype == np.int32 and bary.shape == (64, 8) and bary.dtype == np.float32
        assert not np.isnan(t).any() and np.isfinite(bary).all()
        bits = pk["bits"] if generic else np.full((64, 4), True)
        assert (t[~bits] == -INF).all() and (t[bits] > 0).all()           # finite and positive, +inf on a miss, -inf on a masked lane
        bx, by = bary[:, 0:4], bary[:, 4:8]
        assert (bx >= 0).all() and (by >= 0).all() and (bx.astype(np.float64) + by <= 1.0 + 1e-6).all()
        hit = (t < INF) & bits
        outside_hit += int((hit & ((tri < 0) | (tri >= s.n))).sum())
        assert set(tri[hit & ((tri < 0) | (tri >= s.n))].tolist()) <= {-5, s.n + 7}
        garbage_missed += int((~hit & ((tri < 0) | (tri >= s.n))).sum())
        recipes |= set(pk["recipes"])
        for b in range(16):
            if pk["recipes"][b] == "one":
                assert hit[4 * b:4 * b + 4].all() and (tri[4 * b:4 * b + 4] == tri[4 * b, 0]).all()
                covered.add(int(tri[4 * b, 0]))
        if generic:
            assert pk["dirs"].shape == (64, 3, 4) and pk["dirs"].dtype == np.float32 and np.isfinite(pk["dirs"]).all()
            n_masked += not bits.all()
            n_unmasked += bool(bits.all())
    assert recipes == {"one", "one_material", "materials", "partial_one_material", "lane0_missed", "none", "odd_lane", "garbage_misses", "outside_hits"}
    assert covered == set(range(s.n))                                     # a full block on one triangle, for every triangle
    assert outside_hit >= 16 and garbage_missed >= 16
    if generic:
        assert n_masked >= 8 and n_unmasked >= 8                          # hasMask takes both values


# ---- the conditions on the restatement's diagnostics ----
def test_conditions_of_the_primary_list():
    smp, d = Y.expected_primary(O.MODE_IEEE)
    print(Y.describe(d))
    Y.check_conditions(d)
    assert np.isfinite(smp).all()                                         # nothing overflows: the domain excludes it


def test_conditions_of_the_generic_list():
    smp, bd = Y.expected_generic()
    print(Y.describe(bd.nested, bd))
    Y.check_conditions(bd.nested, bd)
    assert np.isfinite(smp).all()


def test_textured_lanes_reach_the_edges_of_the_coordinate_domain():
    """the interpolated coordinates of the covering blocks' textured lanes: exact integers, negative ones a few ulps below an integer,
    magnitudes next to 2^20, and tiny negatives that ClampTexCoord wraps to exactly 1.0 (x1 = w - 1, x2 wraps to 0).  Each class has 20
    triangles with a TEX material, and every covering block of such a triangle puts lanes on its vertices: 16 lanes is the floor."""
    s, ref = Y.synth(), Y.reference()
    integers = huge = wrapped_to_one = below_integer = 0
    for p in range(s.n_cover):
        pk = s.packet(p)
        for b in range(16):
            slot = int(pk["tri"][4 * b, 0])
            m = Y.MAP[int(s.mat_index[s.input_of[slot]])]
            if m < 0 or s.descs[m][0] != "tex":
                continue
            bx, by = pk["bary"][4 * b:4 * b + 4, 0:4], pk["bary"][4 * b:4 * b + 4, 4:8]
            for c in range(2):
                tc = M.lerp_left(ref.uv[slot, 0, c], ref.uv[slot, 1, c], ref.uv[slot, 2, c], bx, by)
                fr = (tc - np.trunc(tc)).astype(np.float32)
                ux = np.where(fr < 0, fr + F(1.0), fr).astype(np.float32)
                integers += int((fr == 0).sum()); huge += int((np.abs(tc) >= 1048575).sum()); wrapped_to_one += int((ux == 1).sum())
                below_integer += int(((fr < 0) & (fr > -1e-5)).sum())
    print("textured lanes: on integers %d, next to 2^20 %d, wrapped to exactly 1.0 %d, just below an integer %d" % (integers, huge, wrapped_to_one, below_integer))
    assert min(integers, huge, wrapped_to_one, below_integer) >= 16


def test_the_frame_with_the_ten_texture_set_samples_every_texture():
    c, _, ref = Y.frame_case()
    d = M.Diag()
    frame, _, _, _ = ref.render(c["cam70"].as_array13(), Y.FRAME[0], Y.FRAME[1], c["lights"], diag=d)
    assert sorted({t for (t, _) in d.mips}) == list(range(len(Y.SHAPES))) and d.hit_pixels >= 1000 and frame.any()
    assert min(d.blocks_a, d.blocks_c) >= 16, (d.blocks_a, d.blocks_c)      # (the case's one-material bands went with its materials: (b) is the lists')


def test_clamped_ids_follow_the_header_s_rule():
    assert Y.clamp_ids(np.array([-5, -1, 0, 7, 278, 279, 286, 2**31 - 1, -2**31]), 279).tolist() == [0, 0, 0, 7, 278, 278, 278, 278, 0]


def test_the_restatement_samples_a_dyadic_triangle_and_its_partner_identically():
    """the exactness argument of the generator, checked: for the pair packets every product and sum of the interpolation is exact, so the whole
    sample -- texture, normal, N.R -- is the same for the triangle and for its integer-shifted partner"""
    s, ref = Y.synth(), Y.reference()
    tex = 0
    for k in range(4):
        a, b = s.pair_packets(k)
        assert (a["tri"] != b["tri"]).all()
        ra = ref.samples(a["dirs"], a["t"], a["tri"], a["bary"], M.Diag())
        rb = ref.samples(b["dirs"], b["t"], b["tri"], b["bary"], M.Diag())
        for x, y in zip(ra[1:], rb[1:]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        assert ra[2].any()
        tex += sum(s.descs[Y.MAP[int(s.mat_index[s.input_of[int(a["tri"][4 * blk, 0])]])]][0] == "tex" for blk in range(16)
                   if Y.MAP[int(s.mat_index[s.input_of[int(a["tri"][4 * blk, 0])]])] >= 0)
    assert tex >= 16


# ---- pins of RefTexture.sample that do not rest on the restatement ----
def coords(rng, n):
    """dyadic coordinates (multiples of 1/64 below 8) and texture-coordinate steps that reach every level"""
    cu = rng.randint(-511, 512, size=n) / 64.0
    cv = rng.randint(-511, 512, size=n) / 64.0
    td = 10.0 ** rng.uniform(-5, 4, size=(2, n))
    return cu.astype(np.float32), cv.astype(np.float32), td[0].astype(np.float32), td[1].astype(np.float32)


@pytest.mark.parametrize("k", range(len(Y.SHAPES)))
def test_a_grey_texture_samples_to_its_grey_at_every_shape(k):
    """every byte of every level of a constant grey is that grey (for grey only: the height-1 row case of GenMips mixes channels), and any
    bilinear tap of equal texels is the texel: float32(g) * (1 / 255) exactly"""
    t, g = Y.ref_textures(grey=True)[k], Y.GREYS[k]
    assert (t.levels == g).all() and len(t.levels) == P.texture_size(*Y.SHAPES[k])[0]
    cu, cv, tdx, tdy = coords(np.random.RandomState(40 + k), 512)
    cu[:8] = [0.0, 1.0, -1.0, 7.984375, -7.984375, 1048575.9375, -1048575.9375, -1e-9]
    rgb, mip = t.sample(cu, cv, tdx, tdy)
    want = F(g) * (F(1.0) / F(255.0))
    assert (rgb == want).all() and rgb.dtype == np.float32
    if min(Y.SHAPES[k]) >= 2:
        assert set(mip.tolist()) == set(range(len(t.shapes)))
    else:
        assert (mip == 0).all()


@pytest.mark.parametrize("k", range(len(Y.SHAPES)))
def test_a_dyadic_coordinate_and_its_integer_shift_sample_identically_at_every_shape(k):
    t = Y.ref_textures()[k]
    rng = np.random.RandomState(60 + k)
    cu, cv, tdx, tdy = coords(rng, 512)
    base, mip = t.sample(cu, cv, tdx, tdy)
    for lim in (3, 16, 8000):
        su, sv = rng.randint(-lim, lim + 1, size=512), rng.randint(-lim, lim + 1, size=512)
        got, mip2 = t.sample((cu.astype(np.float64) + su).astype(np.float32), (cv.astype(np.float64) + sv).astype(np.float32), tdx, tdy)
        assert np.array_equal(got.view(np.uint32), base.view(np.uint32)) and np.array_equal(mip, mip2), lim
    assert len(np.unique(base.view(np.uint32).reshape(-1, 3), axis=0)) > (0 if Y.SHAPES[k] == (1, 1) else 2)       # (noise: the taps differ)


@pytest.mark.parametrize("k", [4, 5])
def test_texel_centre_taps_on_8x32_and_32x8(k):
    """a tap at a texel centre returns level0[(h - y) & (h - 1), x]: rows count from the top, h wraps to 0"""
    (w, h), level0, t = Y.SHAPES[k], Y.synth().textures[k], Y.ref_textures()[k]
    assert (w, h) in ((8, 32), (32, 8))
    checked = 0
    z = np.zeros(1, np.float32)
    for x in range(w - 1):
        for y in range(h - 1):
            u, v = F(x) / F(w - 1), F(y) / F(h - 1)
            if (u * F(w - 1), v * F(h - 1)) != (x, y):
                continue
            rgb, mip = t.sample(np.array([u]), np.array([v]), z, z)
            want = level0[(h - y) & (h - 1), x].astype(np.float32) * (F(1.0) / F(255.0))
            assert mip[0] == 0 and np.array_equal(rgb[0], want), (x, y)
            checked += 1
    assert checked >= 64
