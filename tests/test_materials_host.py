"""Full shading, the parts that need no GPU: the host functions of include/snail_materials.h against the test-side restatement
(tests/materials_ref.py) byte for byte, the restatement's own pins, and the cases of tests/materials_cases.py against the conditions the
GPU tests put on them (so that a case that stops exercising what it was chosen for shows here first)."""
import numpy as np
import pytest

from snail_amd import materials as P
from tests import materials_cases as K
from tests import materials_ref as M
from tests import oracle_lib as O


@pytest.mark.parametrize("w,h", [(64, 64), (32, 8), (8, 2), (1, 1), (2, 1), (1, 4), (16, 1),
                                 (2, 2), (1, 8), (8, 1), (8, 32), (8192, 2), (2, 8192), (4, 2048), (256, 256)])
def test_texture_build_equals_the_restatement(w, h):
    """(8, 2): its level 4 x 1 -> 2 x 1 -> 1 x 1 goes through the height-1 row case, whose src[4 + i] reads across pixels and, for the last
    pair, one byte into the level being written.  The second row: the shapes of tests/materials_synth.py that the first lacks"""
    level0 = np.random.RandomState(w * 100 + h).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    t = P.Texture(level0)
    want = M.gen_mips(level0)
    assert t.n_levels == len(M.level_shapes(w, h)) and t.levels.shape == want.shape
    assert np.array_equal(t.levels, want), np.flatnonzero(t.levels != want)[:8]
    assert np.array_equal(t.levels[:w * h * 3], level0.reshape(-1))


def test_height_1_row_case_is_the_reference_s_not_the_tidy_one():
    """4 x 1 -> 2 x 1: dst = (src[i] + src[4 + i]) / 2, not the mean of neighbouring pixels"""
    level0 = np.array([[[10, 20, 30], [40, 50, 60], [70, 80, 90], [100, 110, 120]]], dtype=np.uint8)
    got = P.Texture(level0).levels
    assert got[12:15].tolist() == [(10 + 50) // 2, (20 + 60) // 2, (30 + 70) // 2]
    assert got[15:18].tolist() == [(70 + 110) // 2, (80 + 120) // 2, (90 + int(got[12])) // 2]      # the byte past the pair = the level being written
    assert np.array_equal(got, M.gen_mips(level0))


def test_shtris_pack_equals_the_restatement():
    rng = np.random.RandomState(3)
    n = 257
    uv = (rng.rand(n, 3, 2) * 6 - 3).astype(np.float32); nrm = (rng.rand(n, 3, 3) * 2 - 1).astype(np.float32)
    mi = rng.randint(0, 1000, size=n).astype(np.int32); flat = rng.rand(n) < 0.4
    perm = rng.permutation(n).astype(np.int32)
    got = P.pack_shtris(uv, nrm, mi, flat, perm)
    want = M.shtris_bytes(*M.pack_shtris(uv, nrm, mi, flat, perm))
    assert np.array_equal(got, want)
    ident = P.pack_shtris(uv, nrm, mi, flat)
    assert np.array_equal(ident[perm], got)
    assert (got.view(np.uint32).reshape(n, 16)[:, 15] >> 31).astype(bool).tolist() == flat[perm].tolist()


# ---- the restatement's own pins ----
def test_a_tap_at_a_texel_centre_returns_that_texel():
    level0 = np.random.RandomState(9).randint(0, 256, size=(8, 16, 3)).astype(np.uint8)
    t = M.RefTexture(level0)
    checked = 0
    for x, y in ((0, 0), (3, 2), (5, 0), (7, 6), (14, 3), (10, 5), (12, 4), (6, 1)):     # (u = 1 or v = 1 would wrap to texel 0)
        # pos = uv * (w - 1, h - 1) lands on the integer (x, y); the row is H - y, wrapped: row 0 for y = 0
        u, v = np.float32(x) / np.float32(15), np.float32(y) / np.float32(7)
        if (np.float32(u) * np.float32(15), np.float32(v) * np.float32(7)) != (x, y):
            continue
        rgb, mip = t.sample(np.array([u]), np.array([v]), np.array([0.0], np.float32), np.array([0.0], np.float32))
        want = level0[(8 - y) & 7, x].astype(np.float32) * (np.float32(1.0) / np.float32(255.0))
        assert mip[0] == 0 and np.array_equal(rgb[0], want), (x, y, rgb[0], want)
        checked += 1
    assert checked >= 4
    rgb, _ = t.sample(np.array([0.0], np.float32), np.array([0.0], np.float32), np.zeros(1, np.float32), np.zeros(1, np.float32))
    assert np.array_equal(rgb[0], level0[0, 0].astype(np.float32) * (np.float32(1.0) / np.float32(255.0)))


def test_coordinates_outside_0_1_wrap():
    level0 = np.random.RandomState(10).randint(0, 256, size=(16, 16, 3)).astype(np.uint8)
    t = M.RefTexture(level0)
    z = np.zeros(1, np.float32)
    base, _ = t.sample(np.array([0.25], np.float32), np.array([0.75], np.float32), z, z)
    for du, dv in ((1, 0), (2, 1), (-1, 0), (-3, -2), (0, 2)):       # 0.25, 0.75 and their integer shifts are exact in fp32
        got, _ = t.sample(np.array([0.25 + du], np.float32), np.array([0.75 + dv], np.float32), z, z)
        assert np.array_equal(got, base), (du, dv)
    neg, _ = t.sample(np.array([-0.75], np.float32), np.array([-0.25], np.float32), z, z)     # -0.75 -> 0.25, -0.25 -> 0.75
    assert np.array_equal(neg, base)


def test_mip_choice_and_clamp():
    t = M.RefTexture(np.zeros((64, 64, 3), np.uint8))
    z = np.zeros(1, np.float32)
    for diff, want in ((0.0, 0), (0.02, 0), (0.03, 1), (0.06, 2), (0.9, 6), (50.0, 6)):
        _, mip = t.sample(z, z, np.array([diff], np.float32), np.array([diff], np.float32))
        assert mip[0] == want, (diff, mip[0])
    _, mip = t.sample(z, z, np.array([50.0], np.float32), z)          # Min(x, y): the smaller step decides
    assert mip[0] == 0


def test_uber_swaps_diffuse_x_and_z():
    m = M.RefMaterial(M.UBER, True, (0.1, 0.2, 0.3), (0.4, 0.5, 0.6), 0.0)
    assert m.diffuse.tolist() == [np.float32(0.3), np.float32(0.2), np.float32(0.1)] and m.specular.tolist() == [np.float32(0.4), np.float32(0.5), np.float32(0.6)]


# ---- the cases, against what the GPU tests ask of them ----
def run(name, resx, resy, cam=None, mode=O.MODE_IEEE):
    c = K.case(name)
    d = M.Diag()
    K.reference(name).render((cam or c["cam"]).as_array13(), resx, resy, c["lights"], mode=mode, diag=d)
    return d


def test_degenerate_restatement_equals_the_oracle_s_simple_shading():
    """every triangle flat with its plane normal, every material the default: the full-shading restatement is the oracle's Scene::RayTrace"""
    for name in ("degenerate_box", "degenerate_small"):
        c = K.case(name)
        for resx, resy in ((96, 64), (70, 50)):
            got, gst, _, _ = K.reference(name).render(c["cam"].as_array13(), resx, resy, c["lights"])
            want, wst = c["osc"].render_whitted(c["cam"].as_array13(), resx, resy, c["lights"])
            assert np.array_equal(got, want) and got.any(), name
            assert np.array_equal(gst, wst), (gst, wst)


def test_large_case_conditions():
    for resx, resy in ((96, 64), (70, 50)):
        d = run("large", resx, resy)
        lv = sorted(l for (t, l) in d.mips if t == 0)
        assert d.blocks_a >= 100 and len(lv) >= 3 and lv[0] == 0 and lv[-1] == 6, (d.blocks_a, lv)
        assert any(t == 1 for (t, _) in d.mips)
        assert d.normals_right > 0 and d.normals_left_a > 0 and d.normals_flat > 0


def test_small_case_conditions():
    c = K.case("small")
    for resx, resy, cam in ((96, 64, c["cam"]), (70, 50, c["cam70"])):
        d = run("small", resx, resy, cam)
        assert min(d.blocks_a, d.blocks_b, d.blocks_c) >= 100, (d.blocks_a, d.blocks_b, d.blocks_c)
        assert d.default_meets_others >= 1 and d.uber_unmasked >= 1 and d.uber_masked >= 1
        assert d.lit_pixels >= 100 and d.occluded_pixels >= 100 and len(d.culled) >= 1 and len(d.not_culled) >= 1


def test_quirk_case_conditions():
    for resx, resy in ((96, 64), (70, 50)):
        assert run("quirk", resx, resy).quirk_lanes >= 1
