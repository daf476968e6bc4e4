"""The bounce under full shading, the parts that need no GPU: the C-ABI of include/snail_materials_bounce.h as a contract (plain C, every
declared symbol exported and bound, every flag but 0 and SNAIL_RENDER_REFLECTIONS refused before anything touches a device), the test-side
restatement (tests/materials_bounce_ref.py) against the CPU oracle where the two must coincide, and the cases of
tests/materials_bounce_cases.py against the conditions the GPU tests rest on."""
import os
import re
import subprocess

import numpy as np
import pytest

from snail_amd import _lib
from tests import materials_bounce_cases as BK
from tests import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "snail_amd")
MODES = [O.MODE_IEEE, O.MODE_SSE]


def test_signatures_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "snail_materials_bounce.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|int64_t|void)\s*(snail_[a-z_0-9]+)\s*\(", hdr, flags=re.M)))
    from snail_amd._lib import (BVH_FAST_SIGNATURES, HEATMAP_SIGNATURES, INSTANCES_BUILD_SIGNATURES, INSTANCES_SHADE_SIGNATURES, INSTANCES_SIGNATURES,
                                INSTANCES_TILES_SIGNATURES, MATERIALS_BOUNCE_SIGNATURES, MATERIALS_SIGNATURES, SIGNATURES, lib)
    assert sorted(MATERIALS_BOUNCE_SIGNATURES) == declared and len(declared) == 5, declared
    for other in (SIGNATURES, INSTANCES_SIGNATURES, INSTANCES_SHADE_SIGNATURES, INSTANCES_TILES_SIGNATURES, INSTANCES_BUILD_SIGNATURES, BVH_FAST_SIGNATURES,
                  HEATMAP_SIGNATURES, MATERIALS_SIGNATURES):
        assert not set(MATERIALS_BOUNCE_SIGNATURES) & set(other)
    L = lib()
    for name in declared:
        assert hasattr(L, name), "libsnailhip.so does not export " + name
        assert getattr(L, name).argtypes == MATERIALS_BOUNCE_SIGNATURES[name][1]
    # the frame functions take the arguments of the three snail_render_materials_* functions
    for new, old in (("snail_materials_bounce_dev", "snail_render_materials_dev"), ("snail_materials_bounce_packets_dev", "snail_render_materials_packets_dev"),
                     ("snail_materials_bounce_image", "snail_render_materials_image")):
        assert MATERIALS_BOUNCE_SIGNATURES[new] == MATERIALS_SIGNATURES[old]


def test_header_is_a_c_header(tmp_path):
    exe = str(tmp_path / "materials_bounce_c")
    src = os.path.join(ROOT, "tests", "c", "materials_bounce_c.c")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", src, "-o", exe, "-L" + LIBDIR, "-lsnailhip", "-Wl,-rpath," + LIBDIR])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "C materials bounce ABI ok: 5 symbols" in r.stdout, (r.returncode, r.stdout, r.stderr)
    from snail_amd._lib import MATERIALS_BOUNCE_SIGNATURES
    assert set(re.findall(r"ADDR\((snail_[a-z0-9_]+)\)", open(src).read())) == set(MATERIALS_BOUNCE_SIGNATURES)


def test_other_flags_are_refused_before_the_handle_is_looked_at():
    L = _lib.lib()
    cam, amb, img = np.zeros(13, np.float32), np.full(3, 0.1, np.float32), np.full(48, 7, np.uint8)
    for flags in (2, 4, 3, 6, 0x100, -1):       # SNAIL_RENDER_DEPTH, SNAIL_RENDER_AA4, combinations with SNAIL_RENDER_REFLECTIONS, unknown bits
        assert L.snail_materials_bounce_image(None, _lib.ptr(cam), 4, 4, None, 0, _lib.ptr(amb), flags, _lib.ptr(img), 12, None) != 0
        assert b"flags" in L.snail_last_error()
        assert L.snail_materials_bounce_dev(None, _lib.ptr(cam), 4, 4, None, 0, _lib.ptr(amb), flags, _lib.ptr(img), 12, None, None) != 0
        assert b"flags" in L.snail_last_error()
        assert L.snail_materials_bounce_packets_dev(None, _lib.ptr(cam), 4, 4, None, 1, None, 0, _lib.ptr(amb), flags, _lib.ptr(img), None, None) != 0
        assert b"flags" in L.snail_last_error()
    for flags in (0, 1):                        # accepted: the null handle is what stops the call
        assert L.snail_materials_bounce_image(None, _lib.ptr(cam), 4, 4, None, 0, _lib.ptr(amb), flags, _lib.ptr(img), 12, None) != 0
        assert b"flags" not in L.snail_last_error() and b"handle" in L.snail_last_error()
    assert (img == 7).all()


# ---- the restatement against the oracle: the check of it that does not rest on itself ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["degenerate_box", "degenerate_small"])
def test_degenerate_restatement_equals_the_oracle_s_bounce(name, mode):
    """every triangle flat with its plane normal, every material the default: full shading with the bounce is the oracle's simple-shading
    Scene::RayTrace with gVals[7], byte for byte and counter for counter"""
    c = BK.case(name)
    for resx, resy in BK.FRAMES:
        got, gst, _, _, d = BK.reference(name, resx, resy, mode)
        want, wst = c["osc"].render_whitted(c["cam"].as_array13(), resx, resy, c["lights"], mode=mode, reflections=True)
        plain, _ = c["osc"].render_whitted(c["cam"].as_array13(), resx, resy, c["lights"], mode=mode, reflections=False)
        assert np.array_equal(got, want) and got.any(), name
        assert np.array_equal(gst, wst), (gst, wst)
        assert (want != plain).any() and d.mirrored_hits >= 8        # the bounce shows in the frame


# ---- the cases, against what the GPU tests rest on (the restatement's diagnostics, counted per nested call) ----
def diags(names, frame):
    return [BK.reference(n, frame[0], frame[1], O.MODE_IEEE)[4] for n in names]


def test_mirror_case_reaches_branch_a_on_masked_and_unmasked_nested_packets():
    d = BK.reference("mirror", 96, 64, O.MODE_IEEE)[4]
    assert d.packets_masked >= 8 and d.packets_unmasked >= 8, (d.packets_masked, d.packets_unmasked)
    assert d.a_uber_masked >= 8 and d.a_uber_unmasked >= 8, (d.a_uber_masked, d.a_uber_unmasked)       # specular = `specular` / = the sample's diffuse
    assert d.a_tex_masked >= 4 and d.a_tex_mip_above_0 >= 8, (d.a_tex_masked, d.a_tex_mip_above_0)
    assert d.nested.uber_masked >= 8 * 16 and d.nested.uber_unmasked >= 8 * 16
    assert d.mirrored_misses >= 8 and d.mirrored_hits >= 8
    assert len(d.nested.culled) >= 1 and len(d.nested.not_culled) >= 1, (d.nested.culled, d.nested.not_culled)
    assert d.nested.quirk_lanes >= 1                                   # lane 0 of a nested quad missed beside a hit of triangle 0
    d70 = BK.reference("mirror", 70, 50, O.MODE_IEEE)[4]
    assert d70.packets_masked >= 8 and d70.a_uber_masked >= 8 and d70.a_tex_mip_above_0 >= 4 and d70.mirrored_misses >= 8
    assert len(d70.nested.culled) >= 1 and len(d70.nested.not_culled) >= 1


@pytest.mark.parametrize("frame", BK.FRAMES)
def test_the_cases_together_reach_every_nested_branch(frame):
    ds = diags(["mirror", "large", "small", "quirk"], frame)
    total = lambda f: sum(f(d) for d in ds)      # noqa: E731
    assert total(lambda d: d.nested.blocks_c) >= 8
    assert total(lambda d: d.nested.blocks_masked_one) >= 8
    assert total(lambda d: d.mirrored_misses) >= 8
    assert total(lambda d: d.nested.occluded_pixels) >= 8 and total(lambda d: d.nested.lit_pixels) >= 8
    assert total(lambda d: len(d.nested.culled)) >= 1 and total(lambda d: len(d.nested.not_culled)) >= 1
    assert total(lambda d: d.packets_masked) >= 8 and total(lambda d: d.packets_unmasked) >= 8


def test_nested_branch_b_with_one_material():
    """per-quad nested blocks that end in the unmasked Shade of ONE material (:301-308): rare among mirrored rays -- the 96 x 64 frames of
    `mirror` and `large` reach it 8 times together"""
    ds = diags(["mirror", "large"], (96, 64))
    assert sum(d.nested.blocks_b for d in ds) >= 8, [d.nested.blocks_b for d in ds]


def test_large_case_unmasked_nested_packets_and_occlusion():
    for frame in BK.FRAMES:
        d = BK.reference("large", frame[0], frame[1], O.MODE_IEEE)[4]
        assert d.packets_unmasked >= 8 and d.a_unmasked >= 8 and d.a_tex_mip_above_0 >= 8
        assert d.nested.occluded_pixels >= 8 and d.nested.lit_pixels >= 8
