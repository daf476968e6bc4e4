"""The bounce under full shading of instanced scenes, the parts that need no GPU (include/snail_instances_materials_bounce.h): the header as a
C contract (plain C, every declared symbol exported and bound), what is refused before anything touches a device, and the cases of
tests/instances_materials_bounce_cases.py against the conditions the GPU tests rest on, counted by the restatement
(tests/instances_materials_bounce_ref.py).  The counts are lower bounds on coverage, not measurements: if a case misses one, the case
changes, not the bound."""
import os
import re
import subprocess

import numpy as np
import pytest

from snail_amd import _lib
from tests import dbvh_shade_ref as S
from tests import instances_materials_bounce_cases as BK
from tests import instances_materials_bounce_ref as IB
from tests import instances_materials_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "snail_amd")


# ---- the C-ABI ----
def test_signatures_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "snail_instances_materials_bounce.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|void)\s*(snail_[a-z_0-9]+)\s*\(", hdr, flags=re.M)))
    T = _lib.INSTANCES_MATERIALS_BOUNCE_SIGNATURES
    assert sorted(T) == declared and len(declared) == 5, declared
    for other in (_lib.SIGNATURES, _lib.INSTANCES_SIGNATURES, _lib.INSTANCES_SHADE_SIGNATURES, _lib.INSTANCES_TILES_SIGNATURES, _lib.INSTANCES_BUILD_SIGNATURES,
                  _lib.BVH_FAST_SIGNATURES, _lib.HEATMAP_SIGNATURES, _lib.MATERIALS_SIGNATURES, _lib.MATERIALS_BOUNCE_SIGNATURES, _lib.MATERIALS_TILES_SIGNATURES,
                  _lib.MATERIALS_TRANSPARENCY_SIGNATURES, _lib.MATERIALS_TREE_SIGNATURES, _lib.MATERIALS_HEAT_SIGNATURES, _lib.MATERIALS_DYNAMIC_SIGNATURES,
                  _lib.INSTANCES_MATERIALS_SIGNATURES):
        assert not set(T) & set(other)
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), "libsnailhip.so does not export " + name
        assert getattr(L, name).argtypes == T[name][1]
    # the frame functions take the arguments of the three snail_instances_render_materials_* functions
    for new, old in (("snail_instances_materials_bounce_dev", "snail_instances_render_materials_dev"),
                     ("snail_instances_materials_bounce_packets_dev", "snail_instances_render_materials_packets_dev"),
                     ("snail_instances_materials_bounce_image", "snail_instances_render_materials_image")):
        assert T[new] == _lib.INSTANCES_MATERIALS_SIGNATURES[old]
    assert not re.search(r"#include\s+<|//", hdr)      # plain C: no system header of its own, no C++ comment
    # the older header keeps its functions; only its "NOT here" comment moved on
    old = open(os.path.join(ROOT, "include", "snail_instances_materials.h")).read()
    assert "snail_instances_materials_bounce.h" in old.split("#ifndef")[0] and "_bounce" not in old.split("#ifndef")[1]


def test_header_is_a_c_header(tmp_path):
    exe = str(tmp_path / "instances_materials_bounce_c")
    src = os.path.join(ROOT, "tests", "c", "instances_materials_bounce_c.c")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", src, "-o", exe, "-L" + LIBDIR, "-lsnailhip", "-Wl,-rpath," + LIBDIR])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "C instances materials bounce ABI ok: 5 symbols" in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert set(re.findall(r"ADDR\((snail_[a-z0-9_]+)\)", open(src).read())) == set(_lib.INSTANCES_MATERIALS_BOUNCE_SIGNATURES)


# ---- refusals that need no device ----
def test_other_flags_are_refused_before_the_handle_is_looked_at():
    L = _lib.lib()
    cam, amb, img = np.zeros(13, np.float32), np.full(3, 0.1, np.float32), np.full(48, 7, np.uint8)
    for flags in (2, 4, 3, 6, 0x100, -1):       # SNAIL_RENDER_DEPTH, SNAIL_RENDER_AA4, combinations with SNAIL_RENDER_REFLECTIONS, unknown bits
        assert L.snail_instances_materials_bounce_image(None, _lib.ptr(cam), 4, 4, None, 0, _lib.ptr(amb), flags, _lib.ptr(img), 12, None) != 0
        assert b"flags" in L.snail_last_error()
        assert L.snail_instances_materials_bounce_dev(None, _lib.ptr(cam), 4, 4, None, 0, _lib.ptr(amb), flags, _lib.ptr(img), 12, None, None) != 0
        assert b"flags" in L.snail_last_error()
        assert L.snail_instances_materials_bounce_packets_dev(None, _lib.ptr(cam), 4, 4, None, 1, None, 0, _lib.ptr(amb), flags, _lib.ptr(img), None, None) != 0
        assert b"flags" in L.snail_last_error()
    for flags in (0, 1):                        # accepted: the null handle is what stops the call
        assert L.snail_instances_materials_bounce_image(None, _lib.ptr(cam), 4, 4, None, 0, _lib.ptr(amb), flags, _lib.ptr(img), 12, None) != 0
        assert b"flags" not in L.snail_last_error() and b"invalid instanced material set handle" in L.snail_last_error()
        assert L.snail_instances_materials_bounce_dev(None, _lib.ptr(cam), 4, 4, None, 0, _lib.ptr(amb), flags, _lib.ptr(img), 12, None, None) != 0
        assert b"invalid instanced material set handle" in L.snail_last_error()
        assert L.snail_instances_materials_bounce_packets_dev(None, _lib.ptr(cam), 4, 4, None, 1, None, 0, _lib.ptr(amb), flags, _lib.ptr(img), None, None) != 0
        assert b"invalid instanced material set handle" in L.snail_last_error()
    assert (img == 7).all()


def aligned(n_bytes, offset=0):
    """a host buffer whose address is 16-byte aligned, plus `offset` (the checks look at addresses alone: nothing is read)"""
    raw = np.zeros(n_bytes + 32, dtype=np.uint8)
    start = (-raw.ctypes.data) % 16 + offset
    return raw[start:start + n_bytes]


def test_the_stages_refuse_bad_buffers_and_take_no_packets_for_no_work():
    L = _lib.lib()
    cam = np.zeros(13, np.float32)
    bufs = [aligned(64) for _ in range(12)]
    p = [_lib.ptr(b) for b in bufs]
    odd = _lib.ptr(aligned(64, 4))
    # nPackets <= 0: nothing to do, whatever else is given
    for n in (0, -3):
        assert L.snail_instances_materials_shade_rays_dev(None, n, None, None, None, None, None, None, None, None) == 0
        assert L.snail_instances_materials_mirror_packets_dev(None, _lib.ptr(cam), 4, 4, None, n, *([None] * 12)) == 0
    # sound buffers: the null handle is what stops the call
    good_rays = [p[0], None, p[1], p[2], p[3], p[4], p[5]]
    assert L.snail_instances_materials_shade_rays_dev(None, 1, *good_rays, None) != 0
    assert b"invalid instanced material set handle" in L.snail_last_error()
    good_mirror = [p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10]]      # xy, t, samples, origin, dir, idir, mask, distance, object, element, bary
    assert L.snail_instances_materials_mirror_packets_dev(None, _lib.ptr(cam), 4, 4, p[0], 1, *good_mirror[1:], None, None) != 0
    assert b"invalid instanced material set handle" in L.snail_last_error()
    # every buffer null, then misaligned, in turn (the mask of shade_rays may be null: every lane selected; a mask needs no alignment)
    for k in (0, 2, 3, 4, 5, 6):
        for bad in (None, odd):
            a = list(good_rays); a[k] = bad
            assert L.snail_instances_materials_shade_rays_dev(None, 1, *a, None) != 0, k
            assert b"null buffer" in L.snail_last_error(), (k, L.snail_last_error())
    a = list(good_rays); a[1] = odd
    assert L.snail_instances_materials_shade_rays_dev(None, 1, *a, None) != 0 and b"handle" in L.snail_last_error()
    for k in range(1, 11):
        for bad in (None, odd):
            if k == 6 and bad is odd:
                continue
            a = list(good_mirror); a[k] = bad
            assert L.snail_instances_materials_mirror_packets_dev(None, _lib.ptr(cam), 4, 4, p[0], 1, *a[1:], None, None) != 0, k
            assert b"null buffer" in L.snail_last_error(), (k, L.snail_last_error())
    assert L.snail_instances_materials_mirror_packets_dev(None, _lib.ptr(cam), 4, 4, None, 1, *good_mirror[1:], None, None) != 0 and b"null buffer" in L.snail_last_error()
    assert L.snail_instances_materials_mirror_packets_dev(None, None, 4, 4, p[0], 1, *good_mirror[1:], None, None) != 0 and b"camera" in L.snail_last_error()
    assert L.snail_instances_materials_mirror_packets_dev(None, _lib.ptr(cam), 0, 4, p[0], 1, *good_mirror[1:], None, None) != 0 and b"resolution" in L.snail_last_error()


# ---- the restatement where it must coincide with another ----
@pytest.mark.parametrize("resx,resy", BK.FRAMES)
def test_the_degenerate_set_equals_the_simple_shading_restatement_with_reflections(resx, resy):
    """every map entry -1 and every record flat with the triangle's plane normal: dbvh_shade_ref.ShadeRef's frame with color (1, 1, 1) and
    reflections, byte for byte, and equal TreeStats -- the check of the restatement that does not rest on itself"""
    c = BK.case("degenerate")
    frame, st, _, _, d = BK.reference("degenerate", resx, resy)
    want, wst = S.ShadeRef(c["ref"]).render(c["cams"][resx].as_array13(), resx, resy, c["lights"], color=(1.0, 1.0, 1.0), reflections=True)
    assert np.array_equal(frame, want) and np.array_equal(st, wst), (st, wst)
    assert (frame != BK.plain_reference("degenerate", resx, resy)[0]).any() and d.mirrored_hits >= 256


# ---- the cases exercise what the GPU tests claim (over the cases together) ----
def diags():
    return [(name, BK.reference(name, rx, ry)[4]) for name, rx, ry in BK.ALL]


def total(f):
    return sum(f(d) for _, d in diags())


def test_frames_are_small():
    assert all(rx * ry <= 96 * 64 for _, rx, ry in BK.ALL) and ("deep", 64, 64) in BK.ALL
    assert {n for n, _, _ in BK.ALL} == {"main", "degenerate", "updated", "quirk", "deep", "mirror"}      # ONE case more than instances_materials_cases has


def test_mirrored_lanes_hit_several_slots_under_general_and_exact_rotations():
    assert total(lambda d: d.mirrored_hits) >= 256
    d = BK.reference("main", 96, 64)[4]
    ref = BK.case("main")["ref"]
    slots = {s for s, n in d.nested_slots.items() if n >= 1}
    assert len(slots) >= 3, d.nested_slots
    rots = {s: ref.xf[s][:9].reshape(3, 3) for s in slots}
    general = [s for s, r in rots.items() if (r != 0).all()]
    exact = [s for s, r in rots.items() if not np.array_equal(r, np.eye(3)) and set(np.unique(np.abs(r)).tolist()) <= {0.0, 1.0}]
    assert general and exact, (general, exact)
    assert d.nested.rotated_lanes >= 100


def test_nested_packets_and_blocks():
    assert total(lambda d: d.packets_masked) >= 8 and total(lambda d: d.packets_unmasked) >= 8
    # branch (a) with the UBER material on masked AND on unmasked nested packets: specular = `specular` / = the sample's diffuse
    assert total(lambda d: d.a_uber_masked) >= 1 and total(lambda d: d.a_uber_unmasked) >= 1
    m = BK.reference("mirror", 96, 64)[4]
    assert m.a_uber_masked >= 8 and m.a_uber_unmasked >= 8, (m.a_uber_masked, m.a_uber_unmasked)
    assert total(lambda d: d.multi_slot_blocks + d.multi_slot_quads) >= 1
    assert BK.reference("main", 96, 64)[4].multi_slot_quads >= 8
    assert total(lambda d: d.nested.blocks_a) >= 8 and total(lambda d: d.nested.blocks_b) >= 8 and total(lambda d: d.nested.blocks_c) >= 8
    assert total(lambda d: d.nested.blocks_masked_one) >= 8


def test_the_nested_quirk_is_taken():
    """(slot 0, triId 0) beside a lane 0 that is not hit, in a NESTED quad.  The `quirk` case's own mirrored rays do not reach it (28 nested
    hits in all): the `mirror` case's third instance is there for it."""
    assert total(lambda d: d.nested.quirk_lanes) >= 1
    assert BK.reference("mirror", 96, 64)[4].nested.quirk_lanes >= 1 and BK.reference("mirror", 70, 50)[4].nested.quirk_lanes >= 1
    assert int(BK.case("mirror")["ref"].bi[0]) == 1 and np.array_equal(BK.case("mirror")["ref"].xf[0][:9].reshape(3, 3), K.ROT90Y)
    assert BK.reference("quirk", 48, 32)[4].primary.quirk_lanes >= 1          # (the primary quirk is that case's, as before)


def test_nested_lights():
    culled = set().union(*[{(name, p, n) for p, n in d.nested.culled} for name, d in diags()])
    kept = set().union(*[{(name, p, n) for p, n in d.nested.not_culled} for name, d in diags()])
    lights_both = {(name, n) for name, _, n in culled} & {(name, n) for name, _, n in kept}
    assert lights_both, (len(culled), len(kept))            # a nested light culled for some packets and kept for others
    assert total(lambda d: d.nested.occluded_pixels) >= 64
    assert total(lambda d: d.nested.lit_pixels) >= 64


@pytest.mark.parametrize("name,resx,resy", BK.ALL)
def test_the_bounce_shows_in_every_frame(name, resx, resy):
    frame, st, _, _, d = BK.reference(name, resx, resy)
    plain, pst = BK.plain_reference(name, resx, resy)
    assert (frame != plain).any(axis=2).sum() >= 100 and (st[:3] > pst[:3]).all(), (st, pst)
    assert d.mirrored_lanes == d.primary.hit_pixels


@pytest.mark.parametrize("mutation", IB.MUTATIONS)
def test_each_mutation_changes_a_frame(mutation):
    """the restatement without Transform on the nested records / with nested equalities on triId alone / with the primary normal under the
    nested lights gives another frame: the comparisons of the GPU tests can fail"""
    true = BK.reference("main", 96, 64)[0]
    wrong = BK.reference("main", 96, 64, mutation=mutation)[0]
    n = int((true != wrong).any(axis=2).sum())
    assert n >= 1, mutation
