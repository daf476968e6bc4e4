"""The transparency continuation under full shading of instanced scenes, the parts that need no GPU
(include/snail_instances_materials_transparency.h): the header as a C contract (plain C, every declared symbol exported and bound), what is
refused before anything touches a device, and the cases of tests/instances_materials_transparency_cases.py against the conditions the GPU
tests rest on, counted by the restatement (tests/instances_materials_transparency_ref.py).  The counts are lower bounds on coverage, not
measurements: if a case misses one, the case changes, not the bound."""
import os
import re
import subprocess

import numpy as np
import pytest

from snail_amd import _lib
from snail_amd import instances_materials as IP
from snail_amd import materials as P
from tests import instances_materials_transparency_cases as C
from tests import instances_materials_transparency_ref as IT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "snail_amd")
T = _lib.INSTANCES_MATERIALS_TRANSPARENCY_SIGNATURES


# ---- the C-ABI ----
def test_signatures_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "snail_instances_materials_transparency.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|void|SnailInstancesMaterials \*)\s*(snail_[a-z_0-9]+)\s*\(", hdr, flags=re.M)))
    assert sorted(T) == declared and len(declared) == 8, declared
    for name in dir(_lib):
        other = getattr(_lib, name)
        if name.endswith("SIGNATURES") and other is not T:
            assert not set(T) & set(other), name
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), "libsnailhip.so does not export " + name
        assert getattr(L, name).argtypes == T[name][1]
    # the arguments of the functions they extend, plus what the header adds
    I, VP = _lib.INSTANCES_MATERIALS_SIGNATURES, _lib._VP
    B, PT = _lib.INSTANCES_MATERIALS_BOUNCE_SIGNATURES, _lib.MATERIALS_TRANSPARENCY_SIGNATURES
    old = I["snail_instances_materials_create"][1]
    assert T["snail_instances_materials_create_transparent"][1] == old[:5] + [VP] + old[5:]
    old = I["snail_instances_materials_shade_packets_dev"][1]
    assert T["snail_instances_materials_shade_packets_transp_dev"][1] == old[:-1] + [VP, VP] + old[-1:]
    old = B["snail_instances_materials_shade_rays_dev"][1]
    assert T["snail_instances_materials_shade_rays_transp_dev"][1] == old[:-1] + [VP, VP] + old[-1:]
    old = PT["snail_materials_continue_packets_dev"][1]
    assert T["snail_instances_materials_continue_packets_dev"][1] == old[:-3] + [VP, VP] + old[-3:]
    for new, plain in (("snail_instances_materials_transparent_dev", "snail_materials_transparent_dev"),
                       ("snail_instances_materials_transparent_packets_dev", "snail_materials_transparent_packets_dev"),
                       ("snail_instances_materials_transparent_image", "snail_materials_transparent_image")):
        assert T[new] == PT[plain]
    assert not re.search(r"#include\s+<|//", hdr)      # plain C: no system header of its own, no C++ comment
    for out in ("bounce", "Tile lists", "4x antialiasing", "tint", "heat-map", "multi-device", "snail_adapter.hpp", "rebuilt on the device"):
        assert out.lower() in hdr.split("#ifndef")[0].lower(), out
    # the older headers keep their functions; only their "NOT here" comments moved on
    for older, table in (("snail_instances_materials.h", I), ("snail_instances_materials_bounce.h", B)):
        text = open(os.path.join(ROOT, "include", older)).read()
        assert "snail_instances_materials_transparency.h" in text.split("#ifndef")[0]
        assert sorted(set(re.findall(r"^(?:int|void|SnailInstancesMaterials \*)\s*(snail_[a-z_0-9]+)\s*\(", text, flags=re.M))) == sorted(table)


def test_header_is_a_c_header(tmp_path):
    exe = str(tmp_path / "instances_materials_transparency_c")
    src = os.path.join(ROOT, "tests", "c", "instances_materials_transparency_c.c")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", src, "-o", exe, "-L" + LIBDIR, "-lsnailhip", "-Wl,-rpath," + LIBDIR])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "C instances materials transparency ABI ok: 8 symbols" in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert set(re.findall(r"ADDR\((snail_[a-z0-9_]+)\)", open(src).read())) == set(T)


# ---- refusals that need no device ----
def test_every_flag_is_refused_before_the_handle_is_looked_at():
    L = _lib.lib()
    cam, amb, img, tr = np.zeros(13, np.float32), np.full(3, 0.1, np.float32), np.full(48, 7, np.uint8), np.full(1, 5, np.uint64)
    for flags in (1, 2, 4, 3, 0x100, -1):       # SNAIL_RENDER_REFLECTIONS, _DEPTH, _AA4, a combination, unknown bits
        assert L.snail_instances_materials_transparent_image(None, _lib.ptr(cam), 4, 4, None, 0, _lib.ptr(amb), flags, _lib.ptr(img), 12, 8, _lib.ptr(tr), None) != 0
        assert b"flags" in L.snail_last_error()
        assert L.snail_instances_materials_transparent_dev(None, _lib.ptr(cam), 4, 4, None, 0, _lib.ptr(amb), flags, _lib.ptr(img), 12, 8, _lib.ptr(tr), None, None) != 0
        assert b"flags" in L.snail_last_error()
        assert L.snail_instances_materials_transparent_packets_dev(None, _lib.ptr(cam), 4, 4, None, 1, None, 0, _lib.ptr(amb), flags, _lib.ptr(img), 8, _lib.ptr(tr), None, None) != 0
        assert b"flags" in L.snail_last_error()
    for depth, word in ((0, b"maxDepth"), (9, b"maxDepth"), (1, b"invalid instanced material set handle"), (8, b"invalid instanced material set handle")):
        assert L.snail_instances_materials_transparent_image(None, _lib.ptr(cam), 4, 4, None, 0, _lib.ptr(amb), 0, _lib.ptr(img), 12, depth, _lib.ptr(tr), None) != 0
        assert word in L.snail_last_error() and b"flags" not in L.snail_last_error()
        assert L.snail_instances_materials_transparent_dev(None, _lib.ptr(cam), 4, 4, None, 0, _lib.ptr(amb), 0, _lib.ptr(img), 12, depth, _lib.ptr(tr), None, None) != 0
        assert word in L.snail_last_error()
        assert L.snail_instances_materials_transparent_packets_dev(None, _lib.ptr(cam), 4, 4, None, 1, None, 0, _lib.ptr(amb), 0, _lib.ptr(img), depth, _lib.ptr(tr), None, None) != 0
        assert word in L.snail_last_error()
    assert L.snail_instances_materials_transparent_dev(None, _lib.ptr(cam), 4, 4, None, 0, _lib.ptr(amb), 0, _lib.ptr(img), 12, 8, None, None, None) != 0
    assert b"counter" in L.snail_last_error()
    assert (img == 7).all() and tr[0] == 5
    assert L.snail_instances_materials_can_select_transparent(None) == -1 and b"handle" in L.snail_last_error()


def aligned(n_bytes, offset=0):
    """a host buffer whose address is 16-byte aligned, plus `offset` (the checks look at addresses alone: nothing is read)"""
    raw = np.zeros(n_bytes + 32, dtype=np.uint8)
    start = (-raw.ctypes.data) % 16 + offset
    return raw[start:start + n_bytes]


def test_the_stages_refuse_bad_buffers_and_take_no_packets_for_no_work():
    L = _lib.lib()
    cam = _lib.ptr(np.zeros(13, np.float32))
    p = [_lib.ptr(aligned(64)) for _ in range(20)]
    odd = _lib.ptr(aligned(64, 4))
    handle = b"invalid instanced material set handle"
    for n in (0, -3):                           # nPackets <= 0: nothing to do, whatever else is given
        assert L.snail_instances_materials_shade_packets_transp_dev(None, cam, 4, 4, None, n, *([None] * 9)) == 0
        assert L.snail_instances_materials_shade_rays_transp_dev(None, n, *([None] * 10)) == 0
        assert L.snail_instances_materials_continue_packets_dev(None, cam, 4, 4, None, n, *([None] * 16)) == 0
    # shade_packets_transp: xy, t, u, v, inst, tri, samples, opacity, sel
    good = p[:9]
    assert L.snail_instances_materials_shade_packets_transp_dev(None, cam, 4, 4, *good[:1], 1, *good[1:], None) != 0 and handle in L.snail_last_error()
    for k in range(9):
        for bad in (None, odd):
            if bad is odd and k in (0, 8):      # the packet list and the selector need no alignment
                continue
            a = list(good); a[k] = bad
            assert L.snail_instances_materials_shade_packets_transp_dev(None, cam, 4, 4, a[0], 1, *a[1:], None) != 0, k
            assert b"null buffer" in L.snail_last_error(), (k, L.snail_last_error())
    assert L.snail_instances_materials_shade_packets_transp_dev(None, None, 4, 4, good[0], 1, *good[1:], None) != 0 and b"camera" in L.snail_last_error()
    # shade_rays_transp: dir, mask (may be null; no alignment), t, bary, inst, tri, samples, opacity, sel
    good = [p[0], None] + p[1:8]
    assert L.snail_instances_materials_shade_rays_transp_dev(None, 1, *good, None) != 0 and handle in L.snail_last_error()
    for k in (0, 2, 3, 4, 5, 6, 7, 8):
        for bad in (None, odd):
            if bad is odd and k == 8:
                continue
            a = list(good); a[k] = bad
            assert L.snail_instances_materials_shade_rays_transp_dev(None, 1, *a, None) != 0, k
            assert b"null buffer" in L.snail_last_error(), (k, L.snail_last_error())
    a = list(good); a[1] = odd
    assert L.snail_instances_materials_shade_rays_transp_dev(None, 1, *a, None) != 0 and handle in L.snail_last_error()
    # continue_packets: xy | origin_in, dir_in, idir_in, t, sel, origin, dir, idir, mask, distance, object, element, bary, order
    prim = [None, None, None] + p[1:12]
    assert L.snail_instances_materials_continue_packets_dev(None, cam, 4, 4, p[0], 1, *prim, None, None) != 0 and handle in L.snail_last_error()
    gen = p[12:15] + p[1:12]
    assert L.snail_instances_materials_continue_packets_dev(None, None, 0, 0, None, 1, *gen, None, None) != 0 and handle in L.snail_last_error()
    for k in range(3, 14):
        for bad in (None, odd):
            if bad is odd and k in (4, 8, 13):  # selector, mask, order words: no 16-byte alignment
                continue
            a = list(gen); a[k] = bad
            assert L.snail_instances_materials_continue_packets_dev(None, None, 0, 0, None, 1, *a, None, None) != 0, k
            assert b"null buffer" in L.snail_last_error(), (k, L.snail_last_error())
    a = list(gen); a[1] = None
    assert L.snail_instances_materials_continue_packets_dev(None, None, 0, 0, None, 1, *a, None, None) != 0 and b"go together" in L.snail_last_error()
    assert L.snail_instances_materials_continue_packets_dev(None, None, 4, 4, p[0], 1, *prim, None, None) != 0 and b"primary level" in L.snail_last_error()
    a = list(gen); a[5] = a[0]
    assert L.snail_instances_materials_continue_packets_dev(None, None, 0, 0, None, 1, *a, None, None) != 0 and b"written over" in L.snail_last_error()


def one_record(mat_index=0):
    return P.pack_shtris(np.zeros((1, 3, 2), np.float32), np.ones((1, 3, 3), np.float32), [mat_index])


def created(materials, textures, transparent, word):
    with pytest.raises(_lib.SnailError) as e:
        IP.create_instanced_set(None, [one_record()], [[0]], materials, textures, transparent)
    assert word in str(e.value), str(e.value)


def test_the_transparent_creator_accepts_what_it_must_and_the_old_one_keeps_its_refusals():
    tex = [P.Texture(np.zeros((4, 4, 3), np.uint8)), P.Texture(np.zeros((8, 2, 3), np.uint8))]
    stopped = "invalid instances handle"        # the host data passed: the missing handle is what stops the call
    created([P.Material.transparent(0, 1)], tex, True, stopped)
    created([P.Material.transparent(1, 0, ndotr=False)], tex, True, stopped)
    for dissolve in (0.5, 1e-6, 0.999, 0.0, 1.0, -1.0, 2.0, float("inf")):
        created([P.Material.uber((1, 1, 1), (1, 1, 1), dissolve)], [], True, stopped)
    created([P.Material.uber((1, 1, 1), (1, 1, 1), float("nan"))], [], True, "NaN")
    created([P.Material.transparent(2, 0)], tex, True, "texture index")
    created([P.Material.transparent(0, 2)], tex, True, "opacity texture index")
    created([P.Material.transparent(0, 0)], [], True, "texture index")
    created([P.Material.simple((1, 1, 1))], [], True, stopped)
    # every other rule of snail_instances_materials_create, with its words
    with pytest.raises(_lib.SnailError) as e:
        IP.create_instanced_set(None, [one_record()], [[3]], [P.Material.simple((1, 1, 1))], [], True)
    assert "map entry" in str(e.value) and "BLAS 0" in str(e.value)
    with pytest.raises(_lib.SnailError) as e:
        IP.create_instanced_set(None, [one_record(2)], [[0]], [P.Material.simple((1, 1, 1))], [], True)
    assert "material index" in str(e.value)
    # snail_instances_materials_create itself: its old texts
    created([P.Material.transparent(0, 1)], tex, False, "is of the transparent kind: transparency under full shading stays with the host renderer")
    created([P.Material.uber((1, 1, 1), (1, 1, 1), 0.5)], [], False, "could select a transparent lane (accepted: dissolve <= 0 or >= 1)")
    created([P.Material.uber((1, 1, 1), (1, 1, 1), 1.0)], [], False, stopped)


# ---- the cases exercise what the GPU tests claim ----
def glass(resx=96, resy=64, **kw):
    return C.reference("glasshouse", resx, resy, **kw)


def all_diags():
    return [glass(*f)[3] for f in C.FRAMES]


def total(f):
    return sum(f(d) for d in all_diags())


def test_frames_are_small():
    assert C.FRAMES == [(96, 64), (70, 50), (64, 48)] and all(rx * ry <= 96 * 64 for rx, ry in C.FRAMES)
    rot, _tr, bi = C.glasshouse_instances()
    assert (bi == 2).sum() == 3 and (bi == 3).sum() == 2 and set(bi.tolist()) == {0, 1, 2, 3}
    panes = rot[bi == 2]
    assert np.array_equal(panes[0], np.eye(3)) and set(np.unique(np.abs(panes[1])).tolist()) == {0.0, 1.0} and not np.array_equal(panes[1], np.eye(3)) and (panes[2] != 0).all()
    op = C.textures()[2][:, :, 0]
    assert (op == 0).any() and (op == 255).any() and ((op > 0) & (op < 255)).any()


@pytest.mark.parametrize("resx,resy", C.FRAMES)
def test_levels_are_reached_and_packets_are_dropped_and_kept(resx, resy):
    d = glass(resx, resy)[3]
    print(C.describe(d))
    assert d.deepest >= 3
    assert d.level_selected[1] >= 256 and d.level_selected[2] >= 64 and d.level_selected[3] >= 16, d.level_selected
    for level in (1, 2):
        kept = d.nested_full.get(level, 0) + d.nested_masked.get(level, 0)
        assert kept >= 1 and (d.nested_none.get(level, 0) >= 1 or (resx, resy) != (96, 64)), (level, d.nested_none, d.nested_full, d.nested_masked)
    assert d.nested_none.get(2, 0) >= 1      # (every frame drops packets at level 2; the 96 x 64 frame, the stage tests', at level 1 as well)
    assert d.continuation_hits >= 256 and d.continuation_misses >= 1
    for level in (1, 2):
        assert len(d.level_hit_slots[level]) >= 2


def test_nested_packets_full_and_masked():
    assert total(lambda d: sum(d.nested_full.values())) >= 1 and total(lambda d: sum(d.nested_masked.values())) >= 8
    d = glass()[3]
    assert sum(d.nested_full.values()) >= 1 and sum(d.nested_masked.values()) >= 8        # the stage tests' frame has both


def test_the_selector_rule_is_exercised():
    d = glass()[3].samples
    assert d.c_overwritten >= 1 and d.c_deselected_lanes >= 1 and d.c_lost_selectable >= 1, (d.c_overwritten, d.c_deselected_lanes, d.c_lost_selectable)
    assert d.c_overwritten_by_opaque_uber >= 1
    assert d.same_tri_two_slots_b >= 1
    assert d.transparent_opaque_lanes >= 1 and d.flagged_opaque_lanes >= d.transparent_opaque_lanes
    assert d.blocks_a_flag >= 8 and d.blocks_b_flag >= 1 and d.blocks_c_flag >= 8 and d.a_transparent >= 8
    assert d.opacity_zero_lanes >= 1
    # a block on two BLASes with one material: over the frames together
    assert total(lambda x: x.samples.two_blas_one_material) >= 1


def test_truncation():
    assert glass(max_depth=2)[2] >= 16 and glass(max_depth=2)[3].deepest == 2
    assert glass(max_depth=8)[2] == 0
    assert (glass(max_depth=2)[0] != glass()[0]).any()


def test_nested_lights_and_pane_shadows():
    d = glass(shadows=True)[3]
    both = [lvl for lvl, ld in d.lights.items() if lvl >= 1 and ld.culled and ld.not_culled]
    assert both, {k: (len(v.culled), len(v.not_culled)) for k, v in d.lights.items()}
    assert d.pane_shadow_lanes >= 64
    assert np.array_equal(glass(shadows=True)[0], glass()[0]) and np.array_equal(glass(shadows=True)[1], glass()[1])      # (counting enters no result)


def test_the_deep_case_nests_behind_its_pane():
    fr, st, trunc, d, _xy, _rec = C.reference("deep", 64, 64)
    assert d.deepest >= 1 and d.level_selected[1] >= 256 and trunc == 0
    assert d.nested_none.get(1, 0) >= 1 and d.lights[1].not_culled
    plain, _ = C.plain_reference("deep", 64, 64, panes=False, opaque=False)
    assert (fr != plain).any(axis=2).sum() >= 100


@pytest.mark.parametrize("resx,resy", C.FRAMES)
def test_invisible_panes_do_not_show(resx, resy):
    """opacity 0 everywhere, SIMPLE materials without N.R behind, no lights: VLerp(transColor, diffuse, 0) is transColor, and that is the
    colour of what lies behind.  The camera was moved until no continuation ray lands across an edge of the backdrop."""
    fr, st, trunc, d, _xy, _rec = C.reference("invisible", resx, resy, lights_key="none")
    plain, pst = C.plain_reference("invisible", resx, resy, lights_key="none", panes=False, opaque=False)
    assert np.array_equal(fr, plain) and trunc == 0
    assert d.level_selected[1] >= 256 and d.deepest >= 2 and (st[:3] > pst[:3]).all()


@pytest.mark.parametrize("mutation", IT.MUTATIONS)
def test_each_mutation_changes_a_frame_or_its_stats(mutation):
    true = glass()
    wrong = glass(mutation=mutation)
    n = int((true[0] != wrong[0]).any(axis=2).sum())
    print("%s: %d pixels differ; stats %s / %s" % (mutation, n, true[1].tolist(), wrong[1].tolist()))
    assert n >= 1 or not np.array_equal(true[1], wrong[1]), mutation


def test_a_set_without_capable_materials_is_the_plain_restatement():
    """the opaque stand-ins through the new restatement: the frame and TreeStats of tests/instances_materials_ref.py, nothing selected"""
    fr, st, trunc, d, _xy, _rec = glass(opaque=True)
    plain, pst = C.plain_reference("glasshouse", 96, 64)
    assert np.array_equal(fr, plain) and np.array_equal(st, pst) and trunc == 0 and d.deepest == 0
