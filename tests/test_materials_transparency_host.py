"""Transparent materials under full shading, the parts that need no GPU: the C-ABI of include/snail_materials_transparency.h as a contract (plain
C, every declared symbol exported and bound), the creators' refusals (judged before a scene or a device is looked at), the Python binding, and
the inputs of tests/materials_transparency_cases.py against the conditions the GPU tests rest on, on the restatement's diagnostics alone."""
import os
import re
import subprocess

import numpy as np
import pytest

from snail_amd import _lib
from snail_amd import materials as P
from tests import materials_ref as M
from tests import materials_synth as Y
from tests import materials_transparency_cases as TK
from tests import materials_transparency_ref as T
from tests import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "snail_amd")
MODES = [O.MODE_IEEE, O.MODE_SSE]


def test_signatures_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "snail_materials_transparency.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|int64_t|void|SnailMaterials \*)\s*(snail_[a-z_0-9]+)\s*\(", hdr, flags=re.M)))
    from snail_amd._lib import (BVH_FAST_SIGNATURES, HEATMAP_SIGNATURES, INSTANCES_BUILD_SIGNATURES, INSTANCES_SHADE_SIGNATURES, INSTANCES_SIGNATURES,
                                INSTANCES_TILES_SIGNATURES, MATERIALS_BOUNCE_SIGNATURES, MATERIALS_SIGNATURES, MATERIALS_TILES_SIGNATURES,
                                MATERIALS_TRANSPARENCY_SIGNATURES, SIGNATURES, lib)
    assert sorted(MATERIALS_TRANSPARENCY_SIGNATURES) == declared and len(declared) == 8, declared
    for other in (SIGNATURES, INSTANCES_SIGNATURES, INSTANCES_SHADE_SIGNATURES, INSTANCES_TILES_SIGNATURES, INSTANCES_BUILD_SIGNATURES, BVH_FAST_SIGNATURES,
                  HEATMAP_SIGNATURES, MATERIALS_SIGNATURES, MATERIALS_BOUNCE_SIGNATURES, MATERIALS_TILES_SIGNATURES):
        assert not set(MATERIALS_TRANSPARENCY_SIGNATURES) & set(other)
    L = lib()
    for name in declared:
        assert hasattr(L, name), "libsnailhip.so does not export " + name
        assert getattr(L, name).argtypes == MATERIALS_TRANSPARENCY_SIGNATURES[name][1]
    S, B = MATERIALS_TRANSPARENCY_SIGNATURES, MATERIALS_BOUNCE_SIGNATURES
    # the creator: snail_materials_create's arguments with the opacity maps before the textures; the sample stages: the existing ones' arguments
    # with opacity and selector before the stream
    old = MATERIALS_SIGNATURES["snail_materials_create"][1]
    assert S["snail_materials_create_transparent"] == (MATERIALS_SIGNATURES["snail_materials_create"][0], old[:7] + [_lib._VP] + old[7:])
    for new, (res, args) in (("snail_materials_shade_packets_transp_dev", MATERIALS_SIGNATURES["snail_materials_shade_packets_dev"]),
                             ("snail_materials_shade_rays_transp_dev", B["snail_materials_shade_rays_dev"])):
        assert S[new] == (res, args[:-1] + [_lib._VP, _lib._VP] + args[-1:])
    # the frames: the arguments of the snail_render_materials_* functions with maxDepth and the truncated-lane counter before the stats
    for new, old, at in (("snail_materials_transparent_dev", "snail_render_materials_dev", -2), ("snail_materials_transparent_packets_dev", "snail_render_materials_packets_dev", -2),
                         ("snail_materials_transparent_image", "snail_render_materials_image", -1)):
        res, args = MATERIALS_SIGNATURES[old]
        assert S[new] == (res, args[:at] + [_lib._I, _lib._VP] + args[at:])


def test_header_is_a_c_header(tmp_path):
    exe = str(tmp_path / "materials_transparency_c")
    src = os.path.join(ROOT, "tests", "c", "materials_transparency_c.c")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", src, "-o", exe, "-L" + LIBDIR, "-lsnailhip", "-Wl,-rpath," + LIBDIR])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "C materials transparency ABI ok: 8 symbols" in r.stdout, (r.returncode, r.stdout, r.stderr)
    from snail_amd._lib import MATERIALS_TRANSPARENCY_SIGNATURES
    assert set(re.findall(r"ADDR\((snail_[a-z0-9_]+)\)", open(src).read())) == set(MATERIALS_TRANSPARENCY_SIGNATURES)


def create(materials, textures, transparent):
    """a creator over one record and a NULL scene -> the refusal's text (validation comes before the scene is looked at)"""
    sh = np.zeros((1, 64), dtype=np.uint8)
    with pytest.raises(_lib.SnailError) as e:
        P.create_set(None, sh, [0 if materials else -1], materials, textures, transparent)
    return str(e.value)


def test_the_creators_refusals_need_no_device():
    tex = [P.Texture(np.zeros((2, 2, 3), dtype=np.uint8)), P.Texture(np.zeros((4, 2, 3), dtype=np.uint8))]
    # the old creator refuses exactly what it refused
    assert "transparent kind" in create([P.Material.transparent()], tex, False)
    assert "could select a transparent lane" in create([P.Material.uber((1, 1, 1), (0, 0, 0), 0.5)], tex, False)
    assert "could select a transparent lane" in create([P.Material.uber((1, 1, 1), (0, 0, 0), float("nan"))], tex, False)
    for ok in (P.Material.uber((1, 1, 1), (0, 0, 0), 0.0), P.Material.uber((1, 1, 1), (0, 0, 0), 1.0), P.Material.uber((1, 1, 1), (0, 0, 0), -2.0)):
        assert "invalid scene handle" in create([ok], tex, False)
    # the new creator accepts both kinds (the NULL scene is what stops the call), validates both texture indices, and keeps refusing a NaN
    for ok in (P.Material.transparent(), P.Material.transparent(1, 0, False), P.Material.transparent(0, 1), P.Material.uber((1, 1, 1), (0, 0, 0), 0.5),
               P.Material.uber((1, 1, 1), (0, 0, 0), 7.0), P.Material.simple((1, 1, 1)), P.Material.textured(1)):
        msg = create([ok], tex, True)
        assert "snail_materials_create_transparent" in msg and "invalid scene handle" in msg, msg
    assert "texture index 2 outside" in create([P.Material.transparent(2, 0)], tex, True)
    assert "opacity texture index 2 outside" in create([P.Material.transparent(0, 2)], tex, True)
    assert "opacity texture index -1 outside" in create([P.Material.transparent(0, -1)], tex, True)
    assert "texture index" in create([P.Material.transparent()], [], True)
    assert "NaN dissolve" in create([P.Material.uber((1, 1, 1), (0, 0, 0), float("nan"))], tex, True)
    # an infinite dissolve is accepted by both creators, as it was by the old one (+inf: flagged, never selected; -inf: not flagged)
    for d in (float("inf"), float("-inf")):
        for transparent in (False, True):
            assert "invalid scene handle" in create([P.Material.uber((1, 1, 1), (0, 0, 0), d)], tex, transparent)
    assert "unknown kind" in create([P.Material(4)], tex, True)
    assert "texture index 5 outside" in create([P.Material.textured(5)], tex, True)


def test_null_handles_are_refused_by_name():
    L = _lib.lib()
    assert L.snail_materials_can_select_transparent(None) == -1 and b"handle" in L.snail_last_error()
    cam = np.zeros(13, np.float32)
    assert L.snail_materials_shade_packets_transp_dev(None, _lib.ptr(cam), 4, 4, None, 1, None, None, None, None, None, None, None, None) != 0
    assert b"snail_materials_shade_packets_transp_dev" in L.snail_last_error()
    assert L.snail_materials_shade_rays_transp_dev(None, 1, None, None, None, None, None, None, None, None, None, None) != 0
    assert b"snail_materials_shade_rays_transp_dev" in L.snail_last_error()
    assert L.snail_materials_continue_packets_dev(None, _lib.ptr(cam), 4, 4, None, 1, *([None] * 14)) != 0
    assert b"snail_materials_continue_packets_dev" in L.snail_last_error()


def test_python_binding():
    m = P.Material.transparent()
    assert int(m.rec["kind"]) == P.KIND_TRANSPARENT and int(m.rec["texture"]) == 0 and m.opacity_texture == 0 and int(m.rec["ndotr"]) == 1
    m = P.Material.transparent(texture=3, opacity_texture=5, ndotr=False)
    assert int(m.rec["texture"]) == 3 and m.opacity_texture == 5 and int(m.rec["ndotr"]) == 0
    for name in ("can_select_transparent", "shade_packets_transp", "shade_rays_transp", "continue_packets", "render_transparent", "render_transparent_packets",
                 "render_transparent_image_host"):
        assert hasattr(P.MaterialSet, name)


# ---- the inputs of the GPU tests, on the restatement alone ----
def test_the_material_lists():
    ds = TK.descs()
    assert len(ds) == len(Y.synth().descs) and sum(d[0] == "transp" for d in ds) == 6 and sum(d[0] == "tex" for d in ds) == 4
    mats = TK.ref_materials(ds)
    assert sum(T.flagged(m) for m in mats) == 8 and sum(T.can_select(m) for m in mats) == 7
    assert any(m.kind == M.UBER and T.flagged(m) and not T.can_select(m) for m in mats)           # UBER 1.0
    assert not any(T.can_select(m) or m.kind == M.TRANSPARENT for m in TK.ref_materials(TK.descs_opaque()))
    # an opacity map of 255 everywhere samples to exactly 1, one of 0 to exactly 0
    tx = TK.reference().ref.textures
    z = np.zeros((1, 4), dtype=np.float32)
    uv = np.array([[0.1, 0.5, 0.77, 0.999]], dtype=np.float32)
    assert (tx[TK.TEX_OPAQUE].sample(uv, uv, z, z)[0] == np.float32(1.0)).all() and (tx[TK.TEX_CLEAR].sample(uv, uv, z, z)[0] == 0).all()


@pytest.mark.parametrize("mode", MODES)
def test_conditions_of_the_primary_list(mode):
    want, d = TK.expected_primary(mode)
    print(TK.describe(d))
    TK.check_conditions(d, False)
    assert np.isfinite(want["samples"]).all() and (want["opacity"] >= 0).all() and (want["opacity"] <= 1).all()


def test_conditions_of_the_generic_list():
    want, d = TK.expected_generic()
    print(TK.describe(d))
    TK.check_conditions(d, True)
    assert d.packets_some >= 16


@pytest.mark.parametrize("generic", [False, True])
def test_a_list_without_capable_materials_is_the_existing_restatement(generic):
    """the restatement of this pull request against the two it is composed with: with opaque stand-ins (TEX for TRANSPARENT, UBER 0 for UBER 0.5)
    the nine planes are MaterialsRef.samples' / BounceRef.samples_rays', and nothing is selected"""
    from tests import materials_bounce_ref as B
    s = Y.synth()
    tr = TK.reference(opaque=True)
    got, d = TK.expected_generic(True) if generic else TK.expected_primary(O.MODE_IEEE, True)
    assert d.selected_lanes == 0 and not got["sel"].any()
    br, bd, md = B.BounceRef(tr.ref), B.BounceDiag(), M.Diag()
    xy = s.packet_xy()
    for p in range(0, Y.N_PACKETS, 3):
        pk = s.packet(p, generic)
        if generic:
            _, nrm, diff, spec = br.samples_rays(pk["dirs"], pk["t"], Y.clamp_ids(pk["tri"], s.n), pk["bary"], pk["bits"], bd)
        else:
            _, nrm, diff, spec = tr.ref.samples(Y.primary_dirs(int(xy[p, 0]), int(xy[p, 1]), O.MODE_IEEE), pk["t"], Y.clamp_ids(pk["tri"], s.n), pk["bary"], md)
        assert Y.to_planes(nrm, diff, spec).tobytes() == got["samples"][p].tobytes(), p
    # UBER writes its dissolve into the opacity plane whether or not it is flagged: dissolve 1.0 is there, and only there
    assert set(np.unique(got["opacity"]).tolist()) == {0.0, 1.0}


@pytest.mark.parametrize("generic", [False, True])
def test_conditions_of_the_generator_s_inputs(generic):
    c = TK.continue_inputs()
    want, selected = TK.expected_continue(O.MODE_IEEE, generic)
    hit = c["t"] < np.float32(np.inf)
    assert (c["sel"] & ~hit).sum() >= 256                       # bits on lanes that missed: dropped
    assert (want["mask"][0] == 15).all()                        # a packet that goes as RayGroup<0, 0>
    assert (want["order"] == -1).sum() >= 5 and (want["order"] >= 0).sum() >= 8 and (want["order"][want["order"] >= 0] == np.flatnonzero(want["order"] >= 0)).all()
    assert any((want["order"][p] == -1) and hit[p].any() for p in range(len(hit)))      # lanes hit, no bit set: no nested call
    assert selected >= 1024 and np.isfinite(want["origin"]).all()
    on = (want["distance"] == np.float32(np.inf))
    assert int(on.sum()) == selected
    if generic:                                                 # idir is handed on, not computed
        assert np.array_equal(want["idir"].transpose(0, 1, 3, 2)[on], c["idir"].transpose(0, 1, 3, 2)[on])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", TK.SWAPPED)
def test_conditions_of_the_swapped_cases(name, mode):
    """what the two-level GPU test rests on, on the restatement with the oracle's walks alone: packets that nest and packets that do not, a
    packet that goes as RayGroup<0, 0>, continuation lanes that hit and that miss, and in `small` a second selection at level 1"""
    levels, stats, xy, d = TK.swapped_descent(name, mode)
    l0, l1, l2 = levels
    inf = np.float32(np.inf)
    c, tr = TK.swapped_case(name)
    assert sum(T.can_select(m) for m in tr.ref.materials) >= 1 and any(m.kind == M.TRANSPARENT for m in tr.ref.materials)
    assert 8 <= len(l1["packets"]) < len(xy) == 20
    assert (l1["cont"]["mask"] == 15).all(axis=1).any()
    assert (l1["dist"] < inf).sum() >= 1024 and (l1["dist"] == inf).sum() >= 64
    assert int(np.unpackbits(l0["sel"]).sum()) == int((l1["cont"]["distance"] == inf).sum()) >= 2048
    if name == "small":
        assert (l2["cont"]["order"] >= 0).sum() >= 4 and (l2["cont"]["order"] == -1).sum() >= 4
        assert d.c_overwritten_by_opaque_uber >= 8 and d.flagged_opaque_lanes >= 64      # UBER 1.0 beside TRANSPARENT in one block
    assert stats[2] > 256 * len(xy) and stats[0] > 0


# ---- frames ----
def test_frame_functions_judge_flags_and_depth_before_the_handle():
    L = _lib.lib()
    cam, amb, img, tr = np.zeros(13, np.float32), np.full(3, 0.1, np.float32), np.full(48, 7, np.uint8), np.zeros(1, np.uint64)
    for flags in (1, 2, 4, 0x100, -1):          # SNAIL_RENDER_REFLECTIONS among them
        assert L.snail_materials_transparent_image(None, _lib.ptr(cam), 4, 4, None, 0, _lib.ptr(amb), flags, _lib.ptr(img), 12, 8, _lib.ptr(tr), None) != 0
        assert b"flags" in L.snail_last_error()
        assert L.snail_materials_transparent_dev(None, _lib.ptr(cam), 4, 4, None, 0, _lib.ptr(amb), flags, _lib.ptr(img), 12, 8, _lib.ptr(tr), None, None) != 0
        assert b"flags" in L.snail_last_error()
        assert L.snail_materials_transparent_packets_dev(None, _lib.ptr(cam), 4, 4, None, 1, None, 0, _lib.ptr(amb), flags, _lib.ptr(img), 8, _lib.ptr(tr), None, None) != 0
        assert b"flags" in L.snail_last_error()
    for depth in (0, -1, 9):
        assert L.snail_materials_transparent_image(None, _lib.ptr(cam), 4, 4, None, 0, _lib.ptr(amb), 0, _lib.ptr(img), 12, depth, _lib.ptr(tr), None) != 0
        assert b"maxDepth" in L.snail_last_error()
    assert L.snail_materials_transparent_image(None, _lib.ptr(cam), 4, 4, None, 0, _lib.ptr(amb), 0, _lib.ptr(img), 12, 8, None, None) != 0
    assert b"truncated" in L.snail_last_error()
    for depth in (1, 8):                        # accepted: the null handle is what stops the call
        assert L.snail_materials_transparent_image(None, _lib.ptr(cam), 4, 4, None, 0, _lib.ptr(amb), 0, _lib.ptr(img), 12, depth, _lib.ptr(tr), None) != 0
        assert b"handle" in L.snail_last_error()
    assert (img == 7).all() and tr[0] == 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("resx,resy", TK.PANES_FRAMES)
def test_panes_exercises_everything_the_frames_rest_on(resx, resy, mode):
    """conditions on the INPUTS, on the restatement alone: every diagnostic of tests/materials_transparency_ref.py occurs in `panes`"""
    frame, stats, trunc, d, xy = TK.panes_frame(resx, resy, mode)
    print(TK.describe_frame(d))
    s = d.samples
    assert d.deepest >= 3 and trunc == 0 and d.truncated == 0                       # the recursion ends by itself within max_depth = 8
    assert TK.panes_frame(resx, resy, mode, 2)[2] > 0                               # ... and is cut at max_depth = 2
    for level in (1, 2):
        assert d.nested_masked.get(level, 0) >= 1 and d.nested_none.get(level, 0) >= 1, level
    assert d.nested_full.get(1, 0) >= 1                                             # the centre pane: whole packets as RayGroup<0, 0>
    assert d.nested_none.get(d.deepest + 1, 0) >= 1
    assert s.blocks_a_flag >= 8 and s.blocks_b_flag >= 4 and s.blocks_c_flag >= 32 and s.a_transparent >= 4
    assert s.c_overwritten >= 16 and s.c_overwritten_by_opaque_uber >= 8 and s.c_lost_selectable >= 16
    assert s.c_overwritten - s.c_overwritten_by_opaque_uber >= 8                       # ... and by UBER 0.5 / TRANSPARENT, counted apart
    # UBER with dissolve >= 1 (and only that) de-selects a TRANSPARENT neighbour's lanes among the primary hits AND at a nested level
    assert d.opaque_uber_overwrites.get(0, 0) >= 4 and sum(v for k, v in d.opaque_uber_overwrites.items() if k >= 1) >= 4, d.opaque_uber_overwrites
    assert s.flagged_opaque_lanes >= 64 and s.opacity_zero_lanes >= 32
    assert d.continuation_misses >= 64 and d.continuation_hits >= 512
    assert any(len(d.lights[k].culled) >= 1 and len(d.lights[k].not_culled) >= 1 for k in d.lights if k >= 1)      # (packet, light) pairs culled at a nested level
    assert frame.any() and stats[2] > 256 * len(xy)
    # the opacity channel spans 0..255
    op = np.unique(TK.opacity_texture()[:, :, 0])
    assert op.min() == 0 and op.max() == 255 and len(op) >= 30


def test_panes_without_capable_materials_is_the_existing_restatement():
    """with opaque stand-ins nothing nests, and the frame and TreeStats are MaterialsRef.render's"""
    c = TK.panes()
    fr = TK.case_ref(c, opaque=True)
    got = fr.render(c["cam"].as_array13(), 70, 50, c["lights"], mode=O.MODE_IEEE, max_depth=1)
    want = fr.tr.ref.render(c["cam"].as_array13(), 70, 50, c["lights"], mode=O.MODE_IEEE)
    assert got[3].deepest == 0 and got[2] == 0 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
