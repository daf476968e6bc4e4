"""The tile renderer of full-shaded plain scenes, the parts that need no GPU: the C-ABI of include/snail_materials_tiles.h as a contract (plain C,
every declared symbol exported and bound, bad arguments refused before anything touches a device), the adapter's opt-in routing against mock
reference types, the test-side restatement (tests/materials_tiles_ref.py) against what already exists where the two must coincide, and the
frames of tests/materials_tiles_cases.py against the conditions the GPU tests rest on."""
import os
import re
import subprocess

import numpy as np
import pytest

from snail_amd import _lib
from tests import dbvh_shade_ref as S
from tests import materials_bounce_cases as BK
from tests import materials_bounce_ref as B
from tests import materials_tiles_cases as C
from tests import materials_tiles_ref as MT
from tests import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "snail_amd")
MODES = [O.MODE_IEEE, O.MODE_SSE]
REFL, DEPTH, AA = C.REFL, C.DEPTH, C.AA


# ---- the C-ABI ----
def test_signatures_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "snail_materials_tiles.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|int64_t|void)\s*(snail_[a-z_0-9]+)\s*\(", hdr, flags=re.M)))
    from snail_amd._lib import (BVH_FAST_SIGNATURES, HEATMAP_SIGNATURES, INSTANCES_BUILD_SIGNATURES, INSTANCES_SHADE_SIGNATURES, INSTANCES_SIGNATURES,
                                INSTANCES_TILES_SIGNATURES, MATERIALS_BOUNCE_SIGNATURES, MATERIALS_SIGNATURES, MATERIALS_TILES_SIGNATURES, SIGNATURES, lib)
    assert sorted(MATERIALS_TILES_SIGNATURES) == declared and len(declared) == 3, declared
    for other in (SIGNATURES, INSTANCES_SIGNATURES, INSTANCES_SHADE_SIGNATURES, INSTANCES_TILES_SIGNATURES, INSTANCES_BUILD_SIGNATURES, BVH_FAST_SIGNATURES,
                  HEATMAP_SIGNATURES, MATERIALS_SIGNATURES, MATERIALS_BOUNCE_SIGNATURES):
        assert not set(MATERIALS_TILES_SIGNATURES) & set(other)
    assert '#include "snail_materials_bounce.h"' in hdr
    L = lib()
    for name in declared:
        assert hasattr(L, name), "libsnailhip.so does not export " + name
        assert getattr(L, name).argtypes == MATERIALS_TILES_SIGNATURES[name][1]
    # it mirrors snail_instances_tiles.h function for function: the same arguments without the default material's colour
    for new, old in (("snail_materials_frame_packets_dev", "snail_instances_shade_packets_dev"), ("snail_materials_render_tiles", "snail_instances_render_tiles"),
                     ("snail_materials_render_frame", "snail_instances_render_frame")):
        assert len(MATERIALS_TILES_SIGNATURES[new][1]) == len(INSTANCES_TILES_SIGNATURES[old][1]) - 1
    # every parameter of the header's declarations, counted
    for name in declared:
        m = re.search(r"^int " + name + r"\s*\(([^;]*)\);", hdr, flags=re.M | re.S)
        assert m and len(m.group(1).split(",")) == len(MATERIALS_TILES_SIGNATURES[name][1]), name
    # the older headers keep their functions; only their "NOT here" comments moved on
    for h, n in (("snail_materials.h", 9), ("snail_materials_bounce.h", 5)):
        text = open(os.path.join(ROOT, "include", h)).read()
        assert len(set(re.findall(r"^(?:int|int64_t|void|SnailMaterials \*)\s*(snail_[a-z_0-9]+)\s*\(", text, flags=re.M))) == n, h
        assert "snail_materials_tiles.h" in text


def test_header_is_a_c_header(tmp_path):
    exe = str(tmp_path / "materials_tiles_c")
    src = os.path.join(ROOT, "tests", "c", "materials_tiles_c.c")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", src, "-o", exe, "-L" + LIBDIR, "-lsnailhip", "-Wl,-rpath," + LIBDIR])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "C materials tiles ABI ok: 3 symbols" in r.stdout, (r.returncode, r.stdout, r.stderr)
    from snail_amd._lib import MATERIALS_TILES_SIGNATURES
    assert set(re.findall(r"ADDR\((snail_[a-z0-9_]+)\)", open(src).read())) == set(MATERIALS_TILES_SIGNATURES)


def test_python_binding_has_the_three_calls():
    from snail_amd import materials as P
    for name in ("frame_packets", "render_tiles_host", "render_frame_host"):
        assert callable(getattr(P.MaterialSet, name))
    assert (P.RENDER_REFLECTIONS, P.RENDER_DEPTH, P.RENDER_AA4) == (REFL, DEPTH, AA)


class Call:
    """the three entry points with a null handle and plausible arguments; whatever is refused must be refused before the handle, with its own text"""

    def __init__(self):
        self.cam = np.zeros(13, np.float32); self.cam[3] = self.cam[7] = self.cam[11] = self.cam[12] = 1.0
        self.amb = np.full(3, 0.1, np.float32)
        self.lights = np.ones((9, 7), np.float32)
        self.coords = np.array([0, 0, 4, 4, 4, 0, 4, 4], np.int32)
        self.off = np.array([0, 48], np.int64)
        self.xy = np.zeros(2, np.int32)
        self.out = np.full(1024, 7, np.uint8)

    def tiles(self, flags=0, tint=None, coords=None, n_lights=0, data=True, offsets=True, amb=True, cam=True, res=(8, 4)):
        t = None if tint is None else np.asarray(tint, np.float32)
        co = self.coords if coords is None else np.asarray(coords, np.int32)
        rc = _lib.lib().snail_materials_render_tiles(None, _lib.ptr(self.cam) if cam else None, res[0], res[1], _lib.ptr(co), _lib.ptr(self.off) if offsets else None, len(co) // 4,
                                                     _lib.ptr(self.lights) if n_lights else None, n_lights, _lib.ptr(self.amb) if amb else None, flags, _lib.ptr(t),
                                                     _lib.ptr(self.out) if data else None, None)
        return rc, _lib.lib().snail_last_error().decode()

    def packets(self, flags=0, tint=None, n_lights=0, out=True, xy=True, n=1):
        t = None if tint is None else np.asarray(tint, np.float32)
        rc = _lib.lib().snail_materials_frame_packets_dev(None, _lib.ptr(self.cam), 16, 16, _lib.ptr(self.xy) if xy else None, n, _lib.ptr(self.lights) if n_lights else None,
                                                          n_lights, _lib.ptr(self.amb), flags, _lib.ptr(t), _lib.ptr(self.out) if out else None, None, None)
        return rc, _lib.lib().snail_last_error().decode()

    def frame(self, flags=0, n_lights=0, image=True, pitch=24, res=(8, 4)):
        rc = _lib.lib().snail_materials_render_frame(None, _lib.ptr(self.cam), res[0], res[1], _lib.ptr(self.lights) if n_lights else None, n_lights, _lib.ptr(self.amb), flags,
                                                     _lib.ptr(self.out) if image else None, pitch, None)
        return rc, _lib.lib().snail_last_error().decode()


def test_refusals_before_any_device_is_touched():
    c = Call()
    for fn in (c.tiles, c.packets, c.frame):
        for flags in (8, 16, 0x100, -1, 8 | AA):                               # unknown bits: the text names `flags`
            rc, msg = fn(flags=flags)
            assert rc != 0 and "flags" in msg, (fn.__name__, flags, msg)
        for flags in range(8):                                                   # every combination of the three is accepted: the null handle stops the call
            rc, msg = fn(flags=flags)
            assert rc != 0 and "flags" not in msg and "handle" in msg, (fn.__name__, flags, msg)
        rc, msg = fn(flags=AA, n_lights=9)                                       # nLights > SNAIL_MAX_LIGHTS
        assert rc != 0 and "lights" in msg and "handle" not in msg, msg
    for fn in (c.tiles, c.packets):
        for tint in ([0.6, np.nan, 1.0], [np.inf, 1.0, 1.0], [1.0, 1.0, -np.inf]):
            rc, msg = fn(flags=AA, tint=tint)
            assert rc != 0 and "tint" in msg and "handle" not in msg, msg
        rc, msg = fn(flags=AA, tint=[0.7, 1.7, 0.7])                             # a finite tint is accepted
        assert rc != 0 and "handle" in msg
    for bad in ([0, 0, 4, 4, 4, 0, 0, 4], [0, 0, 4, 4, 4, 0, 4, -1], [0, 0, 4, 4, -1, 0, 4, 4], [0, 0, 4, 4, 4, -2, 4, 4]):      # empty, negative size, negative origin
        rc, msg = c.tiles(coords=bad)
        assert rc != 0 and "rect" in msg and "tile 1" in msg and "handle" not in msg, msg
    for kw in (dict(data=False), dict(offsets=False)):                           # null outputs
        rc, msg = c.tiles(**kw)
        assert rc != 0 and "null buffer" in msg, msg
    rc, msg = c.packets(out=False)
    assert rc != 0 and "output" in msg and "handle" not in msg, msg
    rc, msg = c.packets(xy=False)
    assert rc != 0 and "packet list" in msg, msg
    rc, msg = c.frame(image=False)
    assert rc != 0 and "image" in msg and "handle" not in msg, msg
    rc, msg = c.frame(pitch=23)
    assert rc != 0 and "pitch" in msg and "handle" not in msg, msg
    rc, msg = c.tiles(res=(0, 4))
    assert rc != 0 and "resolution" in msg, msg
    assert (c.out == 7).all()                                                    # nothing was written by any of them


# ---- the adapter ----
def build_materials_mock(tmp_path, opted_in=True):
    exe = str(tmp_path / ("materials_mock" + ("_device" if opted_in else "_host")))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread"] + (["-DSNAIL_ADAPTER_DEVICE_MATERIALS"] if opted_in else []) +
                          [os.path.join(ROOT, "tests", "cpp", "materials_mock.cpp"), "-o", exe, "-L" + LIBDIR, "-lsnailhip", "-Wl,-rpath," + LIBDIR])
    return exe


@pytest.mark.parametrize("opted_in", [True, False], ids=["with_the_macro", "without_the_macro"])
def test_adapter_compiles_and_links_against_mock_reference_types(tmp_path, opted_in):
    """... and, before it would touch a device, checks UnsupportedSwitch's old forms and the new one's routing table"""
    r = subprocess.run([build_materials_mock(tmp_path, opted_in)], capture_output=True, text=True)
    assert r.returncode == 0 and ("compiled and linked %s SNAIL_ADAPTER_DEVICE_MATERIALS" % ("with" if opted_in else "without")) in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_the_other_mocks_still_compile(tmp_path):
    """hosts and mocks built without the macro compile unchanged (their routing is their own tests')"""
    for name in ("adapter_mock", "heatmap_mock", "instances_tiles_mock"):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-fsyntax-only", os.path.join(ROOT, "tests", "cpp", name + ".cpp")])


# ---- the restatement against what already exists ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,refl", [("small", False), ("large", False), ("mirror", True), ("small", True)])
def test_plain_flags_are_the_existing_restatements(name, refl, mode):
    """flags 0 / SNAIL_RENDER_REFLECTIONS without tint: the bytes and TreeStats of MaterialsRef.render_packets / BounceRef.render_packets"""
    res = C.PACKET_RES
    cam = C.camera(name, res).as_array13()
    xy = C.frame_xy(res)[::-1].copy()
    lights = BK.case(name)["lights"]
    got, gst = C.tref(name).packets(cam, res[0], res[1], xy, lights, REFL if refl else 0, mode=mode)
    if refl:
        want, wst, _ = B.BounceRef(BK.materials_ref(name)).render_packets(cam, res[0], res[1], xy, lights, mode=mode)
    else:
        want, wst, _ = BK.materials_ref(name).render_packets(cam, res[0], res[1], xy, lights, mode=mode)
    assert want.any() and np.array_equal(got, want) and np.array_equal(gst, wst), (gst, wst)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("flags", [0, AA, DEPTH, AA | DEPTH], ids=["plain", "aa", "depth", "aa_depth"])
def test_degenerate_box_equals_the_oracle_s_simple_shading(flags, mode):
    """default material, flat plane normals: full shading is simple shading, so the restatement's frame and TreeStats are the CPU oracle's
    with the same switches -- the check of it that does not rest on itself"""
    resx, resy = C.RES
    c = BK.case("degenerate_box")
    cam = c["cam"].as_array13()
    got, gst = C.tref("degenerate_box").frame(cam, resx, resy, c["lights"], flags, mode=mode)
    want, wst = c["osc"].render_whitted(cam, resx, resy, c["lights"], mode=mode, antialias=bool(flags & AA), depth=bool(flags & DEPTH))
    other, _ = c["osc"].render_whitted(cam, resx, resy, c["lights"], mode=mode, antialias=not flags & AA, depth=bool(flags & DEPTH))
    bad = np.argwhere((got != want).any(axis=2))
    assert want.any() and (want != other).any()                                # (the antialiased frame is another frame)
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())
    assert np.array_equal(gst, wst), (gst, wst)
    # ... and its tile list is the planar encoding of that frame, zero beyond the image
    planes, tst = C.tref("degenerate_box").tiles(cam, resx, resy, C.TILES, c["lights"], flags, mode=mode)
    padded = np.zeros((128, 48, 3), dtype=np.uint8)
    padded[:resy, :resx] = want
    for k, (a, b) in enumerate(zip(planes, O.planar_encode(padded, C.TILES))):
        t = C.TILES[k]
        b = b.reshape(3, t[3], t[2]).copy()
        b[:, max(0, resy - t[1]):, :] = 0; b[:, :, max(0, resx - t[0]):] = 0     # (G-R and B-R of a zero pixel are zero; R is zero)
        assert np.array_equal(a, b.reshape(-1)), (k, t.tolist())


def test_tint_applies_after_the_reduction_and_under_depth():
    res = C.PACKET_RES
    cam = C.camera("large", res).as_array13()
    xy = C.frame_xy(res)
    lights = BK.case("large")["lights"]
    clamped = 0
    for flags in (AA, AA | DEPTH, REFL):
        col, _ = C.tref("large").colors(cam, res[0], res[1], xy, lights, flags)
        plain, _ = C.tref("large").packets(cam, res[0], res[1], xy, lights, flags)
        tinted, _ = C.tref("large").packets(cam, res[0], res[1], xy, lights, flags, tint=MT.rank_tint(15))
        assert np.array_equal(tinted, S.conv_color(MT.apply_tint(col, MT.rank_tint(15))).reshape(-1, 256, 3)) and not np.array_equal(plain, tinted)
        clamped += int((plain[..., 1][tinted[..., 1] == 255] < 255).sum())
    assert clamped > 0                                                           # 1.7 drove a green channel into the clamp


# ---- non-vacuity: the frames the GPU tests use, on the restatement's diagnostics ----
@pytest.mark.parametrize("mode", MODES)
def test_large_tile_list_under_aa(mode):
    d = C.diag_of("large", C.RES, MT.tile_packets(C.TILES), AA, mode)
    assert d.blocks_a > 0 and d.blocks_c > 0, (d.blocks_a, d.blocks_c)                       # single-triangle blocks, several-material blocks
    assert sum(v for (_, lvl), v in d.mips.items() if lvl > 0) > 0                           # TEX lanes on a mip above 0
    assert d.lit_pixels > 0 and d.occluded_pixels > 0


@pytest.mark.parametrize("mode", MODES)
def test_small_tile_list_under_aa(mode):
    d = C.diag_of("small", C.RES, MT.tile_packets(C.TILES), AA, mode)
    assert d.blocks_a > 0 and d.blocks_b > 0 and d.blocks_c > 0, (d.blocks_a, d.blocks_b, d.blocks_c)
    assert d.uber_masked > 0 and d.uber_unmasked > 0
    assert d.hit_pixels < 4 * 256 * len(MT.tile_packets(C.TILES))                            # misses
    assert len(d.culled) > 0 and len(d.not_culled) > 0                                       # at least one (packet, light) culled


@pytest.mark.parametrize("mode", MODES)
def test_quirk_tile_list_under_aa(mode):
    d = C.diag_of("quirk", C.RES, MT.tile_packets(C.TILES), AA, mode)
    assert d.blocks_masked_one > 0


@pytest.mark.parametrize("mode", MODES)
def test_mirror_frame_under_aa_with_the_bounce(mode):
    d = C.diag_of("mirror", C.PACKET_RES, C.frame_xy(C.PACKET_RES), AA | REFL, mode)
    assert d.packets_masked > 0 and d.packets_unmasked > 0
    assert d.a_masked > 0 and d.a_unmasked > 0                                               # branch (a) in both
    assert d.mirrored_misses > 0 and d.mirrored_hits > 0
