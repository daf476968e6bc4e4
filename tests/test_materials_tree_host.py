"""The transparency continuation together with the bounce, tiles, 4x AA and the tint (include/snail_materials_tree.h), the parts that need no
GPU: the header as plain C with every declared symbol exported and bound, the argument refusals that come before any device call, the level
budget's arithmetic, the Python binding, the adapter's opt-in routing against a mock C-ABI (tests/cpp/materials_tree_mock.cpp), the restatement
(tests/materials_tree_ref.py) against the three it is composed of, and the conditions `room` (tests/materials_tree_cases.py) must meet for the
GPU comparisons to mean something -- on the restatement's diagnostics alone."""
import os
import re
import subprocess

import numpy as np
import pytest

from snail_amd import _lib
from snail_amd import materials as P
from tests import materials_bounce_ref as B
from tests import materials_tiles_ref as MT
from tests import materials_transparency_cases as TK
from tests import materials_tree_cases as K
from tests import materials_tree_ref as TR
from tests import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "snail_amd")
MODES = [O.MODE_IEEE, O.MODE_SSE]
REFL, DEPTH, AA = P.RENDER_REFLECTIONS, P.RENDER_DEPTH, P.RENDER_AA4


def test_signatures_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "snail_materials_tree.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|int64_t|void)\s*(snail_[a-z_0-9]+)\s*\(", hdr, flags=re.M)))
    S = _lib.MATERIALS_TREE_SIGNATURES
    assert sorted(S) == declared and len(declared) == 6, declared
    for other in (_lib.SIGNATURES, _lib.MATERIALS_SIGNATURES, _lib.MATERIALS_BOUNCE_SIGNATURES, _lib.MATERIALS_TILES_SIGNATURES, _lib.MATERIALS_TRANSPARENCY_SIGNATURES):
        assert not set(S) & set(other)
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), "libsnailhip.so does not export " + name
        assert getattr(L, name).argtypes == S[name][1]
    # the frames: the arguments of their snail_materials_tiles.h namesakes with maxDepth and the truncated-lane counter before the stats
    Tl = _lib.MATERIALS_TILES_SIGNATURES
    for new, old, at in (("snail_materials_tree_frame_packets_dev", "snail_materials_frame_packets_dev", -2), ("snail_materials_tree_render_tiles", "snail_materials_render_tiles", -1),
                         ("snail_materials_tree_render_frame", "snail_materials_render_frame", -1)):
        res, args = Tl[old]
        assert S[new] == (res, args[:at] + [_lib._I, _lib._VP] + args[at:])
    # the older headers neither name the new functions nor changed their lists
    assert len(Tl) == 3 and len(_lib.MATERIALS_TRANSPARENCY_SIGNATURES) == 8 and len(_lib.MATERIALS_BOUNCE_SIGNATURES) == 5 and len(_lib.MATERIALS_SIGNATURES) == 9


def test_header_is_a_c_header(tmp_path):
    exe = str(tmp_path / "materials_tree_c")
    src = os.path.join(ROOT, "tests", "c", "materials_tree_c.c")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", src, "-o", exe, "-L" + LIBDIR, "-lsnailhip", "-Wl,-rpath," + LIBDIR])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "C materials tree ABI ok: 6 symbols" in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert set(re.findall(r"ADDR\((snail_[a-z0-9_]+)\)", open(src).read())) == set(_lib.MATERIALS_TREE_SIGNATURES)


def test_refusals_come_before_the_handle():
    """flags first, then maxDepth, the null counter, the tint, the rects -- all with a null handle, which is what stops an accepted call"""
    L = _lib.lib()
    cam, amb, img, tr = np.zeros(13, np.float32), np.full(3, 0.1, np.float32), np.full(48, 7, np.uint8), np.zeros(1, np.uint64)
    rect, off = np.array([0, 0, 4, 4], np.int32), np.zeros(1, np.int64)
    err = lambda: L.snail_last_error().decode()

    def frame(flags, depth=8, trunc=tr):
        return L.snail_materials_tree_render_frame(None, _lib.ptr(cam), 4, 4, None, 0, _lib.ptr(amb), flags, _lib.ptr(img), 12, depth, _lib.ptr(trunc), None)

    def tiles(flags, depth=8, trunc=tr, tint=None, r=rect):
        return L.snail_materials_tree_render_tiles(None, _lib.ptr(cam), 4, 4, _lib.ptr(r), _lib.ptr(off), 1, None, 0, _lib.ptr(amb), flags, _lib.ptr(tint), _lib.ptr(img), depth,
                                                   _lib.ptr(trunc), None)

    def packets(flags, depth=8, trunc=tr, tint=None):
        return L.snail_materials_tree_frame_packets_dev(None, _lib.ptr(cam), 4, 4, None, 1, None, 0, _lib.ptr(amb), flags, _lib.ptr(tint), _lib.ptr(img), depth, _lib.ptr(trunc),
                                                        None, None)

    for call in (frame, tiles, packets):
        for flags in (8, 0x100, -1, 16 | REFL):
            assert call(flags, 0, None) != 0 and "flags" in err(), err()       # (a bad depth and a null counter as well: the flags are named)
        for flags in range(8):                                                     # every combination of the three is accepted
            assert call(flags, 0) != 0 and "maxDepth" in err(), (flags, err())
        for depth in (-1, 0, 9):
            assert call(REFL | AA, depth, None) != 0 and "maxDepth" in err()
        assert call(REFL, 8, None) != 0 and "truncated" in err()
    bad_tint = np.array([1.0, np.inf, 1.0], np.float32)
    assert tiles(AA, tint=bad_tint) != 0 and "tint" in err()
    assert packets(AA, tint=bad_tint) != 0 and "tint" in err()
    for r in ([0, 0, 0, 4], [-1, 0, 4, 4], [0, 0, 4, -2]):
        assert tiles(REFL, r=np.array(r, np.int32)) != 0 and "bad rect" in err(), err()
    assert packets(REFL) != 0 and "packet list" in err()
    for call in (frame, tiles):
        assert call(REFL | AA | DEPTH) != 0 and "handle" in err(), err()
    assert L.snail_materials_mirror_rays_dev(None, 1, *([None] * 15)) != 0 and "snail_materials_mirror_rays_dev" in err()
    assert L.snail_materials_set_level_budget(None, 1 << 20) != 0 and "handle" in err()
    assert (img == 7).all() and tr[0] == 0


def test_level_bytes_and_the_budget_arithmetic():
    lb = P.MaterialSet.level_bytes

    def level(n, nl):                                              # one level of n packets (materials_transparency_host.inc: TranspLevel::bytes)
        pad = lambda b: (b + 255) & ~255
        return pad(n * 1024 * (25 + nl) + pad(n * 64)) + extra(n)

    def extra(n):                                                  # opacity, selector, order
        pad = lambda b: (b + 255) & ~255
        return n * 1024 + pad(n * 64) + pad(n * 4)

    for nl in (0, 2, 8):
        for d in (1, 2, 8):
            assert lb(nl, 0, d) == extra(1) + d * level(1, nl)                                  # D A-levels + level 0's three planes
            assert lb(nl, REFL, d) == extra(1) + (2 * d + 1) * level(1, nl)                     # + D + 1 B-levels
            assert lb(nl, AA, d) == extra(4) + d * level(4, nl)                                 # four double-resolution packets
            assert lb(nl, REFL | AA, d) == extra(4) + (2 * d + 1) * level(4, nl)
            assert lb(nl, DEPTH | REFL | AA, d) == 0                                            # depth shading runs no level
            # a slice of s output packets fits whenever s * level_bytes does: rounding is per buffer, so n packets take at most n times one's
            for s in (2, 5, 450):
                q = 4
                assert extra(s * q) + (2 * d + 1) * level(s * q, nl) <= s * lb(nl, REFL | AA, d)
    # the header's arithmetic of the default
    assert lb(8, REFL | AA, 8) == 17 * 140032 + 4608 == 2385152 and 140032 == 136.75 * 1024 and (1 << 30) // 2385152 == 450 and -(-8160 // 450) == 19
    for bad in ((9, 0, 8), (-1, 0, 8), (0, 8, 8), (0, 0, 0), (0, 0, 9)):
        with pytest.raises(_lib.SnailError):
            lb(*bad)


def test_python_binding():
    for name in ("mirror_rays", "tree_frame_packets", "render_tree_tiles_host", "render_tree_frame_host", "set_level_budget", "level_bytes"):
        assert hasattr(P.MaterialSet, name)


# ---- the adapter, against a mock C-ABI ----
def build_mock(tmp_path, name, *defines):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread"] + ["-D" + d for d in defines] +
                          [os.path.join(ROOT, "tests", "cpp", "materials_tree_mock.cpp"), "-o", exe])
    return exe


def test_adapter_routing_against_the_mock_abi(tmp_path):
    both = build_mock(tmp_path, "both", "SNAIL_ADAPTER_DEVICE_MATERIALS", "SNAIL_ADAPTER_DEVICE_TRANSPARENCY")
    r = subprocess.run([both, "routing"], capture_output=True, text=True)
    assert r.returncode == 0 and "ok (with SNAIL_ADAPTER_DEVICE_TRANSPARENCY)" in r.stdout and "_tree_ 3 + 2 times" in r.stdout, (r.returncode, r.stdout, r.stderr)
    r = subprocess.run([both, "truncated"], capture_output=True, text=True)
    assert r.returncode == 0 and "rendered again by the host renderer" in r.stdout, (r.returncode, r.stdout, r.stderr)
    # without the new macro: today's routing -- a set that can select is the host renderer's, _tree_ is never reached
    old = build_mock(tmp_path, "old", "SNAIL_ADAPTER_DEVICE_MATERIALS")
    r = subprocess.run([old, "routing"], capture_output=True, text=True)
    assert r.returncode == 0 and "ok (without SNAIL_ADAPTER_DEVICE_TRANSPARENCY)" in r.stdout and "_tree_ 0 + 0 times" in r.stdout, (r.returncode, r.stdout, r.stderr)
    # the new macro alone is without effect
    alone = build_mock(tmp_path, "alone", "SNAIL_ADAPTER_DEVICE_TRANSPARENCY")
    r = subprocess.run([alone, "truncated"], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)


def test_adapter_aborts_without_a_host_renderer(tmp_path):
    """SNAIL_ADAPTER_NO_HOST_RENDERER: a frame whose counter moved aborts with a message naming the depth (a child process, on the CPU)"""
    exe = build_mock(tmp_path, "nohost", "SNAIL_ADAPTER_DEVICE_MATERIALS", "SNAIL_ADAPTER_DEVICE_TRANSPARENCY", "SNAIL_ADAPTER_NO_HOST_RENDERER")
    r = subprocess.run([exe, "truncated"], capture_output=True, text=True)
    assert r.returncode == -6 and "maxDepth 8" in r.stderr and "SNAIL_ADAPTER_NO_HOST_RENDERER" in r.stderr, (r.returncode, r.stdout, r.stderr)


def test_the_other_mocks_still_compile():
    for name in ("adapter_mock", "heatmap_mock", "instances_tiles_mock", "materials_mock"):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-fsyntax-only", os.path.join(ROOT, "tests", "cpp", name + ".cpp")])


# ---- the restatement against those it is composed of ----
@pytest.mark.parametrize("mode", MODES)
def test_without_the_bounce_the_restatement_is_transp_frames(mode):
    c = K.room()
    xy = K.frame_packets(38, 26)
    for depth in (2, 8):
        got = TR.TreeFrames(K.room_tr(), bounce=False).render_packets(c["cam"].as_array13(), 38, 26, xy, c["lights"], mode=mode, max_depth=depth)
        want = TK.case_ref(c).render_packets(c["cam"].as_array13(), 38, 26, xy, c["lights"], mode=mode, max_depth=depth)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2] and got[0].any()
        a, b = got[3], want[3]
        assert (a.deepest, a.nested_full, a.nested_masked, a.nested_none, a.continuation_hits, a.truncated) == (
            b.deepest, b.nested_full, b.nested_masked, b.nested_none, b.continuation_hits, b.truncated)
        assert not a.b_calls and a.truncated_b == 0
    ref = K.tiles_ref(8)
    col, st = ref.packets(c["cam"].as_array13(), 38, 26, xy, c["lights"], 0, None, mode=mode)
    assert np.array_equal(col, want[0]) and np.array_equal(st, want[1]) and ref.truncated == 0


def test_with_an_opaque_set_the_restatement_is_the_bounce_s_and_the_tiles():
    c = K.room()
    xy = K.frame_packets(38, 26)
    cam13 = c["cam"].as_array13()
    tr = K.room_tr(opaque=True)
    old = MT.MaterialTilesRef(tr.ref)
    want = B.BounceRef(tr.ref).render_packets(cam13, 38, 26, xy, c["lights"])
    for depth in (1, 8):
        got = TR.TreeFrames(tr).render_packets(cam13, 38, 26, xy, c["lights"], max_depth=depth)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == 0 and got[0].any()
        d = got[3]
        assert d.deepest == 0 and set(d.b_calls) == {(0, 0)}
        ref = K.tiles_ref(depth, opaque=True)
        for flags, tint in ((REFL | AA, K.TINT), (AA, None), (DEPTH, None)):
            a, b = ref.packets(cam13, 38, 26, xy, c["lights"], flags, tint), old.packets(cam13, 38, 26, xy, c["lights"], flags, tint)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and ref.truncated == 0 and a[0].any()


# ---- the conditions ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("resx,resy", K.FRAMES + [(96, 64), (76, 52)])
def test_room_meets_the_conditions(resx, resy, mode):
    """conditions on the INPUTS, on the restatement's diagnostics alone, for both frames and their double-resolution frames under 4x AA"""
    n = len(K.frame_packets(resx, resy))
    _, _, trunc, d = K.diag_frame(resx, resy, mode, 8)
    _, _, t2, d2 = K.diag_frame(resx, resy, mode, 2)
    _, _, t1, d1 = K.diag_frame(resx, resy, mode, 1)
    print("D = 8:", K.describe(d)); print("D = 2:", K.describe(d2)); print("D = 1:", K.describe(d1))
    assert trunc == 0
    K.check_conditions_depth8(d, n)
    for lights in ("none", "eight"):
        assert K.diag_frame(resx, resy, mode, 8, lights)[2] == 0
    assert d2.truncated_a > 0 and d2.truncated_b > 0 and t2 == d2.truncated_a + d2.truncated_b, (d2.truncated_a, d2.truncated_b)
    assert d1.truncated_at.get((1, 1), 0) > 0 and d1.truncated_a > 0, d1.truncated_at       # B_{1,1} is cut at once
    # (D + 1) + (D + 1)(D + 2) / 2 bodies: no call outside the triangle, and every call of chain A mirrors, hit or not
    for dd, depth in ((d, 8), (d2, 2), (d1, 1)):
        assert all(0 <= k <= depth for k in dd.a_calls) and all(0 <= k <= j <= depth for (k, j) in dd.b_calls)
        assert all(dd.b_calls.get((k, k), 0) == dd.a_calls[k] for k in dd.a_calls)
