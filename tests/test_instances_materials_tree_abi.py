"""Host-only checks (no GPU) of the C-ABI of include/snail_instances_materials_tree.h: the header as a C contract (plain C, every declared symbol
exported and bound, the older headers' symbol lists as they were) and what is refused before anything touches a device."""
import os
import re
import subprocess

import numpy as np
import pytest

from snail_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "snail_amd")
T = _lib.INSTANCES_MATERIALS_TREE_SIGNATURES
DECL = r"^(?:int|int64_t|void|SnailInstancesMaterials \*)\s*(snail_[a-z_0-9]+)\s*\("
ALL = 1 | 2 | 4


def test_signatures_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "snail_instances_materials_tree.h")).read()
    declared = sorted(set(re.findall(DECL, hdr, flags=re.M)))
    assert sorted(T) == declared and len(declared) == 6, declared
    for name in dir(_lib):
        other = getattr(_lib, name)
        if name.endswith("SIGNATURES") and other is not T:
            assert not set(T) & set(other), name
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), "libsnailhip.so does not export " + name
        assert getattr(L, name).argtypes == T[name][1] and getattr(L, name).restype == T[name][0]
    # the arguments of the plain scenes' twins; the mirror stage has d_element and d_bary besides, before d_order
    P, VP = _lib.MATERIALS_TREE_SIGNATURES, _lib._VP
    for name in T:
        twin = P[name.replace("snail_instances_materials_", "snail_materials_")]
        if name == "snail_instances_materials_mirror_rays_dev":
            assert T[name] == (twin[0], twin[1][:14] + [VP, VP] + twin[1][14:])
        else:
            assert T[name] == twin


def test_the_older_headers_keep_their_symbol_lists():
    hdr = open(os.path.join(ROOT, "include", "snail_instances_materials_tree.h")).read()
    for older, table in (("snail_instances_materials.h", _lib.INSTANCES_MATERIALS_SIGNATURES), ("snail_instances_materials_bounce.h", _lib.INSTANCES_MATERIALS_BOUNCE_SIGNATURES),
                         ("snail_instances_materials_transparency.h", _lib.INSTANCES_MATERIALS_TRANSPARENCY_SIGNATURES), ("snail_materials_tree.h", _lib.MATERIALS_TREE_SIGNATURES)):
        text = open(os.path.join(ROOT, "include", older)).read()
        assert sorted(set(re.findall(DECL, text, flags=re.M))) == sorted(table), older
        assert "snail_instances_materials_tree.h" not in text.split("#ifndef", 1)[1], older      # named in the comment alone: no code of the older header changes
    for inc in ("snail_instances_materials_transparency.h", "snail_instances_materials_bounce.h"):
        assert '#include "%s"' % inc in hdr


def test_header_is_a_c_header(tmp_path):
    exe = str(tmp_path / "instances_materials_tree_c")
    src = os.path.join(ROOT, "tests", "c", "instances_materials_tree_c.c")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", src, "-o", exe, "-L" + LIBDIR, "-lsnailhip", "-Wl,-rpath," + LIBDIR])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "C instances materials tree ABI ok: 6 symbols" in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert set(re.findall(r"ADDR\((snail_[a-z0-9_]+)\)", open(src).read())) == set(T)


# ---- refusals that need no device ----
def _args():
    cam = np.zeros(13, dtype=np.float32)
    amb = np.full(3, 0.1, dtype=np.float32)
    return cam, amb, np.zeros((1, 2), dtype=np.int32), np.full((256, 3), 7, dtype=np.uint8), np.full(1, 5, dtype=np.uint64)


def _refused(rc, *words):
    msg = _lib.lib().snail_last_error().decode()
    assert rc != 0 and all(w in msg for w in words), (rc, msg)
    return msg


@pytest.mark.parametrize("flags", [8, 16, ALL | 32, -1])
def test_unknown_flag_bits_are_refused_with_a_text_that_names_flags(flags):
    L, p = _lib.lib(), _lib.ptr
    cam, amb, xy, out, trunc = _args()
    tile, off = np.array([0, 0, 16, 16], dtype=np.int32), np.zeros(1, dtype=np.int64)
    # before everything else: the other arguments are all bad as well
    _refused(L.snail_instances_materials_tree_frame_packets_dev(None, None, 0, 0, None, 1, None, 0, None, flags, None, None, 0, None, None, None), "flags")
    _refused(L.snail_instances_materials_tree_render_tiles(None, None, 0, 0, None, None, 1, None, 0, None, flags, None, None, 0, None, None), "flags")
    _refused(L.snail_instances_materials_tree_render_frame(None, None, 0, 0, None, 0, None, flags, None, 0, 0, None, None), "flags")
    assert L.snail_instances_materials_level_bytes(0, flags, 1) == -1 and "flags" in L.snail_last_error().decode()
    assert (out == 7).all() and trunc[0] == 5 and p(tile) and p(off) and p(cam) and p(amb) and p(xy)


@pytest.mark.parametrize("flags", range(8))
def test_every_known_combination_reaches_the_handle(flags):
    L, p = _lib.lib(), _lib.ptr
    cam, amb, xy, out, trunc = _args()
    msg = _refused(L.snail_instances_materials_tree_frame_packets_dev(None, p(cam), 16, 16, p(xy), 1, None, 0, p(amb), flags, None, p(out), 8, p(trunc), None, None), "handle")
    assert "flags" not in msg and (out == 7).all() and trunc[0] == 5


@pytest.mark.parametrize("depth", [0, 9, -1])
def test_max_depth_outside_1_to_8_is_refused(depth):
    L, p = _lib.lib(), _lib.ptr
    cam, amb, xy, out, trunc = _args()
    tile, off = np.array([0, 0, 16, 16], dtype=np.int32), np.zeros(1, dtype=np.int64)
    _refused(L.snail_instances_materials_tree_frame_packets_dev(None, p(cam), 16, 16, p(xy), 1, None, 0, p(amb), 1, None, p(out), depth, p(trunc), None, None), "maxDepth")
    _refused(L.snail_instances_materials_tree_render_tiles(None, p(cam), 16, 16, p(tile), p(off), 1, None, 0, p(amb), 1, None, p(out), depth, p(trunc), None), "maxDepth")
    _refused(L.snail_instances_materials_tree_render_frame(None, p(cam), 4, 4, None, 0, p(amb), 1, p(out), 12, depth, p(trunc), None), "maxDepth")
    assert L.snail_instances_materials_level_bytes(0, 0, depth) == -1
    assert (out == 7).all() and trunc[0] == 5


def test_null_counter_tint_rect_and_handle():
    L, p = _lib.lib(), _lib.ptr
    cam, amb, xy, out, trunc = _args()
    tile, off = np.array([0, 0, 16, 16], dtype=np.int32), np.zeros(1, dtype=np.int64)
    _refused(L.snail_instances_materials_tree_frame_packets_dev(None, p(cam), 16, 16, p(xy), 1, None, 0, p(amb), 0, None, p(out), 8, None, None, None), "truncated")
    _refused(L.snail_instances_materials_tree_render_tiles(None, p(cam), 16, 16, p(tile), p(off), 1, None, 0, p(amb), 0, None, p(out), 8, None, None), "truncated")
    _refused(L.snail_instances_materials_tree_render_frame(None, p(cam), 4, 4, None, 0, p(amb), 0, p(out), 12, 8, None, None), "truncated")
    for bad in ((np.nan, 1.0, 1.0), (1.0, np.inf, 1.0), (1.0, 1.0, -np.inf)):
        tint = np.array(bad, dtype=np.float32)
        _refused(L.snail_instances_materials_tree_frame_packets_dev(None, p(cam), 16, 16, p(xy), 1, None, 0, p(amb), 0, p(tint), p(out), 8, p(trunc), None, None), "tint")
        _refused(L.snail_instances_materials_tree_render_tiles(None, p(cam), 16, 16, p(tile), p(off), 1, None, 0, p(amb), 0, p(tint), p(out), 8, p(trunc), None), "tint")
    for rect in ((0, 0, 0, 16), (0, 0, 16, -1), (-1, 0, 16, 16), (0, 1 << 24, 16, 16)):
        r = np.array(rect, dtype=np.int32)
        _refused(L.snail_instances_materials_tree_render_tiles(None, p(cam), 16, 16, p(r), p(off), 1, None, 0, p(amb), 0, None, p(out), 8, p(trunc), None), "bad rect")
    # good arguments: the null handle is what is left to refuse
    good = np.array([0.6, 1.0, 0.6], dtype=np.float32)
    _refused(L.snail_instances_materials_tree_frame_packets_dev(None, p(cam), 16, 16, p(xy), 1, None, 0, p(amb), ALL, p(good), p(out), 8, p(trunc), None, None), "handle")
    _refused(L.snail_instances_materials_tree_render_tiles(None, p(cam), 16, 16, p(tile), p(off), 1, None, 0, p(amb), ALL, p(good), p(out), 8, p(trunc), None), "handle")
    _refused(L.snail_instances_materials_tree_render_frame(None, p(cam), 4, 4, None, 0, p(amb), ALL, p(out), 12, 8, p(trunc), None), "handle")
    _refused(L.snail_instances_materials_set_level_budget(None, 1 << 20), "handle")
    _refused(L.snail_instances_materials_set_level_budget(None, 0), "0 bytes")
    # no packets / no tiles: no work once the arguments and the handle are good -- with a null handle the handle is refused first
    _refused(L.snail_instances_materials_tree_frame_packets_dev(None, p(cam), 16, 16, None, 0, None, 0, p(amb), 0, None, None, 8, p(trunc), None, None), "handle")
    assert L.snail_instances_materials_mirror_rays_dev(*([None, 0] + [None] * 17)) == 0
    _refused(L.snail_instances_materials_mirror_rays_dev(*([None, 1] + [None] * 17)), "null buffer")
    assert (out == 7).all() and trunc[0] == 5


def test_level_bytes_is_the_header_s_figure():
    L = _lib.lib()
    level = lambda n, lights: ((n * 1024 * (26 + lights) + ((n * 64 + 255) & ~255) + 255) & ~255) + n * 1024 + ((n * 64 + 255) & ~255) + ((n * 4 + 255) & ~255)
    extra = lambda n: n * 1024 + ((n * 64 + 255) & ~255) + ((n * 4 + 255) & ~255)
    assert level(4, 8) == 144128 and extra(4) == 4608      # 140.75 KiB and 4.5 KiB
    for lights in (0, 2, 8):
        for depth in (1, 2, 8):
            for flags in range(8):
                want = 0 if flags & 2 else extra(4 if flags & 4 else 1) + (depth + ((depth + 1) if flags & 1 else 0)) * level(4 if flags & 4 else 1, lights)
                assert L.snail_instances_materials_level_bytes(lights, flags, depth) == want, (lights, depth, flags)
    assert L.snail_instances_materials_level_bytes(8, 1 | 4, 8) == 17 * 144128 + 4608 == int(2397.25 * 1024)
    assert (1 << 30) // (17 * 144128 + 4608) == 437 and -(-8160 // 437) == 19
    assert L.snail_instances_materials_level_bytes(9, 0, 1) == -1 and L.snail_instances_materials_level_bytes(-1, 0, 1) == -1
