"""The tile renderer of instanced scenes, the parts that need no GPU: the test-side restatement tests/dbvh_tiles_ref.py is pinned to the
oracle's RenderTask::Work (one identity instance reproduces the plain scene: 4x antialiasing, depth shading, the planar store), its tint to
values worked out here, and the new C-ABI is a contract: the header is plain C, every new symbol is exported by libsnailhip.so, and the
adapter's opt-in overloads compile."""
import os
import re
import subprocess

import numpy as np
import pytest

from snail_amd.render import divide_image
from tests import dbvh_shade_ref as S
from tests import dbvh_tiles_ref as T
from tests import instances_shade_cases as K
from tests import oracle_lib as O
from tests import util as U
from tests.test_instances_shade_host import identity_ref, scene_lights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "snail_amd")
F = np.float32


@pytest.mark.parametrize("mode", [O.MODE_IEEE, O.MODE_SSE], ids=["ieee", "host_sse"])
@pytest.mark.parametrize("kind", ["lit", "reflections", "depth"])
@pytest.mark.parametrize("name", ["box", "lancia"])
def test_antialiased_restatement_of_an_identity_instance_equals_the_oracle(name, kind, mode):
    """Frame and tile bytes only: the instanced inner walk counts differently, so TreeStats are not compared here."""
    resx, resy = 64, 48
    cam = U.camera_for(name, K.tri_verts(name))
    lights = scene_lights(name, cam)
    flags = T.AA4 | {"lit": 0, "reflections": T.REFLECTIONS, "depth": T.DEPTH}[kind]
    ref = T.TilesRef(identity_ref(name))
    diag = S.Diag()
    ref.colors(cam.as_array13(), resx, resy, S.frame_packets(resx, resy), lights, flags, mode=mode, diag=diag)
    got, _ = ref.frame(cam.as_array13(), resx, resy, lights, flags, mode=mode)
    want, _ = K.oracle(name).render_whitted(cam.as_array13(), resx, resy, lights, mode=mode, reflections=kind == "reflections", antialias=True, depth=kind == "depth")
    plain, _ = K.oracle(name).render_whitted(cam.as_array13(), resx, resy, lights, mode=mode, reflections=kind == "reflections", depth=kind == "depth")
    print(name, kind, mode, "hit samples", diag.hit_pixels, "lit", diag.lit_pixels, "pixels the antialiasing changes", int((want != plain).any(axis=2).sum()))
    assert diag.hit_pixels >= 400 and (kind == "depth" or diag.lit_pixels >= 200)      # (counted over the 4 x 64 x 48 samples)
    assert (want != plain).any(axis=2).sum() >= 20                                      # (the antialiased frame is another frame)
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())
    tiles = divide_image(resx, resy)
    planes, _ = ref.tiles(cam.as_array13(), resx, resy, tiles, lights, flags, mode=mode)
    wplanes = O.planar_encode(want, tiles)
    assert len(planes) == len(wplanes) == len(tiles)
    for k, (a, b) in enumerate(zip(planes, wplanes)):
        assert np.array_equal(a, b), (k, tiles[k].tolist())


def test_tint_is_an_add_and_a_multiply_each_rounded():
    cols = np.array([[0.25, 0.5, 0.75], [-0.3, 0.0, 1.5], [0.9, 0.5, 0.2], [0.33333334, 0.1, 0.7], [1e-3, 0.9999999, 0.45]], dtype=np.float32)
    assert (cols < 0).any() and (cols > 1).any()
    seen_over = False
    for rank in (3, 15, 31, 8):
        tint = T.rank_tint(rank)
        assert np.array_equal(tint, T.NCOLORS[rank % 16])
        got = S.conv_color(T.apply_tint(cols, tint))
        for i in range(len(cols)):
            for ch in range(3):
                a = F(cols[i, ch]) + F(0.1)                # float32 + float32 -> float32: rounded
                m = F(a) * F(tint[ch])                     # rounded again
                v = F(m) * F(255.0)
                v = F(0.0) if not v > 0 else v
                v = F(255.0) if not v < F(255.0) else v
                assert got[i, 2 - ch] == int(v), (rank, i, ch)
                seen_over |= rank % 16 == 15 and ch == 1 and float(a) <= 1.0 and float(m) * 255.0 > 255.0 and got[i, 2 - ch] == 255
    assert seen_over                                        # 1.7 pushed a channel that was inside [0, 1] over 255
    assert T.rank_tint(15)[1] == F(1.7)
    # depth shading is tinted too: the tint applies to whatever colour the packet has
    name = "box"
    cam = U.camera_for(name, K.tri_verts(name))
    ref = T.TilesRef(identity_ref(name))
    xy = S.frame_packets(32, 32)
    plain, _ = ref.packets(cam.as_array13(), 32, 32, xy, None, T.DEPTH)
    tinted, _ = ref.packets(cam.as_array13(), 32, 32, xy, None, T.DEPTH, tint=T.rank_tint(3))
    col, _ = ref.colors(cam.as_array13(), 32, 32, xy, None, T.DEPTH)
    assert not np.array_equal(plain, tinted) and np.array_equal(tinted, S.conv_color(T.apply_tint(col, T.rank_tint(3))).reshape(-1, 256, 3))


def test_tiles_signatures_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "snail_instances_tiles.h")).read()
    declared = sorted(set(re.findall(r"^int (snail_instances_[a-z_0-9]+)\s*\(", hdr, flags=re.M)))
    from snail_amd._lib import INSTANCES_SHADE_SIGNATURES, INSTANCES_SIGNATURES, INSTANCES_TILES_SIGNATURES, SIGNATURES, lib
    assert sorted(INSTANCES_TILES_SIGNATURES) == declared and len(declared) == 3
    assert not set(INSTANCES_TILES_SIGNATURES) & (set(SIGNATURES) | set(INSTANCES_SIGNATURES) | set(INSTANCES_SHADE_SIGNATURES))
    assert '#include "snail_instances_tiles.h"' in open(os.path.join(ROOT, "include", "snail_instances.h")).read()
    L = lib()
    for name in declared:
        assert hasattr(L, name), "libsnailhip.so does not export " + name


def test_tiles_header_is_a_c_header(tmp_path):
    exe = str(tmp_path / "instances_tiles_c")
    src = os.path.join(ROOT, "tests", "c", "instances_tiles_c.c")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", src, "-o", exe, "-L" + LIBDIR, "-lsnailhip", "-Wl,-rpath," + LIBDIR])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "C instances tiles ABI ok: 3 symbols" in r.stdout, (r.returncode, r.stdout, r.stderr)
    from snail_amd._lib import INSTANCES_TILES_SIGNATURES
    assert set(re.findall(r"ADDR\((snail_[a-z0-9_]+)\)", open(src).read())) == set(INSTANCES_TILES_SIGNATURES)


def build_tiles_mock(tmp_path):
    exe = str(tmp_path / "instances_tiles_mock")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", os.path.join(ROOT, "tests", "cpp", "instances_tiles_mock.cpp"), "-o", exe,
                           "-L" + LIBDIR, "-lsnailhip", "-Wl,-rpath," + LIBDIR])
    return exe


def test_adapter_compiles_with_the_instanced_tile_overloads(tmp_path):
    src = open(os.path.join(ROOT, "tests", "cpp", "instances_tiles_mock.cpp")).read()
    assert "#define SNAIL_ADAPTER_INSTANCED_TILES" in src
    r = subprocess.run([build_tiles_mock(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "compiled and linked" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_python_binding_refuses_before_the_device():
    """the argument checks that need no GPU: a null handle is refused with the function's name"""
    import ctypes as C
    from snail_amd import _lib
    cam = np.zeros(13, np.float32); v3 = np.ones(3, np.float32)
    coords = np.array([0, 0, 4, 4], np.int32); off = np.zeros(1, np.int64); data = np.full(48, 7, np.uint8)
    rc = _lib.lib().snail_instances_render_tiles(None, _lib.ptr(cam), 4, 4, _lib.ptr(coords), _lib.ptr(off), 1, None, 0, _lib.ptr(v3), _lib.ptr(v3), 0, None,
                                                 _lib.ptr(data), None)
    assert rc != 0 and b"snail_instances_render_tiles" in _lib.lib().snail_last_error() and (data == 7).all()
