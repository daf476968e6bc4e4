"""The C-ABI of include/snail_materials.h as a contract, without a GPU: the header is plain C, every declared symbol is exported by
libsnailhip.so and bound in snail_amd._lib.MATERIALS_SIGNATURES, and what a set must refuse is refused before anything touches a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from snail_amd import _lib
from snail_amd import materials as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "snail_amd")


def test_signatures_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "snail_materials.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|int64_t|void|SnailMaterials \*)\s*(snail_[a-z_0-9]+)\s*\(", hdr, flags=re.M)))
    from snail_amd._lib import MATERIALS_SIGNATURES, SIGNATURES, lib
    assert sorted(MATERIALS_SIGNATURES) == declared and len(declared) == 9, declared
    assert not set(MATERIALS_SIGNATURES) & set(SIGNATURES)
    L = lib()
    for name in declared:
        assert hasattr(L, name), "libsnailhip.so does not export " + name
        assert getattr(L, name).argtypes == MATERIALS_SIGNATURES[name][1]


def test_header_is_a_c_header(tmp_path):
    exe = str(tmp_path / "materials_c")
    src = os.path.join(ROOT, "tests", "c", "materials_c.c")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", src, "-o", exe, "-L" + LIBDIR, "-lsnailhip", "-Wl,-rpath," + LIBDIR])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "C materials ABI ok: 9 symbols" in r.stdout, (r.returncode, r.stdout, r.stderr)
    from snail_amd._lib import MATERIALS_SIGNATURES
    assert set(re.findall(r"ADDR\((snail_[a-z0-9_]+)\)", open(src).read())) == set(MATERIALS_SIGNATURES)


def one_record(mat_index=0):
    return P.pack_shtris(np.zeros((1, 3, 2), np.float32), np.ones((1, 3, 3), np.float32), [mat_index])


def refused(shtris, material_map, materials, textures, word):
    """the set is refused with a text that names the reason -- with NO scene: the checks come before the handle is looked at"""
    with pytest.raises(_lib.SnailError) as e:
        P.create_set(None, shtris, material_map, materials, textures)
    assert word in str(e.value), str(e.value)


def test_transparent_kind_is_refused():
    refused(one_record(), [0], [P.Material.transparent()], [], "transparent")


@pytest.mark.parametrize("dissolve", [0.5, 1e-6, 0.999, float("nan")])
def test_uber_with_a_dissolve_between_0_and_1_is_refused(dissolve):
    refused(one_record(), [0], [P.Material.uber((1, 1, 1), (1, 1, 1), dissolve)], [], "dissolve")


@pytest.mark.parametrize("dissolve", [0.0, 1.0, -1.0, 2.0])
def test_uber_with_dissolve_0_or_1_passes_the_material_checks(dissolve):
    """... and is then stopped by the missing scene only"""
    refused(one_record(), [0], [P.Material.uber((1, 1, 1), (1, 1, 1), dissolve)], [], "invalid scene handle")


def test_non_power_of_two_texture_is_refused():
    class T:
        levels, width, height = np.zeros(64 * 48 * 3 * 2, np.uint8), 48, 64
    refused(one_record(), [0], [P.Material.textured(0)], [T], "powers of two")
    with pytest.raises(_lib.SnailError):
        P.Texture(np.zeros((64, 48, 3), np.uint8))
    with pytest.raises(_lib.SnailError):
        P.Texture(np.zeros((1, 16384, 3), np.uint8))


def test_out_of_range_entries_are_refused():
    refused(one_record(), [1], [P.Material.simple((1, 1, 1))], [], "map entry")
    refused(one_record(), [-2], [], [], "map entry")
    refused(one_record(3), [-1], [], [], "outside the map")
    refused(one_record(), [0], [P.Material.textured(0)], [], "texture index")


def test_nonzero_flags_are_refused():
    L = _lib.lib()
    cam, amb, img = np.zeros(13, np.float32), np.full(3, 0.1, np.float32), np.full(48, 7, np.uint8)
    for flags in (1, 2, 4, 0x100):
        assert L.snail_render_materials_image(None, _lib.ptr(cam), 4, 4, None, 0, _lib.ptr(amb), flags, _lib.ptr(img), 12, None) != 0
        assert b"flags" in L.snail_last_error()
        assert L.snail_render_materials_dev(None, _lib.ptr(cam), 4, 4, None, 0, _lib.ptr(amb), flags, _lib.ptr(img), 12, None, None) != 0
        assert b"flags" in L.snail_last_error()
        assert L.snail_render_materials_packets_dev(None, _lib.ptr(cam), 4, 4, None, 1, None, 0, _lib.ptr(amb), flags, _lib.ptr(img), None, None) != 0
        assert b"flags" in L.snail_last_error()
    assert (img == 7).all()


def test_pack_refuses_what_the_kernels_presuppose():
    uv, nrm = np.zeros((1, 3, 2), np.float32), np.ones((1, 3, 3), np.float32)
    for bad in (np.inf, np.nan, 2.0 ** 20):
        u = uv.copy(); u[0, 1, 0] = bad
        with pytest.raises(_lib.SnailError):
            P.pack_shtris(u, nrm, [0])
    n = nrm.copy(); n[0, 2, 2] = np.nan
    with pytest.raises(_lib.SnailError):
        P.pack_shtris(uv, n, [0])
    with pytest.raises(_lib.SnailError):
        P.pack_shtris(uv, nrm, [-1])
    with pytest.raises(_lib.SnailError):
        P.pack_shtris(uv, nrm, [0], perm=[1])


def test_a_scene_built_on_the_device_is_refused_by_the_python_class():
    """its tree may be rebuilt there, which renumbers the triangles under a set made before; and a scene without a permutation cannot be served"""
    class Bvh:
        perm = None

    class DevScene:
        _fast_dev, bvh, _h = True, Bvh, None

    class NoPerm:
        bvh, _h = Bvh, None
    z = np.zeros((1, 3, 2), np.float32), np.ones((1, 3, 3), np.float32), [0]
    with pytest.raises(_lib.SnailError, match="built on the device"):
        P.MaterialSet(DevScene(), *z)
    with pytest.raises(_lib.SnailError, match="no permutation"):
        P.MaterialSet(NoPerm(), *z)
