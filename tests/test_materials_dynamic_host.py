"""The material set of a deforming mesh (include/snail_materials_dynamic.h), the parts that need no GPU: the header as plain C with every
declared symbol exported by both libraries and bound, the refusals that come before any device call, the Python binding, the adapter's
RebuildShaded against a mock C-ABI (tests/cpp/materials_dynamic_mock.cpp), and the numpy restatement of the face normal
(tests/shtris_dev_ref.py) against cases computed by hand."""
import os
import re
import subprocess

import numpy as np
import pytest

from snail_amd import _lib
from snail_amd import materials as P
from tests import shtris_dev_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "snail_amd")
ROCM_LIB = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
F = np.float32


def build_c_program(tmp_path):
    """tests/c/materials_dynamic_c.c against the header and the product library (and the HIP runtime, for its `gpu` mode's device memory)"""
    exe = str(tmp_path / "materials_dynamic_c")
    src = os.path.join(ROOT, "tests", "c", "materials_dynamic_c.c")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", src, "-o", exe, "-L" + LIBDIR, "-lsnailhip", "-Wl,-rpath," + LIBDIR,
                           "-L" + ROCM_LIB, "-lamdhip64", "-Wl,-rpath," + ROCM_LIB])
    return exe, src


def test_signatures_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "snail_materials_dynamic.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|SnailMaterials \*)\s*(snail_[a-z_0-9]+)\s*\(", hdr, flags=re.M)))
    S = _lib.MATERIALS_DYNAMIC_SIGNATURES
    assert sorted(S) == declared and len(declared) == 3, declared
    for other in (_lib.SIGNATURES, _lib.BVH_FAST_SIGNATURES, _lib.MATERIALS_SIGNATURES, _lib.MATERIALS_BOUNCE_SIGNATURES, _lib.MATERIALS_TILES_SIGNATURES,
                  _lib.MATERIALS_TRANSPARENCY_SIGNATURES, _lib.MATERIALS_TREE_SIGNATURES, _lib.DEBUG_SIGNATURES):
        assert not set(S) & set(other)
    for L in (_lib.lib(), _lib.debug_lib()):
        for name in declared:
            assert hasattr(L, name), "%s does not export %s" % (L._name, name)
            assert getattr(L, name).argtypes == S[name][1]
    # the test-only read-back of the records lives in the workbench build alone, and in no header
    assert hasattr(_lib.debug_lib(), "snail_materials_debug_records") and not hasattr(_lib.lib(), "snail_materials_debug_records")
    for h in os.listdir(os.path.join(ROOT, "include")):
        assert "snail_materials_debug_records" not in open(os.path.join(ROOT, "include", h)).read()
    # the older headers' lists are what they were
    assert len(_lib.MATERIALS_TREE_SIGNATURES) == 6 and len(_lib.MATERIALS_TRANSPARENCY_SIGNATURES) == 8 and len(_lib.MATERIALS_SIGNATURES) == 9 and len(_lib.BVH_FAST_SIGNATURES) == 3


def test_header_is_a_c_header(tmp_path):
    exe, src = build_c_program(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "C materials dynamic ABI ok: 3 symbols" in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert set(re.findall(r"ADDR\((snail_[a-z0-9_]+)\)", open(src).read())) == set(_lib.MATERIALS_DYNAMIC_SIGNATURES)


def test_refusals_come_before_any_device_call():
    """null arrays first, then the host-side material data through the creators' shared check (their texts, under the new function's name),
    then the handles -- a null scene is what stops a call whose host data is accepted"""
    L = _lib.lib()
    err = lambda: L.snail_last_error().decode()      # noqa: E731
    fake = np.zeros(16, np.float32)                   # never read: every call below is refused on the host
    perm = np.zeros(1, np.int32)
    mp = np.array([-1], np.int32)

    def create(uv=fake, mi=perm, pm=perm, nrm=fake, verts=None, n=1, mmap=mp, mats=(), textures=(), transparent=False, scene=None):
        recs = P._material_records(list(mats))
        tex = P._texture_array(list(textures))
        op = np.array([getattr(m, "opacity_texture", 0) for m in mats] or [0], np.int32) if transparent else None
        import ctypes as C
        h = L.snail_materials_create_dev(scene, _lib.ptr(uv), _lib.ptr(mi), None, n, _lib.ptr(pm), _lib.ptr(nrm), _lib.ptr(verts), _lib.ptr(mmap), len(mmap),
                                         _lib.ptr(recs) if len(recs) else None, len(recs), _lib.ptr(op), C.cast(tex, C.c_void_p) if len(textures) else None, len(textures), None)
        assert not h
        return err()

    assert "snail_materials_create_dev" in create(pm=None) and "perm" in create(pm=None)
    assert "null uv" in create(uv=None) and "null uv" in create(mi=None)
    assert "neither normals nor vertices" in create(nrm=None, verts=None)
    # bad host-side material data: the texts of snail_materials_create / _create_transparent
    assert "at least one triangle and one map entry" in create(n=0)
    assert "map entry 0 = 3 is outside -1..0" in create(mmap=np.array([3], np.int32), mats=[P.Material.simple((1, 1, 1))])
    assert "texture index 0 outside 0..-1" in create(mats=[P.Material.textured(0)])
    assert "transparent kind" in create(mats=[P.Material.transparent(0, 0)])                                 # the plain creator's refusal ...
    assert "dissolve 0.5 could select" in create(mats=[P.Material.uber((1, 1, 1), (0, 0, 0), 0.5)])
    assert "scene handle" in create(mats=[P.Material.uber((1, 1, 1), (0, 0, 0), 0.5)], transparent=True)      # ... and the other's acceptance
    assert "unknown kind 7" in create(mats=[P.Material(7)])

    class BadTex:
        levels, width, height = np.zeros(64, np.uint8), 12, 8
    assert "powers of two" in create(textures=[BadTex()])
    # accepted host data: the scene is looked at next
    assert "invalid scene handle" in create()
    assert "invalid scene handle" in create(nrm=None, verts=fake)
    # the set's functions
    assert L.snail_materials_rebuild_dev(None, _lib.ptr(fake), None, None, None, None) != 0 and "snail_materials_rebuild_dev: invalid material set handle" in err()
    assert L.snail_materials_update_dev(None, _lib.ptr(perm), _lib.ptr(fake), None, None, None) != 0 and "snail_materials_update_dev: invalid material set handle" in err()


def test_python_binding_and_the_older_refusal():
    """from_dev is a classmethod next to a constructor that still refuses a device-built scene (tests/test_materials_abi.py pins the text)"""
    for name in ("from_dev", "rebuild_dev", "update_dev"):
        assert hasattr(P.MaterialSet, name)
    assert isinstance(P.MaterialSet.__dict__["from_dev"], classmethod)

    class FakeScene:
        _fast_dev = True
    with pytest.raises(_lib.SnailError, match="built on the device"):
        P.MaterialSet(FakeScene(), np.zeros((1, 3, 2)), np.zeros((1, 3, 3)), [0])

    class HostScene:
        _fast_dev = False
    with pytest.raises(_lib.SnailError, match="from_fast_dev"):
        P.MaterialSet.from_dev(HostScene(), None, None)
    ms = P.MaterialSet.__new__(P.MaterialSet)          # a set of the constructor's kind has no device rebuild
    for call in (lambda: ms.rebuild_dev(None), lambda: ms.update_dev()):
        with pytest.raises(_lib.SnailError, match="from_dev"):
            call()


def test_adapter_rebuild_shaded_against_the_mock_abi(tmp_path):
    exe = str(tmp_path / "materials_dynamic_mock")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", os.path.join(ROOT, "tests", "cpp", "materials_dynamic_mock.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "materials dynamic adapter ok: scene rebuilds 3, set rebuilds 3" in r.stdout, (r.returncode, r.stdout, r.stderr)
    for name in ("adapter_mock", "heatmap_mock", "instances_tiles_mock", "materials_mock", "materials_tree_mock"):      # the header still serves the others
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-fsyntax-only", os.path.join(ROOT, "tests", "cpp", name + ".cpp")])


def test_face_normal_restatement_against_hand_computed_cases():
    # 1. the unit right triangle in the xy plane: cross = (0, 0, 1), |.|^2 = 1, RSqrt = 1
    # 2. legs 2 along y and 3 along z from (1, 1, 1): cross = (2*3 - 0*0, 0, 0) = (6, 0, 0); 36 -> sqrt 6 -> 1/6 in fp32; 6 * fl(1/6) in fp32
    # 3. b = (1, 2, 3), c = (-2, 1, 4): cross = (2*4 - 3*1, 3*-2 - 1*4, 1*1 - 2*-2) = (5, -10, 5); |.|^2 = 25 + 100 + 25 = 150
    # 4. zero area (p2 on the line p0 p1): cross = 0, 1 / sqrt(0) = inf, 0 * inf = NaN
    # 5. a denormal cross product survives: legs of 2^-70 -> cross.z = 2^-140 (a denormal), its square underflows to 0 -> inf -> inf
    tv = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]],
                   [[1, 1, 1], [1, 3, 1], [1, 1, 4]],
                   [[0.5, 0.5, 0.5], [1.5, 2.5, 3.5], [-1.5, 1.5, 4.5]],
                   [[0, 0, 0], [1, 1, 1], [2, 2, 2]],
                   [[0, 0, 0], [2.0 ** -70, 0, 0], [0, 2.0 ** -70, 0]]], dtype=F)
    n = R.face_normals(tv)
    assert n.dtype == F
    assert n[0].tolist() == [0.0, 0.0, 1.0]
    sixth = F(1) / F(6)
    assert n[1].tolist() == [float(F(6) * sixth), 0.0, 0.0]
    r150 = F(1) / np.sqrt(F(150))
    assert n[2].tolist() == [float(F(5) * r150), float(F(-10) * r150), float(F(5) * r150)]
    assert abs(float(np.linalg.norm(n[2].astype(np.float64))) - 1.0) < 1e-6
    assert np.isnan(n[3]).all()
    assert np.isnan(n[4][:2]).all() and np.isposinf(n[4][2])                  # 0 * inf, 0 * inf, 2^-140 * inf
    # the dot product is summed left to right, (x^2 + y^2) + z^2: a triangle (found by a seeded search) where x^2 + (y^2 + z^2) rounds another way
    b, c = (-2247, -1473, 550), (-1112, -1890, -1969)
    f = [F(b[1] * c[2] - b[2] * c[1]), F(b[2] * c[0] - b[0] * c[2]), F(b[0] * c[1] - b[1] * c[0])]      # (integers below 2^24: exact)
    assert [int(v) for v in f] == [3939837, -5035943, 2608854]
    sq = [F(v * v) for v in f]
    ltr, rtl = F(F(sq[0] + sq[1]) + sq[2]), F(sq[0] + F(sq[1] + sq[2]))
    assert ltr != rtl
    no = R.face_normals(np.array([[(0, 0, 0), b, c]], dtype=F))[0]
    assert no.tolist() == [float(F(v * (F(1) / np.sqrt(ltr)))) for v in f] != [float(F(v * (F(1) / np.sqrt(rtl)))) for v in f]
    # the deviation and the three vertex normals
    v = R.vertex_normals_from_faces(tv)
    assert v.shape == (5, 3, 3) and np.array_equal(v[2, 0], v[2, 1]) and np.array_equal(v[2, 0], v[2, 2]) and np.array_equal(v[2, 0], n[2])
    z, count = R.zero_nonfinite(v)
    assert count == 2 and not z[3].any() and not z[4].any() and np.array_equal(z[:3], v[:3])
    given = np.ones((2, 3, 3), F)
    given[1, 2, 1] = np.inf
    z, count = R.zero_nonfinite(given)
    assert count == 1 and z[0].all() and not z[1].any()
    # through the host pack the restatement's normals give records whose two difference vectors are zero
    rec = P.pack_shtris(np.zeros((3, 3, 2), F), v[:3], np.zeros(3, np.int32)).view(F).reshape(3, 16)
    assert np.array_equal(rec[:, 6:9], n[:3]) and not rec[:, 9:15].any()
