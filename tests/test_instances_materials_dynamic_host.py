"""Full shading of instanced scenes whose BLASes deform on the device (include/snail_instances_materials_dynamic.h), the parts that need no
GPU: the header as plain C with every declared symbol exported by both libraries and bound, the refusals that come before any device call with
their texts (tests/c/instances_materials_dynamic_c.c), the Python binding, the poses of the GPU tests
(tests/instances_materials_dynamic_cases.py), and the documents that named the older refusal."""
import os
import re
import subprocess

import numpy as np
import pytest

from snail_amd import _lib
from snail_amd import instances_materials as IMS
from tests import instances_materials_dynamic_cases as DK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "snail_amd")
HEADER = "snail_instances_materials_dynamic.h"
OLDER = ["snail_instances_materials.h", "snail_instances_materials_bounce.h", "snail_instances_materials_transparency.h", "snail_instances_materials_tree.h",
         "snail_instances_materials_heatmap.h"]


def test_signatures_match_the_header():
    hdr = open(os.path.join(ROOT, "include", HEADER)).read()
    declared = sorted(set(re.findall(r"^(?:int|SnailInstancesMaterials \*)\s*(snail_[a-z_0-9]+)\s*\(", hdr, flags=re.M)))
    S = _lib.INSTANCES_MATERIALS_DYNAMIC_SIGNATURES
    assert sorted(S) == declared and len(declared) == 3, declared
    others = [getattr(_lib, k) for k in dir(_lib) if k.endswith("SIGNATURES") and k != "INSTANCES_MATERIALS_DYNAMIC_SIGNATURES"]
    assert len(others) >= 20
    for other in others:
        assert not set(S) & set(other)
    for L in (_lib.lib(), _lib.debug_lib()):
        for name in declared:
            assert hasattr(L, name), "%s does not export %s" % (L._name, name)
            assert getattr(L, name).argtypes == S[name][1]
    # the test-only read-back of the records lives in the workbench build alone, and in no header
    name = "snail_instances_materials_debug_records"
    assert hasattr(_lib.debug_lib(), name) and not hasattr(_lib.lib(), name)
    for h in os.listdir(os.path.join(ROOT, "include")):
        assert name not in open(os.path.join(ROOT, "include", h)).read()
    # plain C, included by no other header; the older headers' lists are what they were
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h != HEADER:
            assert '#include "%s"' % HEADER not in open(os.path.join(ROOT, "include", h)).read(), h
    assert len(_lib.INSTANCES_MATERIALS_SIGNATURES) == 6 and len(_lib.INSTANCES_MATERIALS_TRANSPARENCY_SIGNATURES) == 8 and len(_lib.MATERIALS_DYNAMIC_SIGNATURES) == 3
    # the ctypes mirrors of the two structures against the header's field lists
    for struct, cls in (("SnailBlasShadingDev", IMS._BlasShadingDev), ("SnailBlasRebuild", IMS._BlasRebuild)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, hdr).group(1)
        fields = re.findall(r"\*?\s*\*?([A-Za-z_0-9]+)\s*;", body)
        assert fields == [f[0] for f in cls._fields_], (struct, fields)


def test_header_is_a_c_header_and_the_refusals_before_any_device_call(tmp_path):
    exe = str(tmp_path / "instances_materials_dynamic_c")
    src = os.path.join(ROOT, "tests", "c", "instances_materials_dynamic_c.c")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", src, "-o", exe, "-L" + LIBDIR, "-lsnailhip", "-Wl,-rpath," + LIBDIR])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "C instances materials dynamic ABI ok: 3 symbols" in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert set(re.findall(r"ADDR\((snail_[a-z0-9_]+)\)", open(src).read())) == set(_lib.INSTANCES_MATERIALS_DYNAMIC_SIGNATURES)


def test_refusals_through_the_binding():
    """the same refusals through ctypes, for the texts the C program does not look at; and the older creators' text is today's"""
    import ctypes as C
    L = _lib.lib()
    err = lambda: L.snail_last_error().decode()      # noqa: E731
    fake = np.zeros(16, np.float32)                   # never read: every call below is refused on the host
    arr = (IMS._BlasRebuild * 2)()
    for fn in (L.snail_instances_materials_rebuild_dev, L.snail_instances_materials_update_dev):
        assert fn(None, None, 0, None) != 0 and "no BLAS listed" in err()
        assert fn(None, C.cast(arr, C.c_void_p), -3, None) != 0 and "no BLAS listed" in err()
    arr[0].blas, arr[1].blas = 1, 1
    arr[0].d_verts9 = arr[1].d_verts9 = fake.ctypes.data
    arr[0].d_perm = arr[1].d_perm = fake.ctypes.data
    assert L.snail_instances_materials_rebuild_dev(None, C.cast(arr, C.c_void_p), 2, None) != 0 and "entry 1: BLAS 1 is listed twice (entry 0)" in err()
    arr[1].blas = -7
    assert L.snail_instances_materials_update_dev(None, C.cast(arr, C.c_void_p), 2, None) != 0 and "entry 1: BLAS index -7 is out of range" in err()
    arr[1].blas = 0
    assert L.snail_instances_materials_rebuild_dev(None, C.cast(arr, C.c_void_p), 2, None) != 0 and "invalid instanced material set handle" in err()
    src = open(os.path.join(ROOT, "snail_amd", "csrc", "instances_materials_host.inc")).read()
    assert "BLAS %d is rebuilt on the device, which renumbers its triangles: no records for such a BLAS here" in src


def test_python_binding_and_the_older_refusal():
    for name in ("from_dev", "rebuild_blas_dev", "update_blas_dev"):
        assert hasattr(IMS.InstancedMaterialSet, name)
    assert isinstance(IMS.InstancedMaterialSet.__dict__["from_dev"], classmethod)
    d = IMS.DevBlasShading("uv", "mi", None, [-1], d_verts="v")
    assert (d.d_uv, d.d_mat_index, d.d_flat, d.material_map, d.d_nrm, d.d_verts) == ("uv", "mi", None, [-1], None, "v")

    class FastScene:
        _fast_dev = True

    class HostScene:
        _fast_dev = False

    class FakeInstanced:
        blas = [FastScene(), HostScene()]
    data = (np.zeros((1, 3, 2)), np.zeros((1, 3, 3)), [0], None, [-1])
    # the constructor keeps refusing a device-built BLAS with its present text
    with pytest.raises(_lib.SnailError, match="BLAS 0 carries no host permutation"):
        IMS.InstancedMaterialSet(FakeInstanced(), [data, data])
    # from_dev wants each BLAS's data in the form that fits it
    with pytest.raises(_lib.SnailError, match="BLAS 0: a Scene.from_fast_dev BLAS takes a DevBlasShading"):
        IMS.InstancedMaterialSet.from_dev(FakeInstanced(), [data, data])
    with pytest.raises(_lib.SnailError, match="shading data of 1 BLASes for an instanced scene of 2"):
        IMS.InstancedMaterialSet.from_dev(FakeInstanced(), [data])
    ms = IMS.InstancedMaterialSet.__new__(IMS.InstancedMaterialSet)          # a set of the constructor's kind has no device rebuild
    for call in (lambda: ms.rebuild_blas_dev({0: (None, None)}), lambda: ms.update_blas_dev({0: (None, None)})):
        with pytest.raises(_lib.SnailError, match="from_dev"):
            call()


def test_the_poses_differ_in_perm_and_root_box():
    moved, ba, bb = DK.check_poses()
    print("sheet: %d of %d slots hold another triangle; root boxes %s / %s" % (moved, len(DK.poses()["uv"]), ba.tolist(), bb.tolist()))
    p = DK.poses()
    assert p["A"][0].shape == p["B"][0].shape and (p["A"][1] != p["B"][1]).any()
    # shared vertices stay shared: equal positions in A are equal in B
    va, vb = p["A"][0].reshape(-1, 3), p["B"][0].reshape(-1, 3)
    _, first, inv = np.unique(va, axis=0, return_index=True, return_inverse=True)
    assert np.array_equal(vb, vb[first][inv.ravel()])


def test_documents_point_to_the_new_header():
    inc = os.path.join(ROOT, "include")
    for h in OLDER + ["snail_materials_dynamic.h"]:
        assert HEADER in open(os.path.join(inc, h)).read(), h
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert HEADER in open(os.path.join(ROOT, doc)).read(), doc
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    start = integ.index("### Instanced scenes whose BLASes deform (`include/%s`)" % HEADER)      # the per-frame call sequence of the subsection
    at = [integ.index(s, start) for s in ("snail_instances_materials_rebuild_dev(set", "snail_instances_rebuild_dev(instances", "snail_instances_render_materials_dev(set")]
    assert at[0] < at[1] < at[2]
    res = open(os.path.join(ROOT, "profiles", "instances_materials_dynamic_resources.txt")).read()
    assert "0 of them missing or different after; 2 new kernels" in res
    for k in ("k_ishd_pack", "k_ishd_info"):          # the new kernels' rows: VGPRs, SGPRs, scratch bytes per lane, spills, occupancy
        row = re.search(r"\|\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+devshd::%s\(" % k, res)
        assert row and [int(row.group(i)) for i in (3, 4, 5)] == [0, 0, 0], k
    assert "LDS Size" in res
