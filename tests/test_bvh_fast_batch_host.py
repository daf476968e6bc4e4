"""The batched fast builder (include/snail_bvh_fast_batch.h) and the one-call frame step of a deforming instanced scene
(include/snail_instances_materials_rebuild_all.h), the parts that need no GPU: the headers as plain C with every declared symbol exported by
both libraries and bound, the refusals that come before any device call (tests/c/bvh_fast_batch_c.c), the Python binding."""
import ctypes as C
import os
import re
import subprocess

import pytest

from snail_amd import _lib
from snail_amd import instances_materials as IMS
from snail_amd import scene as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "snail_amd")
HEADERS = {"snail_bvh_fast_batch.h": "BVH_FAST_BATCH_SIGNATURES", "snail_instances_materials_rebuild_all.h": "INSTANCES_MATERIALS_REBUILD_ALL_SIGNATURES"}


@pytest.mark.parametrize("header", sorted(HEADERS))
def test_signatures_match_the_header(header):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    declared = sorted(set(re.findall(r"^int\s+(snail_[a-z_0-9]+)\s*\(", hdr, flags=re.M)))
    S = getattr(_lib, HEADERS[header])
    assert sorted(S) == declared and len(declared) == 1, declared
    for k in dir(_lib):
        if k.endswith("SIGNATURES") and k != HEADERS[header]:
            assert not set(S) & set(getattr(_lib, k)), k
    for L in (_lib.lib(), _lib.debug_lib()):
        for name in declared:
            assert hasattr(L, name), "%s does not export %s" % (L._name, name)
            assert getattr(L, name).argtypes == S[name][1]
            params = re.search(r"%s\s*\(([^;]*)\)\s*;" % name, hdr).group(1)
            assert len(params.split(",")) == len(S[name][1]), name


def test_the_structure_mirror_and_the_older_tables():
    hdr = open(os.path.join(ROOT, "include", "snail_bvh_fast_batch.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} SnailFastRebuild;", hdr).group(1)
    assert re.findall(r"\*?\s*\*?([A-Za-z_0-9]+)\s*;", body) == [f[0] for f in SC._FastRebuild._fields_]
    # the headers this work sits next to keep their lists
    assert len(_lib.BVH_FAST_SIGNATURES) == 3 and len(_lib.INSTANCES_MATERIALS_DYNAMIC_SIGNATURES) == 3 and len(_lib.INSTANCES_BUILD_SIGNATURES) == 2


def test_the_product_library_exports_nothing_new_named_debug():
    def debug_symbols(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return sorted(s for s in (line.split()[-1] for line in out.splitlines() if line.strip()) if s.startswith("snail_") and "debug" in s)
    assert debug_symbols(os.path.join(LIBDIR, "libsnailhip.so")) == []
    # the test-only read of a handle's rebuild count lives in the workbench build alone, and in no header
    name = "snail_scene_debug_rebuilds"
    assert name in debug_symbols(os.path.join(LIBDIR, "libsnailhip_debug.so")) and not hasattr(_lib.lib(), name)
    for h in os.listdir(os.path.join(ROOT, "include")):
        assert name not in open(os.path.join(ROOT, "include", h)).read(), h


def test_headers_are_c_headers_and_the_refusals_before_any_device_call(tmp_path):
    exe = str(tmp_path / "bvh_fast_batch_c")
    src = os.path.join(ROOT, "tests", "c", "bvh_fast_batch_c.c")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", src, "-o", exe, "-L" + LIBDIR, "-lsnailhip", "-Wl,-rpath," + LIBDIR])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "C bvh fast batch ABI ok: 1 + 1 symbols" in r.stdout, (r.returncode, r.stdout, r.stderr)
    text = open(src).read()
    assert set(re.findall(r"ADDR\((snail_[a-z0-9_]+)\)", text)) == set(_lib.BVH_FAST_BATCH_SIGNATURES)
    assert set(re.findall(r"ALL\((snail_[a-z0-9_]+)\)", text)) == set(_lib.INSTANCES_MATERIALS_REBUILD_ALL_SIGNATURES)


def test_null_list_and_empty_list_through_the_binding():
    L = _lib.lib()
    err = lambda: L.snail_last_error().decode()      # noqa: E731
    arr = (SC._FastRebuild * 2)()
    assert L.snail_scenes_rebuild_fast_dev(None, 3, None) != 0 and "no handle listed (a null list or nList <= 0)" in err()
    for n in (0, -1):
        assert L.snail_scenes_rebuild_fast_dev(C.cast(arr, C.c_void_p), n, None) != 0 and "no handle listed (a null list or nList <= 0)" in err()
    with pytest.raises(ValueError, match="one vertex tensor"):
        SC.rebuild_fast_dev_batch([object()], [])

    class Host:
        _fast_dev = False
    with pytest.raises(_lib.SnailError, match="scene 0 was not made by from_fast_dev"):
        SC.rebuild_fast_dev_batch([Host()], [None])
    assert hasattr(IMS.InstancedMaterialSet, "rebuild_all_dev")
    ms = IMS.InstancedMaterialSet.__new__(IMS.InstancedMaterialSet)          # a set of the constructor's kind has no device rebuild
    with pytest.raises(_lib.SnailError, match="from_dev"):
        ms.rebuild_all_dev({0: (None, None)}, None)
