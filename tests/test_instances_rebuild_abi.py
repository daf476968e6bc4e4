"""The device top-level builder's C-ABI (include/snail_instances_build.h) as a contract: its Python table matches its declarations, the
header is plain C and part of snail_instances.h, both symbols link from a C host with the header's signatures, and a null handle is
refused before any device is touched."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "snail_amd")


def test_build_signatures_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "snail_instances_build.h")).read()
    declared = sorted(set(re.findall(r"^int (snail_instances_[a-z_0-9]+)\s*\(", hdr, flags=re.M)))
    from snail_amd._lib import (INSTANCES_BUILD_SIGNATURES, INSTANCES_SHADE_SIGNATURES, INSTANCES_SIGNATURES, INSTANCES_TILES_SIGNATURES, SIGNATURES,
                                lib)
    assert sorted(INSTANCES_BUILD_SIGNATURES) == declared == ["snail_instances_read_tree", "snail_instances_rebuild_dev"]
    assert not set(INSTANCES_BUILD_SIGNATURES) & (set(SIGNATURES) | set(INSTANCES_SIGNATURES) | set(INSTANCES_SHADE_SIGNATURES) | set(INSTANCES_TILES_SIGNATURES))
    # one parameter of the header per argtype
    for name in declared:
        params = re.search(name + r"\s*\(([^;]*)\);", hdr).group(1)
        assert len(params.split(",")) == len(INSTANCES_BUILD_SIGNATURES[name][1]), name
    # included last from snail_instances.h, after the shade and tiles headers
    top = open(os.path.join(ROOT, "include", "snail_instances.h")).read()
    order = [top.index('#include "snail_instances_%s.h"' % k) for k in ("shade", "tiles", "build")]
    assert order == sorted(order)
    L = lib()
    for name in declared:
        assert hasattr(L, name), "libsnailhip.so does not export " + name


def test_build_header_is_a_c_header(tmp_path):
    exe = str(tmp_path / "instances_build_c")
    src = os.path.join(ROOT, "tests", "c", "instances_build_c.c")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", src, "-o", exe, "-L" + LIBDIR, "-lsnailhip", "-Wl,-rpath," + LIBDIR])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "C instances build ABI ok: 2 symbols" in r.stdout, (r.returncode, r.stdout, r.stderr)
    from snail_amd._lib import INSTANCES_BUILD_SIGNATURES
    assert set(re.findall(r"ADDR\((snail_[a-z0-9_]+)\)", open(src).read())) == set(INSTANCES_BUILD_SIGNATURES)


def test_rebuild_refuses_a_null_handle_before_the_device():
    from snail_amd import _lib
    L = _lib.lib()
    xf = np.zeros((3, 12), np.float32)      # (stands in for a device pointer: never read)
    perm = np.full(3, 7, np.int32); info = np.full(4, 7, np.int32)
    rc = L.snail_instances_rebuild_dev(None, _lib.ptr(xf), None, 3, _lib.ptr(perm), _lib.ptr(info), None)
    assert rc != 0 and b"snail_instances_rebuild_dev" in L.snail_last_error() and b"handle" in L.snail_last_error()
    assert (perm == 7).all() and (info == 7).all()
    for n in (0, -1, (1 << 30) + 1):
        assert L.snail_instances_rebuild_dev(None, _lib.ptr(xf), None, n, None, None, None) != 0 and b"instances" in L.snail_last_error()
    assert L.snail_instances_rebuild_dev(None, None, None, 3, None, None, None) != 0 and b"null transforms" in L.snail_last_error()
    assert L.snail_instances_read_tree(None, None, 0, None, None, None, 0, None) != 0 and b"snail_instances_read_tree" in L.snail_last_error()
