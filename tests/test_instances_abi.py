"""The instanced-scene C-ABI (include/snail_instances.h) as a contract: its Python table matches its declarations, the header is plain C
and every declared function links from a C host, and the C++ adapter's HipDBVH compiles against mock reference types."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "snail_amd")


def test_instances_signatures_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "snail_instances.h")).read()
    declared = sorted(set(re.findall(r"\b(snail_instances_[a-z_0-9]+)\s*\(", hdr)))
    from snail_amd._lib import INSTANCES_SIGNATURES, SIGNATURES, lib
    assert sorted(INSTANCES_SIGNATURES) == declared
    assert not set(INSTANCES_SIGNATURES) & set(SIGNATURES)
    L = lib()
    for name in declared:
        assert hasattr(L, name), "libsnailhip.so does not export " + name


def test_instances_header_is_a_c_header(tmp_path):
    exe = str(tmp_path / "instances_c")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", os.path.join(ROOT, "tests", "c", "instances_c.c"), "-o", exe, "-L" + LIBDIR,
                           "-lsnailhip", "-Wl,-rpath," + LIBDIR])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "C instances ABI ok: 12 symbols, 5 nodes, depth 2" in r.stdout, (r.returncode, r.stdout, r.stderr)
    src = open(os.path.join(ROOT, "tests", "c", "instances_c.c")).read()
    from snail_amd._lib import INSTANCES_SIGNATURES
    assert set(re.findall(r"ADDR\((snail_[a-z0-9_]+)\)", src)) == set(INSTANCES_SIGNATURES)


def build_instances_mock(tmp_path):
    exe = str(tmp_path / "instances_mock")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", os.path.join(ROOT, "tests", "cpp", "instances_mock.cpp"), "-o", exe,
                           "-L" + LIBDIR, "-lsnailhip", "-Wl,-rpath," + LIBDIR])
    return exe


def test_cpp_hipdbvh_compiles_and_links(tmp_path):
    out = subprocess.run([build_instances_mock(tmp_path)], capture_output=True, text=True, check=True).stdout
    assert "compiled and linked" in out
