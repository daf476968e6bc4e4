"""include/snail_wide.h, the parts that need no GPU: the cases of tests/wide_cases.py tell the walk of tests/wide_ref.py from each of its
mutations; the header is plain C, every declared symbol is exported by both libraries and bound, and the refusals come before any device
call (tests/c/wide_c.c); the Python side (snail_amd/photons.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

from snail_amd import _lib, photons
from snail_amd import scene as SC
from tests import wide_cases as WC
from tests import wide_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "snail_amd")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def walked():
    """every case under the walk and under each mutation, once"""
    cases = list(WC.small_cases()) + [WC.fuzz()]
    return {c["name"]: {m: WC.expected(c, m) for m in (None,) + WR.MUTATIONS} for c in cases}


@pytest.mark.parametrize("mutation", WR.MUTATIONS)
def test_the_cases_discriminate_each_mutation(walked, mutation):
    changed = []
    for name, res in walked.items():
        (d0, v0), (d1, v1) = res[None], res[mutation]
        if not np.array_equal(_bits(d0), _bits(d1)) or not np.array_equal(v0, v1):
            changed.append(name)
    assert changed, "no case tells %s from the walk" % mutation
    print(mutation, "changes", changed)


def test_what_the_cases_contain(walked):
    d, v = walked["root_leaf"][None]
    assert WC.bvh("two").nodes[0]["sub"] & 0x80000000 and (v[:, 0] == 0).all() and (v[:, 1] == 2).all()    # the root is a leaf: no box test
    assert (d < 0).sum() >= 2 and np.isinf(d).any()                      # rays pointing away bring negative distances back
    d, v = walked["box_subset"][None]
    c = [c for c in WC.small_cases() if c["name"] == "box_subset"][0]
    out = np.setdiff1d(np.arange(130), c["indices"])
    assert len(out) == 53 and np.array_equal(_bits(d[out]), _bits(c["dist"][out])) and (v[out] == 0).all()
    d, v = walked["axis_parallel"][None]
    assert np.isnan(d).any()
    d, v = walked["prune"][None]
    c = [c for c in WC.small_cases() if c["name"] == "prune"][0]
    assert np.isnan(d[32:48]).all() and (v[32:48, 0] == 2).all()         # a NaN distance fails every box
    assert (v[:16].sum(axis=1) <= v[48:64].sum(axis=1)).all() and (v[:16].sum() < v[48:64].sum())   # a small distance prunes
    b = WC.bvh("chain")
    assert b.depth == 63 and (b.nodes["aux"][(b.nodes["sub"] & 0x80000000) != 0] > 64).any()
    d, v = walked["chain"][None]
    assert v[:, 1].max() > 64                                            # a ray reaches the long last leaf
    d, v = walked["box_idir_same"][None]
    c = [c for c in WC.small_cases() if c["name"] == "box_idir_same"][0]
    d2, v2 = WR.wide_trace(WC.bvh("box").nodes, WC.bvh("box").tris, c["origin"], c["dir"], c["dist"])
    assert np.array_equal(_bits(d), _bits(d2)) and np.array_equal(v, v2)    # idir = 1 / dir given or computed: the same walk
    assert not np.array_equal(walked["box_idir_skew"][None][1], v)
    assert len(walked["fuzz"][None][0]) == 2000


def test_signatures_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "snail_wide.h")).read()
    declared = sorted(set(re.findall(r"^int\s+(snail_[a-z_0-9]+)\s*\(", hdr, flags=re.M)))
    S = _lib.WIDE_SIGNATURES
    assert sorted(S) == declared and len(declared) == 4, declared
    for k in dir(_lib):
        if k.endswith("SIGNATURES") and k != "WIDE_SIGNATURES":
            assert not set(S) & set(getattr(_lib, k)), k
    for L in (_lib.lib(), _lib.debug_lib()):
        for name in declared:
            assert hasattr(L, name), "%s does not export %s" % (L._name, name)
            assert getattr(L, name).argtypes == S[name][1]
            params = re.search(r"%s\s*\(([^;]*)\)\s*;" % name, hdr).group(1)
            assert len(params.split(",")) == len(S[name][1]), name
    body = re.search(r"typedef struct \{([^}]*)\} SnailPhoton;", hdr).group(1)
    assert re.findall(r"([a-z]+)(?:\[\d\])?\s*;", body) == list(photons.PHOTON.names) and photons.PHOTON.itemsize == 32
    for m in ("wide_trace", "wide_trace_host", "trace_photons", "trace_photons_host"):
        assert hasattr(SC.Scene, m), m


def test_header_is_a_c_header_and_the_refusals_before_any_device_call(tmp_path):
    exe = str(tmp_path / "wide_c")
    src = os.path.join(ROOT, "tests", "c", "wide_c.c")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", src, "-o", exe, "-L" + LIBDIR, "-lsnailhip", "-Wl,-rpath," + LIBDIR])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "C wide ABI ok: 4 symbols" in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert set(re.findall(r"ADDR\((snail_[a-z0-9_]+)\)", open(src).read())) == set(_lib.WIDE_SIGNATURES)


def test_refusals_through_the_binding():
    L = _lib.lib()
    err = lambda: L.snail_last_error().decode()      # noqa: E731
    f = np.zeros(21, dtype=np.float32)
    n = np.full(1, 7, dtype=np.int32)
    assert L.snail_wide_trace(None, -1, _lib.ptr(f), _lib.ptr(f), None, None, 0, _lib.ptr(f), 0, None, None) != 0 and "negative count" in err()
    assert L.snail_wide_trace(None, 2, _lib.ptr(f), _lib.ptr(f), None, None, 0, _lib.ptr(f), 0, None, None) != 0 and "invalid scene handle" in err()
    assert L.snail_photons_trace(None, 9, 1, _lib.ptr(f), _lib.ptr(f), _lib.ptr(f), _lib.ptr(f), _lib.ptr(n), None) != 0 and "9 lights outside 0..8" in err()
    assert n[0] == 7


def test_emit_is_deterministic_and_stratified():
    o, d = photons.emit((1.0, 2.0, 3.0), 1000, seed=5)
    o2, d2 = photons.emit((1.0, 2.0, 3.0), 1000, seed=5)
    assert o.dtype == np.float32 and d.dtype == np.float32 and o.shape == (1000, 3) and d.shape == (1000, 3)
    assert np.array_equal(o, o2) and np.array_equal(d, d2) and not np.array_equal(d, photons.emit((1.0, 2.0, 3.0), 1000, seed=6)[1])
    # unit vectors, except where the jitter takes u1 outside 0..1 (the first and last strata): there |z| > 1 and r = sqrt(max(0, .)) = 0, as in the reference
    poles = np.abs(d[:, 2]) > 1.0
    assert np.abs(np.linalg.norm(d[~poles].astype(np.float64), axis=1) - 1.0).max() < 1e-5
    assert (d[poles, :2] == 0).all() and poles.sum() < 40 and np.abs(d[poles, 2]).max() < 1.0 + 0.75 / 31
    off = o.astype(np.float64) - np.array([1.0, 2.0, 3.0])
    assert ((off * off).sum(axis=1) <= 4.0 + 1e-4).all() and np.abs(off).max() <= 2.0 + 1e-5
    # stratified: photon n lies in stratum (n % 31, n // 31) of the (u1, u2) square, jittered by at most 0.375 of a cell
    z = d[:, 2].astype(np.float64)
    u1 = (1.0 - z) / 2.0 * 31
    assert (np.abs(u1 - (np.arange(1000) % 31)) <= 0.376).all()
    assert abs(d.mean(axis=0)).max() < 0.05
    assert photons.emit((0, 0, 0), 1)[1].shape == (1, 3)


def test_the_photon_colour_rule():
    assert WR.photon_colour([2.0, -1.0, np.nan]).tolist() == [255, 0, 0, 0]
    assert WR.photon_colour([0.5, 0.999, 1.0]).tolist() == [127, 254, 255, 0]        # truncated, not rounded
