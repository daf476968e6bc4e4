"""Per-packet TreeStats and the gVals[5] heat-map under full shading (include/snail_materials_heatmap.h), the parts that need no GPU: the header as
plain C with every declared symbol exported and bound, every refusal that comes before the handle, the Python binding, the adapter's opt-in routing
against a mock C-ABI (tests/cpp/materials_heat_mock.cpp), the restatement (tests/materials_heat_ref.py) against the whole-frame restatement it is
cut from, and the conditions `room` (tests/materials_tree_cases.py) must meet for the GPU comparisons to mean something."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from snail_amd import _lib
from snail_amd import materials as P
from tests import materials_heat_ref as MH
from tests import materials_tree_cases as K
from tests import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "snail_amd")
MODES = [O.MODE_IEEE, O.MODE_SSE]
REFL, DEPTH, AA = P.RENDER_REFLECTIONS, P.RENDER_DEPTH, P.RENDER_AA4
NAMES = ["snail_materials_packet_stats_dev", "snail_materials_heat_packets_dev", "snail_materials_render_heat_tiles", "snail_materials_render_heat_frame"]


def test_signatures_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "snail_materials_heatmap.h")).read()
    declared = re.findall(r"^int (snail_[a-z_0-9]+)\s*\(([^;]*)\);", hdr, flags=re.M | re.S)
    S = _lib.MATERIALS_HEAT_SIGNATURES
    assert [n for n, _ in declared] == NAMES and sorted(S) == sorted(NAMES)
    for name, args in declared:
        res, argtypes = S[name]
        assert res is C.c_int
        params = [a.strip() for a in args.replace("\n", " ").split(",")]
        assert len(params) == len(argtypes), name
        for p, t in zip(params, argtypes):
            is_ptr = "*" in p or "[" in p
            assert (t is C.c_void_p) == is_ptr and (is_ptr or t is C.c_int), (name, p)
        assert "ambient" not in args
    for other in (_lib.SIGNATURES, _lib.HEATMAP_SIGNATURES, _lib.MATERIALS_SIGNATURES, _lib.MATERIALS_TILES_SIGNATURES, _lib.MATERIALS_TRANSPARENCY_SIGNATURES,
                  _lib.MATERIALS_TREE_SIGNATURES, _lib.MATERIALS_DYNAMIC_SIGNATURES):
        assert not set(S) & set(other)
    assert len(_lib.HEATMAP_SIGNATURES) == 8 and len(_lib.MATERIALS_TREE_SIGNATURES) == 6            # the existing headers' lists are what they were
    for L in (_lib.lib(), _lib.debug_lib()):
        for name in NAMES:
            assert hasattr(L, name), "the library does not export " + name
            assert getattr(L, name).restype is C.c_int and list(getattr(L, name).argtypes) == S[name][1]
    assert "MATERIALS_HEAT_SIGNATURES" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_header_is_a_c_header(tmp_path):
    exe = str(tmp_path / "materials_heat_c")
    src = os.path.join(ROOT, "tests", "c", "materials_heat_c.c")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", src, "-o", exe, "-L" + LIBDIR, "-lsnailhip", "-Wl,-rpath," + LIBDIR])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "C materials heat ABI ok: 4 symbols" in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert set(re.findall(r"ADDR\((snail_[a-z0-9_]+)\)", open(src).read())) == set(NAMES)


def _call(name, flags=0, depth=8, trunc="own", n_lights=0, tint=None, out=None, rect=(0, 0, 4, 4), cam=True, pitch=12):
    """the entry point with a NULL handle and plausible arguments otherwise, `out` as every output buffer -> (status, message)"""
    L = _lib.lib()
    cam13 = np.zeros(13, np.float32) if cam else None
    lights = np.ones((9, 7), np.float32)
    lp = _lib.ptr(lights) if n_lights else None
    tr = np.zeros(1, np.uint64) if trunc == "own" else trunc
    coords = np.array(rect, np.int32); off = np.zeros(1, np.int64)
    o = _lib.ptr(out)
    tnt = None if tint is None else np.asarray(tint, np.float32)
    if name == "snail_materials_packet_stats_dev":
        rc = L.snail_materials_packet_stats_dev(None, _lib.ptr(cam13), 4, 4, None, 0, lp, n_lights, flags, depth, o, _lib.ptr(tr), None, None)
    elif name == "snail_materials_heat_packets_dev":
        rc = L.snail_materials_heat_packets_dev(None, _lib.ptr(cam13), 4, 4, None, 0, lp, n_lights, flags, _lib.ptr(tnt), o, None, depth, _lib.ptr(tr), None, None)
    elif name == "snail_materials_render_heat_tiles":
        rc = L.snail_materials_render_heat_tiles(None, _lib.ptr(cam13), 4, 4, _lib.ptr(coords), _lib.ptr(off), 1, lp, n_lights, flags, _lib.ptr(tnt), o, depth, _lib.ptr(tr), None)
    else:
        rc = L.snail_materials_render_heat_frame(None, _lib.ptr(cam13), 4, 4, lp, n_lights, flags, o, pitch, depth, _lib.ptr(tr), None)
    assert tr is None or tr[0] == 0
    return rc, L.snail_last_error().decode()


@pytest.mark.parametrize("name", NAMES)
def test_every_refusal_comes_before_the_handle(name):
    """the flags first (SNAIL_RENDER_DEPTH, unknown bits, AA4 on the counters), then maxDepth, the null counter, the lights, the tint, the outputs and
    the rects -- all with a null handle, which is what stops an accepted call; nothing is written"""
    out = np.full(64, 0xAB, np.uint8)
    aa_ok = name != "snail_materials_packet_stats_dev"
    # the flags are named even with a bad depth and a null counter
    rc, msg = _call(name, DEPTH, 0, None, out=out)
    assert rc != 0 and name in msg and "SNAIL_RENDER_DEPTH" in msg and "flags" in msg
    rc, msg = _call(name, DEPTH | REFL | AA, out=out)
    assert rc != 0 and "SNAIL_RENDER_DEPTH" in msg
    for flags in (8, 0x100, -1 & ~DEPTH, 16 | REFL, 0x40000000):
        rc, msg = _call(name, flags, 0, None, out=out)
        assert rc != 0 and name in msg and "flags" in msg, (flags, msg)
    rc, msg = _call(name, AA, 0, None, out=out)
    assert rc != 0 and (("maxDepth" in msg) if aa_ok else ("flags" in msg)), msg
    ok_flags = (REFL | AA) if aa_ok else REFL
    for depth in (-1, 0, 9):
        rc, msg = _call(name, ok_flags, depth, None, out=out)
        assert rc != 0 and name in msg and "maxDepth" in msg, msg
    rc, msg = _call(name, ok_flags, 8, None, out=out)
    assert rc != 0 and "truncated" in msg, msg
    rc, msg = _call(name, ok_flags, cam=False, out=out)
    assert rc != 0 and name in msg and "camera" in msg
    for n_lights in (9, -1):
        rc, msg = _call(name, ok_flags, n_lights=n_lights, out=out)
        assert rc != 0 and name in msg and "lights" in msg, msg
    if name in ("snail_materials_heat_packets_dev", "snail_materials_render_heat_tiles"):
        rc, msg = _call(name, ok_flags, tint=(1.0, np.inf, 1.0), out=out)
        assert rc != 0 and "tint" in msg
    if name == "snail_materials_render_heat_tiles":
        for r in ([0, 0, 0, 4], [-1, 0, 4, 4], [0, 0, 4, -2]):
            rc, msg = _call(name, ok_flags, rect=r, out=out)
            assert rc != 0 and "bad rect" in msg, msg
    if name == "snail_materials_render_heat_frame":
        rc, msg = _call(name, ok_flags, pitch=11, out=out)
        assert rc != 0 and "pitch" in msg
    rc, msg = _call(name, ok_flags, out=None)                      # a null output
    assert rc != 0 and name in msg and "handle" not in msg, msg
    if name.endswith("_dev"):
        rc, msg = _call(name, ok_flags, out=out[1:])               # an unaligned one
        assert rc != 0 and "aligned" in msg, msg
    # an accepted call: the handle is what stops it, for every accepted flag combination
    for flags in ((0, REFL, AA, REFL | AA) if aa_ok else (0, REFL)):
        rc, msg = _call(name, flags, 1, n_lights=8, out=out)
        assert rc != 0 and name in msg and "handle" in msg, (flags, msg)
    assert (out == 0xAB).all()


def test_python_binding():
    for name in ("packet_stats", "render_heat_packets", "render_heat_tiles_host", "render_heat_frame_host"):
        assert hasattr(P.MaterialSet, name)
    ms = P.MaterialSet.__new__(P.MaterialSet)
    ms._h = None
    cam = type("Cam", (), {"as_array13": lambda self: np.zeros(13, np.float32)})()
    with pytest.raises(_lib.SnailError, match="snail_materials_render_heat_frame.*handle"):
        ms.render_heat_frame_host(cam, 16, 16)
    with pytest.raises(_lib.SnailError, match="SNAIL_RENDER_DEPTH"):
        ms.render_heat_frame_host(cam, 16, 16, flags=DEPTH)
    with pytest.raises(_lib.SnailError, match="maxDepth"):
        ms.render_heat_tiles_host(cam, 16, 16, [[0, 0, 16, 16]], max_depth=9)
    with pytest.raises(_lib.SnailError, match="snail_materials_render_heat_tiles.*lights"):
        ms.render_heat_tiles_host(cam, 16, 16, [[0, 0, 16, 16]], lights7=np.ones((9, 7), np.float32))


# ---- the adapter, against a mock C-ABI ----
def build_mock(tmp_path, name, *defines):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread"] + ["-D" + d for d in defines] +
                          [os.path.join(ROOT, "tests", "cpp", "materials_heat_mock.cpp"), "-o", exe])
    return exe


def test_adapter_routing_against_the_mock_abi(tmp_path):
    M, T, H = "SNAIL_ADAPTER_DEVICE_MATERIALS", "SNAIL_ADAPTER_DEVICE_TRANSPARENCY", "SNAIL_ADAPTER_DEVICE_MATERIALS_HEATMAP"
    # the new routing with the macro: any set with the transparency opt-in, a set that cannot select without it
    full = build_mock(tmp_path, "full", M, T, H)
    r = subprocess.run([full, "routing"], capture_output=True, text=True)
    assert r.returncode == 0 and "ok (with %s, with %s)" % (H, T) in r.stdout and "_heat_ 4 + 4 times" in r.stdout, (r.returncode, r.stdout, r.stderr)
    r = subprocess.run([full, "truncated"], capture_output=True, text=True)
    assert r.returncode == 0 and "rendered again by the host renderer" in r.stdout, (r.returncode, r.stdout, r.stderr)
    part = build_mock(tmp_path, "part", M, H)
    r = subprocess.run([part, "routing"], capture_output=True, text=True)
    assert r.returncode == 0 and "ok (with %s, without %s)" % (H, T) in r.stdout and "_heat_ 2 + 2 times" in r.stdout, (r.returncode, r.stdout, r.stderr)
    # without the new macro: today's routing -- gVals[5] under full shading is the host renderer's, _heat_ is never reached
    old = build_mock(tmp_path, "old", M, T)
    r = subprocess.run([old, "routing"], capture_output=True, text=True)
    assert r.returncode == 0 and "ok (without %s" % H in r.stdout and "_heat_ 0 + 0 times" in r.stdout, (r.returncode, r.stdout, r.stderr)
    # the new macro without SNAIL_ADAPTER_DEVICE_MATERIALS is without effect
    alone = build_mock(tmp_path, "alone", H, T)
    r = subprocess.run([alone, "truncated"], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)


def test_adapter_aborts_without_a_host_renderer(tmp_path):
    """SNAIL_ADAPTER_NO_HOST_RENDERER: a heat frame whose counter moved aborts with a message naming the depth (a child process, on the CPU)"""
    exe = build_mock(tmp_path, "nohost", "SNAIL_ADAPTER_DEVICE_MATERIALS", "SNAIL_ADAPTER_DEVICE_TRANSPARENCY", "SNAIL_ADAPTER_DEVICE_MATERIALS_HEATMAP", "SNAIL_ADAPTER_NO_HOST_RENDERER")
    r = subprocess.run([exe, "truncated"], capture_output=True, text=True)
    assert r.returncode == -6 and "maxDepth 8" in r.stderr and "SNAIL_ADAPTER_NO_HOST_RENDERER" in r.stderr, (r.returncode, r.stdout, r.stderr)


def test_the_other_mocks_still_compile():
    for name in ("adapter_mock", "heatmap_mock", "instances_tiles_mock", "materials_mock", "materials_dynamic_mock"):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-fsyntax-only", os.path.join(ROOT, "tests", "cpp", name + ".cpp")])
    for defines in ([], ["-DSNAIL_ADAPTER_DEVICE_MATERIALS", "-DSNAIL_ADAPTER_DEVICE_TRANSPARENCY"]):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-fsyntax-only"] + defines + [os.path.join(ROOT, "tests", "cpp", "materials_tree_mock.cpp")])


# ---- the restatement against the whole-frame restatement ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bounce", [True, False])
@pytest.mark.parametrize("resx,resy", K.FRAMES)
def test_the_packets_counters_sum_to_the_frame_s(resx, resy, bounce, mode):
    c = K.room()
    xy = K.frame_packets(resx, resy)
    ps, trunc = MH.room_ref().packet_stats(c["cam"].as_array13(), resx, resy, xy, c["lights"], REFL if bounce else 0, mode, 8)
    _, st, ftrunc, _ = K.diag_frame(resx, resy, mode, 8, "case", bounce)
    print("%dx%d bounce=%d mode=%d: per packet %s; frame %s" % (resx, resy, bounce, mode, ps.tolist(), np.asarray(st).tolist()))
    assert ps.shape == (len(xy), 4) and np.array_equal(ps.sum(axis=0), np.asarray(st, dtype=np.uint64)) and trunc == ftrunc == 0
    assert (ps[:, 2] >= 256).all()                                 # TracingRays of the primary call alone


# ---- the conditions ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("resx,resy", K.FRAMES)
def test_room_meets_the_conditions(resx, resy, mode):
    """conditions on the INPUTS, on the restatement alone"""
    c = K.room()
    ref = MH.room_ref()
    cam13 = c["cam"].as_array13()
    xy = K.frame_packets(resx, resy)
    # at least three distinct colours in the heat frame, with and without AA
    for flags in (REFL, REFL | AA):
        frame, _, _ = ref.heat_frame(cam13, resx, resy, c["lights"], flags, mode, 8)
        colours = np.unique(frame.reshape(-1, 3), axis=0)
        print("%dx%d mode=%d flags=%d: %d distinct colours" % (resx, resy, mode, flags, len(colours)))
        assert len(colours) >= 3
    # a packet whose counters the bounce changes
    on, _ = ref.packet_stats(cam13, resx, resy, xy, c["lights"], REFL, mode, 8)
    off, _ = ref.packet_stats(cam13, resx, resy, xy, c["lights"], 0, mode, 8)
    assert (on != off).any(axis=1).any()
    # a packet whose counters are not simple shading's, with which the heat-map of include/snail_heatmap.h would pass: the packets are the frame's
    # own, so per-packet counters that were equal would sum to the oracle's simple-shading frame, bounce on or off
    for bounce, got in ((True, on), (False, off)):
        simple = c["osc"].render_whitted(cam13, resx, resy, np.asarray(c["lights"], dtype=np.float32), mode=mode, reflections=bounce, threads=1)[1]
        print("   bounce=%d: full shading %s, simple shading %s" % (bounce, got.sum(axis=0).tolist(), np.asarray(simple).tolist()))
        assert not np.array_equal(got.sum(axis=0), np.asarray(simple, dtype=np.uint64))
    # the cut: D = 2 moves the counter, D = 8 does not; and it changes a packet's counters
    d2, t2 = ref.packet_stats(cam13, resx, resy, xy, c["lights"], REFL, mode, 2)
    _, t8 = ref.packet_stats(cam13, resx, resy, xy, c["lights"], REFL, mode, 8)
    assert t2 > 0 and t8 == 0 and (d2 != on).any()
    # culled (packet, light) pairs and packets that drop out of levels are test_materials_tree_host.py's conditions on the same frames
    _, _, trunc, d = K.diag_frame(resx, resy, mode, 8)
    K.check_conditions_depth8(d, len(xy))
