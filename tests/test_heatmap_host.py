"""include/snail_heatmap.h without a GPU: symbols and signatures in both libraries, the header as C, the argument checks that are answered before a
device is touched, the Python bindings' errors, and the test-side restatement of the heat colour (tests/heat_ref.py) pinned on literal bits."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from snail_amd import _lib
from tests import heat_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "snail_amd")
NAMES = ["snail_packet_stats_dev", "snail_render_heat_packets_dev", "snail_render_heat_tiles", "snail_render_heat_image",
         "snail_instances_packet_stats_dev", "snail_instances_heat_packets_dev", "snail_instances_render_heat_tiles", "snail_instances_render_heat_frame"]
DEPTH, AA4 = 2, 4


def test_signatures_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "snail_heatmap.h")).read()
    declared = re.findall(r"^int (snail_[a-z_0-9]+)\s*\(([^;]*)\);", hdr, flags=re.M | re.S)
    assert [n for n, _ in declared] == NAMES
    assert sorted(_lib.HEATMAP_SIGNATURES) == sorted(NAMES)
    for name, args in declared:
        res, argtypes = _lib.HEATMAP_SIGNATURES[name]
        assert res is C.c_int
        params = [a.strip() for a in args.replace("\n", " ").split(",")]
        assert len(params) == len(argtypes), name
        for p, t in zip(params, argtypes):
            is_ptr = "*" in p or "[" in p
            assert (t is C.c_void_p) == is_ptr and (is_ptr or t is C.c_int), (name, p)
    others = set(_lib.SIGNATURES) | set(_lib.INSTANCES_SIGNATURES) | set(_lib.INSTANCES_SHADE_SIGNATURES) | set(_lib.INSTANCES_TILES_SIGNATURES)
    assert not set(NAMES) & others
    for L in (_lib.lib(), _lib.debug_lib()):
        for name in NAMES:
            fn = getattr(L, name)
            assert fn.restype is C.c_int and list(fn.argtypes) == _lib.HEATMAP_SIGNATURES[name][1]
    src = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "HEATMAP_SIGNATURES" in src


def test_header_is_a_c_header(tmp_path):
    exe = str(tmp_path / "heatmap_c")
    src = os.path.join(ROOT, "tests", "c", "heatmap_c.c")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", src, "-o", exe, "-L" + LIBDIR, "-lsnailhip", "-Wl,-rpath," + LIBDIR])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "C heatmap ABI ok: 8 symbols" in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert set(re.findall(r"ADDR\((snail_[a-z0-9_]+)\)", open(src).read())) == set(NAMES)


def test_adapter_compiles_with_the_device_heatmap(tmp_path):
    """the Render(...) overloads with SNAIL_ADAPTER_DEVICE_HEATMAP against the mock reference types; without the macro the adapter's other mocks keep
    their routing (their own tests)"""
    src = os.path.join(ROOT, "tests", "cpp", "heatmap_mock.cpp")
    text = open(src).read()
    assert "#define SNAIL_ADAPTER_DEVICE_HEATMAP" in text and "#define SNAIL_ADAPTER_INSTANCED_TILES" in text
    exe = str(tmp_path / "heatmap_mock")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", src, "-o", exe, "-L" + LIBDIR, "-lsnailhip", "-Wl,-rpath," + LIBDIR])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "compiled and linked" in r.stdout, (r.returncode, r.stdout, r.stderr)


def _call(name, handle, flags, n_lights, out):
    """the entry point with plausible arguments, `out` as every output buffer; -> (status, message)"""
    L = _lib.lib()
    cam = np.zeros(13, np.float32)
    lights = np.ones((9, 7), np.float32)
    lp = _lib.ptr(lights) if n_lights else None
    coords = np.array([0, 0, 16, 16], np.int32); off = np.zeros(1, np.int64)
    o = _lib.ptr(out)
    tint = np.ones(3, np.float32)
    if name == "snail_instances_packet_stats_dev":
        rc = L.snail_instances_packet_stats_dev(handle, _lib.ptr(cam), 16, 16, None, 0, lp, n_lights, flags, o, None, None)
    elif name == "snail_instances_heat_packets_dev":
        rc = L.snail_instances_heat_packets_dev(handle, _lib.ptr(cam), 16, 16, None, 0, lp, n_lights, flags, _lib.ptr(tint), o, None, None, None)
    elif name == "snail_instances_render_heat_tiles":
        rc = L.snail_instances_render_heat_tiles(handle, _lib.ptr(cam), 16, 16, _lib.ptr(coords), _lib.ptr(off), 1, lp, n_lights, flags, _lib.ptr(tint), o, None)
    elif name == "snail_instances_render_heat_frame":
        rc = L.snail_instances_render_heat_frame(handle, _lib.ptr(cam), 16, 16, lp, n_lights, flags, o, 48, None)
    elif name == "snail_packet_stats_dev":
        rc = L.snail_packet_stats_dev(handle, _lib.ptr(cam), 16, 16, None, 0, lp, n_lights, flags, o, None, None)
    elif name == "snail_render_heat_packets_dev":
        rc = L.snail_render_heat_packets_dev(handle, _lib.ptr(cam), 16, 16, None, 0, lp, n_lights, flags, o, None, None, None)
    elif name == "snail_render_heat_tiles":
        rc = L.snail_render_heat_tiles(handle, _lib.ptr(cam), 16, 16, _lib.ptr(coords), _lib.ptr(off), 1, lp, n_lights, flags, o, None)
    else:
        rc = L.snail_render_heat_image(handle, _lib.ptr(cam), 16, 16, lp, n_lights, flags, o, 48, None)
    return rc, L.snail_last_error().decode()


@pytest.mark.parametrize("name", NAMES)
def test_refusals_need_no_device(name):
    """a null handle, SNAIL_RENDER_DEPTH, an unknown flag bit and nine lights: each refused with the function's name, nothing written"""
    out = np.full(16 * 16 * 3, 0xAB, np.uint8)
    rc, msg = _call(name, None, 0, 0, out)
    assert rc != 0 and name in msg and ("invalid scene handle" in msg or "invalid instances handle" in msg)
    rc, msg = _call(name, None, DEPTH, 0, out)
    assert rc != 0 and name in msg and "SNAIL_RENDER_DEPTH" in msg
    rc, msg = _call(name, None, 8, 0, out)
    assert rc != 0 and name in msg and "flag" in msg
    rc, msg = _call(name, None, 0x40000000, 1, out)
    assert rc != 0 and name in msg and "flag" in msg
    rc, msg = _call(name, None, 0, 9, out)
    assert rc != 0 and name in msg and "lights" in msg
    rc, msg = _call(name, None, 0, -1, out)
    assert rc != 0 and name in msg
    if name.endswith("packet_stats_dev"):       # counters have no antialiased form: AA4 is a flag of the three image forms only
        rc, msg = _call(name, None, AA4, 0, out)
        assert rc != 0 and name in msg and "flag" in msg
    assert (out == 0xAB).all()


def test_python_bindings_raise():
    """the Scene methods hand the library's refusal on as SnailError (no device: the handle of a closed scene is null)"""
    from snail_amd.scene import Scene
    sc = Scene.__new__(Scene)
    sc._h = None
    sc.device = 0
    cam = type("Cam", (), {"as_array13": lambda self: np.zeros(13, np.float32)})()
    with pytest.raises(_lib.SnailError, match="snail_render_heat_image"):
        sc.render_heat_image_host(cam, 16, 16)
    with pytest.raises(_lib.SnailError, match="SNAIL_RENDER_DEPTH"):
        sc.render_heat_image_host(cam, 16, 16, flags=Scene.RENDER_DEPTH)
    with pytest.raises(_lib.SnailError, match="snail_render_heat_tiles"):
        sc.render_heat_tiles_host(cam, 16, 16, [[0, 0, 16, 16]], lights7=np.ones((9, 7), np.float32))
    with pytest.raises(_lib.SnailError, match="snail_render_heat_tiles"):
        sc.render_heat_tiles_host(cam, 16, 16, [[0, 0, 16, 16]], flags=8)
    from snail_amd.instances import InstancedScene
    isc = InstancedScene.__new__(InstancedScene)
    isc._h = None
    with pytest.raises(_lib.SnailError, match="snail_instances_render_heat_frame"):
        isc.render_heat_frame_host(cam, 16, 16)
    with pytest.raises(_lib.SnailError, match="SNAIL_RENDER_DEPTH"):
        isc.render_heat_tiles_host(cam, 16, 16, [[0, 0, 16, 16]], flags=InstancedScene.RENDER_DEPTH, tint=(1, 1, 1))
    with pytest.raises(_lib.SnailError, match="snail_instances_render_heat_tiles"):
        isc.render_heat_tiles_host(cam, 16, 16, [[0, 0, 16, 16]], lights7=np.ones((9, 7), np.float32))


# literal counters -> literal float bits (r, g, b) and B,G,R bytes: the output of the program quoted in tests/heat_ref.py
PINS = [
    ((0, 0, 256, 0), (0x00000000, 0x00000000, 0x00000000), (0, 0, 0)),
    ((1, 1, 256, 1), (0x3803126F, 0x39A3D70A, 0x3E800000), (63, 0, 0)),
    ((12345, 678, 300, 2), (0x3EC5851F, 0x3E58F5C2, 0x3F000000), (127, 54, 98)),
    ((40000, 4000, 512, 3), (0x3FA00000, 0x3FA00000, 0x3F400000), (191, 255, 255)),             # r and g clamp (1.25 > 1)
    ((32000, 3200, 256, 4), (0x3F800000, 0x3F800000, 0x3F800000), (255, 255, 255)),             # skips = 4: blue saturates at exactly 1.0
    ((4000000000, 4000000000, 256, 7), (0x47F42401, 0x49989680, 0x3FE00000), (255, 255, 255)),  # counters above 2^31: the conversion is unsigned
    ((31999, 3199, 256, 0), (0x3F7FFDF5, 0x3F7FEB85, 0x00000000), (0, 254, 254)),               # just below 1: truncation, not rounding
]


@pytest.mark.parametrize("stats,bits,bgr", PINS)
def test_restatement_is_pinned(stats, bits, bgr):
    c = H.heat_rgb(np.array(stats, np.uint64))
    assert c.dtype == np.float32 and tuple(c.view(np.uint32).tolist()) == bits
    assert tuple(H.heat_bgr_bytes(stats).tolist()) == bgr
    assert tuple(H.heat_packets([stats])[0, 255].tolist()) == bgr


def test_restatement_antialiased_reduction():
    """((c + c) * 0.25) + ((c + c) * 0.25) is c exactly for every finite c without overflow (doubling and quartering are exact, x/2 + x/2 = x), so the
    antialiased bytes of a packet whose four sub-packets cost the same are the plain bytes; quadrants follow (k & 1, k >> 1)"""
    for stats, _, bgr in PINS:
        assert tuple(H.heat_aa_bgr_bytes(stats).tolist()) == bgr
    four = np.array([PINS[1][0], PINS[2][0], PINS[3][0], PINS[6][0]])
    img = H.heat_aa_packets(four[None]).reshape(16, 16, 3)
    assert tuple(img[0, 0]) == PINS[1][2] and tuple(img[0, 15]) == PINS[2][2] and tuple(img[15, 0]) == PINS[3][2] and tuple(img[8, 8]) == PINS[6][2]
    assert tuple(img[7, 7]) == PINS[1][2] and tuple(img[7, 8]) == PINS[2][2]
