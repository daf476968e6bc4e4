"""Per-packet TreeStats and the gVals[5] heat-map under full shading of instanced scenes (include/snail_instances_materials_heatmap.h), the parts
that need no GPU: the header as plain C with every declared symbol exported and bound, every refusal that comes before the handle, the Python
binding, the restatement (tests/instances_materials_heat_ref.py) against the whole-frame restatement it is cut from
(tests/instances_materials_tree_ref.py), and the conditions the cases of tests/instances_materials_tree_cases.py must meet for the GPU
comparisons (tests/test_gpu_instances_materials_heat.py) to mean something.  The conditions are lower bounds on coverage, asserted on the
restatement alone: if a case misses one, the case changes, not the bound."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from snail_amd import _lib
from snail_amd import instances_materials as IM
from snail_amd import materials as P
from tests import instances_materials_heat_ref as MH
from tests import instances_materials_tree_cases as K
from tests import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "snail_amd")
REFL, DEPTH, AA = P.RENDER_REFLECTIONS, P.RENDER_DEPTH, P.RENDER_AA4
NAMES = ["snail_instances_materials_packet_stats_dev", "snail_instances_materials_heat_packets_dev", "snail_instances_materials_render_heat_tiles",
         "snail_instances_materials_render_heat_frame"]


def test_signatures_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "snail_instances_materials_heatmap.h")).read()
    assert '#include "snail_instances_materials_tree.h"' in hdr and '#include "snail_heatmap.h"' in hdr
    declared = re.findall(r"^int (snail_[a-z_0-9]+)\s*\(([^;]*)\);", hdr, flags=re.M | re.S)
    S = _lib.INSTANCES_MATERIALS_HEAT_SIGNATURES
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
        # the signature of the plain scenes' function of the same kind, with the instanced handle
        assert argtypes == _lib.MATERIALS_HEAT_SIGNATURES[name.replace("snail_instances_materials_", "snail_materials_")][1], name
    others = [v for k, v in vars(_lib).items() if k.endswith("SIGNATURES") and k != "INSTANCES_MATERIALS_HEAT_SIGNATURES"]
    assert len(others) >= 19
    for other in others:
        assert not set(S) & set(other)
    assert len(_lib.HEATMAP_SIGNATURES) == 8 and len(_lib.INSTANCES_MATERIALS_TREE_SIGNATURES) == 6 and len(_lib.MATERIALS_HEAT_SIGNATURES) == 4   # the existing lists are what they were
    for L in (_lib.lib(), _lib.debug_lib()):
        for name in NAMES:
            assert hasattr(L, name), "the library does not export " + name
            assert getattr(L, name).restype is C.c_int and list(getattr(L, name).argtypes) == S[name][1]
    assert "INSTANCES_MATERIALS_HEAT_SIGNATURES" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_header_is_a_c_header(tmp_path):
    exe = str(tmp_path / "instances_materials_heat_c")
    src = os.path.join(ROOT, "tests", "c", "instances_materials_heat_c.c")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", src, "-o", exe, "-L" + LIBDIR, "-lsnailhip", "-Wl,-rpath," + LIBDIR])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "C instances materials heat ABI ok: 4 symbols" in r.stdout, (r.returncode, r.stdout, r.stderr)
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
    if name == NAMES[0]:
        rc = L.snail_instances_materials_packet_stats_dev(None, _lib.ptr(cam13), 4, 4, None, 0, lp, n_lights, flags, depth, o, _lib.ptr(tr), None, None)
    elif name == NAMES[1]:
        rc = L.snail_instances_materials_heat_packets_dev(None, _lib.ptr(cam13), 4, 4, None, 0, lp, n_lights, flags, _lib.ptr(tnt), o, None, depth, _lib.ptr(tr), None, None)
    elif name == NAMES[2]:
        rc = L.snail_instances_materials_render_heat_tiles(None, _lib.ptr(cam13), 4, 4, _lib.ptr(coords), _lib.ptr(off), 1, lp, n_lights, flags, _lib.ptr(tnt), o, depth,
                                                           _lib.ptr(tr), None)
    else:
        rc = L.snail_instances_materials_render_heat_frame(None, _lib.ptr(cam13), 4, 4, lp, n_lights, flags, o, pitch, depth, _lib.ptr(tr), None)
    assert tr is None or tr[0] == 0
    return rc, L.snail_last_error().decode()


@pytest.mark.parametrize("name", NAMES)
def test_every_refusal_comes_before_the_handle(name):
    """the flags first (SNAIL_RENDER_DEPTH, unknown bits, AA4 on the counters), then maxDepth, the null counter, the lights, the tint, the outputs and
    the rects -- all with a null handle, which is what stops an accepted call; nothing is written"""
    out = np.full(64, 0xAB, np.uint8)
    aa_ok = name != NAMES[0]
    # the flags are named even with a bad depth and a null counter
    rc, msg = _call(name, DEPTH, 0, None, out=out)
    assert rc != 0 and name in msg and "SNAIL_RENDER_DEPTH" in msg and "flags" in msg
    rc, msg = _call(name, DEPTH | REFL | AA, out=out)
    assert rc != 0 and "SNAIL_RENDER_DEPTH" in msg
    for flags in (8, 0x100, -1 & ~DEPTH, 16 | REFL, 0x40000000):
        rc, msg = _call(name, flags, 0, None, out=out)
        assert rc != 0 and name in msg and "flags" in msg and "SNAIL_RENDER_DEPTH" not in msg, (flags, msg)
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
    if name in (NAMES[1], NAMES[2]):
        for tint in ((1.0, np.inf, 1.0), (np.nan, 1.0, 1.0)):
            rc, msg = _call(name, ok_flags, tint=tint, out=out)
            assert rc != 0 and "tint" in msg
    if name == NAMES[2]:
        for r in ([0, 0, 0, 4], [-1, 0, 4, 4], [0, 0, 4, -2]):
            rc, msg = _call(name, ok_flags, rect=r, out=out)
            assert rc != 0 and "bad rect" in msg, msg
    if name == NAMES[3]:
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
        assert hasattr(IM.InstancedMaterialSet, name)
        import inspect
        assert list(inspect.signature(getattr(IM.InstancedMaterialSet, name)).parameters) == list(inspect.signature(getattr(P.MaterialSet, name)).parameters), name
    ms = IM.InstancedMaterialSet.__new__(IM.InstancedMaterialSet)
    ms._h = None
    cam = type("Cam", (), {"as_array13": lambda self: np.zeros(13, np.float32)})()
    with pytest.raises(_lib.SnailError, match="snail_instances_materials_render_heat_frame.*handle"):
        ms.render_heat_frame_host(cam, 16, 16)
    with pytest.raises(_lib.SnailError, match="SNAIL_RENDER_DEPTH"):
        ms.render_heat_frame_host(cam, 16, 16, flags=DEPTH)
    with pytest.raises(_lib.SnailError, match="maxDepth"):
        ms.render_heat_tiles_host(cam, 16, 16, [[0, 0, 16, 16]], max_depth=9)
    with pytest.raises(_lib.SnailError, match="snail_instances_materials_render_heat_tiles.*lights"):
        ms.render_heat_tiles_host(cam, 16, 16, [[0, 0, 16, 16]], lights7=np.ones((9, 7), np.float32))


def test_no_document_still_says_not_on_the_device():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert not re.search(r"Not on the device:[^\n]*per-packet TreeStats of instanced full shading", text), doc
        assert "snail_instances_materials_heatmap.h" in text, doc


# ---- the restatement against the whole-frame restatement ----
def packet_stats(name, n_lights, bounce, depth, mode=O.MODE_IEEE, frame=K.FRAME, flags=0, xy=None):
    resx, resy = frame
    xy = K.S.frame_packets(resx, resy) if xy is None else xy
    return MH.case_ref(name).packet_stats(K.camera(name).as_array13(), resx, resy, xy, K.lights_of(name, n_lights), flags | (REFL if bounce else 0), mode, depth)


@pytest.mark.parametrize("name,n_lights,depth", [("glasshouse", 2, K.GPU_DEPTH), ("moved", 2, K.GPU_DEPTH), ("deep", 1, K.CUT_DEPTH), ("deep", 1, K.GPU_DEPTH)])
def test_the_packets_counters_sum_to_the_frame_s(name, n_lights, depth):
    ps, trunc = packet_stats(name, n_lights, True, depth)
    _, st, ftrunc, _, xy, _ = K.reference(name, O.MODE_IEEE, n_lights, depth)
    print("%s, %d lights, maxDepth %d: per packet %s; frame %s, truncated %d / %d" % (name, n_lights, depth, ps.tolist(), np.asarray(st).tolist(), trunc, ftrunc))
    assert ps.shape == (len(xy), 4) and np.array_equal(ps.sum(axis=0), np.asarray(st, dtype=np.uint64)) and trunc == ftrunc
    assert (ps[:, 2] >= 256).all()                                 # TracingRays of the primary call alone


# ---- the conditions ----
@pytest.mark.parametrize("name", ["glasshouse", "moved"])
def test_the_cases_meet_the_conditions(name):
    """conditions on the INPUTS, on the restatement alone, at FRAME (96x64, 24 packets) and GPU_DEPTH"""
    on, _ = packet_stats(name, 2, True, K.GPU_DEPTH)
    off, _ = packet_stats(name, 2, False, K.GPU_DEPTH)
    rows = np.unique(on, axis=0)
    print("%s: %d distinct counter rows of %d" % (name, len(rows), len(on)))
    assert len(on) == 24 and len(rows) >= 3
    assert (on != off).any(axis=1).any()                           # the bounce changes some packet's counters
    one, _ = packet_stats(name, 1, True, K.GPU_DEPTH)
    assert (on[:, 2] != one[:, 2]).any()                           # two lights: a `rays` word that is not one light's
    none, _ = packet_stats(name, 0, True, K.GPU_DEPTH)
    assert (one[:, 2] != none[:, 2]).any()


@pytest.mark.parametrize("name", ["glasshouse", "moved"])
def test_a_light_is_culled_for_one_packet_and_not_for_another(name):
    """with the eight lights of lights_of(name, 8): the primary call's (packet, light) pairs of the whole-frame restatement"""
    d = K.reference(name, O.MODE_IEEE, 8, K.GPU_DEPTH)[3]
    culled, kept = d.lights[0].culled, d.lights[0].not_culled
    both = sorted({n for _, n in culled} & {n for _, n in kept})
    print("%s: %d culled and %d walked (packet, light) pairs at the primary level; lights on both sides: %s" % (name, len(culled), len(kept), both))
    assert both


def test_deep_is_cut_at_cut_depth_alone_and_its_counters_differ():
    cut, tc = packet_stats("deep", 1, True, K.CUT_DEPTH)
    whole, tw = packet_stats("deep", 1, True, 2)
    print("deep: truncated %d at maxDepth %d, %d at 2; %d packets differ" % (tc, K.CUT_DEPTH, tw, int((cut != whole).any(axis=1).sum())))
    assert tc > 0 and tw == 0 and (cut != whole).any()


def test_an_all_miss_packet_books_its_256_rays():
    seen = 0
    for name in K.NAMES:
        rec = K.reference(name, O.MODE_IEEE, 1 if name == "deep" else 2, K.GPU_DEPTH)[5]
        miss = [p for p, calls in enumerate(rec) if np.isinf(calls[0]["t"]).all()]
        if not miss:
            continue
        ps, _ = packet_stats(name, 0, True, K.GPU_DEPTH, xy=K.S.frame_packets(*K.FRAME)[miss])
        print("%s: primary all-miss packets %s, counters %s" % (name, miss, ps.tolist()))
        assert (ps[:, 2] == 256).all()                             # no hit lane: nothing mirrored, no light; the primary call's rays alone
        seen += len(miss)
    assert seen >= 1


def test_aa_counters_are_the_four_sub_packets():
    name = "moved"
    resx, resy = K.AA_FRAME
    xy = K.S.frame_packets(resx, resy)
    ps, trunc = packet_stats(name, 2, True, K.GPU_DEPTH, frame=K.AA_FRAME, flags=AA)
    sub = np.array([(2 * x + 16 * (k & 1), 2 * y + 16 * (k >> 1)) for x, y in xy.tolist() for k in range(4)], dtype=np.int32)
    fr = MH.R.InstTreeFrames(K.transp_ref(name))
    _, wst, wtrunc, _ = fr.render_packets(K.camera(name).as_array13(), resx * 2, resy * 2, sub, K.lights_of(name, 2), max_depth=K.GPU_DEPTH)
    assert ps.shape == (len(xy), 4, 4) and np.array_equal(ps.reshape(-1, 4).sum(axis=0), np.asarray(wst, dtype=np.uint64)) and trunc == wtrunc
    plain = MH.heat_bytes(ps, True, None)
    tinted = MH.heat_bytes(ps, True, K.TINT)
    assert plain.shape == (len(xy), 256, 3) and (plain != tinted).any()
    assert len(np.unique(plain.reshape(-1, 3), axis=0)) >= 3
