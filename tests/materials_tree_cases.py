"""Inputs of the tests of include/snail_materials_tree.h (tests/test_materials_tree_host.py, tests/test_gpu_materials_tree.py), chosen with the
restatement alone, on the CPU.  Scene `room`: the six rects and the materials of `panes` (tests/materials_transparency_cases.py), MOVED -- twice
as wide and as high and shifted by (2.4, 0.7), so that at 3 x 2 packets a nested packet is hit in all 256 lanes while others miss altogether or
drop out of a level -- and a wall BEHIND the camera, one TEX triangle and one TRANSPARENT triangle, so that the mirrored rays of the primary
packets hit something and the B chains end on something (or go on through it).  Frames 48 x 32 (3 x 2 packets) and 38 x 26 (the last column and row partial); with 4x AA 96 x 64 and
76 x 52.  Seeded numpy, float32; nothing here touches the product library."""
from __future__ import annotations

import functools

import numpy as np

from tests import materials_transparency_cases as TK
from tests import materials_tree_ref as TR
from tests import oracle_lib as O

FRAMES = [(48, 32), (38, 26)]
TINT = (0.9, 0.55, 1.2)
WALL_Z = -4.5
PANES_SCALE, PANES_SHIFT = 2.0, (2.4, 0.7)
STAGE_FRAME = (96, 64)             # the stage test's level-1 packets: 24 of them


@functools.lru_cache(maxsize=None)
def room():
    """-> dict in the form of materials_cases.case(): panes(), moved, + two triangles at z = WALL_Z"""
    p = TK.panes()
    panes_tv = p["tv"].copy()
    panes_tv[:, :, 0:2] *= np.float32(PANES_SCALE)
    panes_tv[:, :, 0] += np.float32(PANES_SHIFT[0]); panes_tv[:, :, 1] += np.float32(PANES_SHIFT[1])
    x0, x1, y0, y1, z = -3.4, 3.6, -2.3, 2.6, WALL_Z
    a, b, c, d = (x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)
    wall = [(a, b, c), (a, c, d)]
    tv = np.ascontiguousarray(np.concatenate([panes_tv, np.array(wall, dtype=np.float32)]))
    uv = np.concatenate([p["uv"], np.array([[(0.31 * v[0] + 0.2, 0.29 * v[1] + 0.1) for v in tri] for tri in wall], dtype=np.float32)])
    rng = np.random.RandomState(47)
    nrm = np.concatenate([p["nrm"], (np.array([0.0, 0.0, 1.0]) + (rng.rand(2, 3, 3) - 0.5) * 0.5).astype(np.float32)])
    mat_index = np.concatenate([p["mat_index"], np.array([5, 3], dtype=np.int32)])          # TEX, TRANSPARENT
    c = dict(p)
    c.update(tv=tv, osc=O.OracleScene(tv), uv=uv.astype(np.float32), nrm=nrm, mat_index=mat_index.astype(np.int32), flat=np.arange(len(tv)) % 3 == 1)
    return c


def room_tr(opaque=False):
    """the TranspRef of `room` (opaque: with the stand-ins of materials_transparency_cases.case_ref)"""
    return TK.case_ref(room(), opaque).tr


@functools.lru_cache(maxsize=None)
def tiles_ref(max_depth=8, opaque=False):
    """the tile restatement of `room` at one depth; shared (its memo is what keeps the tests' references from being computed twice)"""
    return TR.TreeTilesRef(room_tr(opaque), max_depth)


@functools.lru_cache(maxsize=None)
def frame_packets(resx, resy):
    from tests import dbvh_shade_ref as S
    return np.asarray(S.frame_packets(resx, resy), dtype=np.int32).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def diag_frame(resx, resy, mode, max_depth, lights="case", bounce=True):
    """TreeFrames over the whole frame -> (bytes [n,256,3], stats, truncated, TreeDiag)"""
    c = room()
    fr = TR.TreeFrames(room_tr(), bounce)
    out = fr.render_packets(c["cam"].as_array13(), resx, resy, frame_packets(resx, resy), TK.lights_of(c, lights), mode=mode, max_depth=max_depth)
    out[0].setflags(write=False)
    return out


def describe(d):
    return ("A calls %s; B calls %s; mirrored <0,0> %s <0,1> %s all-miss %s; truncated A %d B %d; culled pairs A %s B %s" % (
        dict(sorted(d.a_calls.items())), dict(sorted(d.b_calls.items())), dict(d.mirrored_full), dict(d.mirrored_masked), dict(d.mirrored_all_miss), d.truncated_a,
        d.truncated_b, {k: len(v.culled) for k, v in sorted(d.lights.items())}, {k: len(v.culled) for k, v in sorted(d.b_lights.items()) if len(v.culled)}))


def check_conditions_depth8(d, n_packets):
    """what a frame at D = 8 with the bounce must exercise for a comparison over it to mean something; both of FRAMES do, in both arithmetics"""
    assert d.truncated == 0
    assert any(depth - k >= 3 for (k, depth) in d.b_calls), "no B chain reaches 3 levels below its mirror"
    deep = [k for k in d.a_calls if k >= 1]
    assert any(d.mirrored_masked.get(k, 0) for k in deep) and any(d.mirrored_full.get(k, 0) for k in deep) and any(d.mirrored_all_miss.get(k, 0) for k in deep), \
        (d.mirrored_masked, d.mirrored_full, d.mirrored_all_miss)
    # a packet that is not part of a level: fewer calls than packets, and its B chain with it
    assert any(0 < d.a_calls[k] < n_packets and d.b_calls.get((k, k), 0) == d.a_calls[k] for k in deep), d.a_calls
    assert any(len(v.culled) >= 1 and len(v.not_culled) >= 1 for v in d.b_lights.values()), "no (packet, light) culled at a B level"
