"""The cases of the instanced tree tests (tests/test_instances_materials_tree_host.py, tests/test_gpu_instances_materials_tree.py): `glasshouse`,
`moved` and `deep` of tests/instances_materials_transparency_cases.py, with their own cameras, lights and material lists, at 96x64 with
reflections; chosen with the restatement (tests/instances_materials_tree_ref.py) alone, on the CPU.  What they must exercise -- every mutation
of the restatement, the all-miss packets of a nested level that are mirrored all the same, B-level lanes that continue, `deep` cut at
maxDepth 2 -- is asserted on the restatement's counters in the host test, with and without a GPU.  Nothing here touches a device."""
from __future__ import annotations

import functools

import numpy as np

from tests import dbvh_shade_ref as S
from tests import instances_materials_transparency_cases as C
from tests import instances_materials_transparency_ref as IT
from tests import instances_materials_tree_ref as R
from tests import oracle_lib as O

NAMES = ("glasshouse", "moved", "deep")
FRAME = (96, 64)                   # 24 packets
AA_FRAME = (48, 32)                # 6 output packets, 24 double-resolution ones
TILE_FRAME = (88, 56)              # the last column and row of packets are partial
GPU_DEPTH = 2                      # the maxDepth of the GPU test's frames against the restatement
FULL_DEPTH = 6                     # ... and the one at which no lane of `glasshouse` and `moved` is cut: the counter is 0 (the host test's docstring has the figures)
CUT_DEPTH = 1                      # `deep` with its one pane is cut here, and nowhere deeper
TINT = (0.6, 1.0, 0.6)             # ncolors[2] of src/render.cpp:119-128
# one 16x64 tile; one that crosses the right edge; one 24x40 rect; two tiles sharing a packet (their rects overlap in the packet at (32, 32))
TILE_LISTS = {
    "column": [(16, 0, 16, 64)],
    "right_edge": [(64, 16, 32, 32)],
    "rect": [(8, 8, 24, 40)],
    "shared_packet": [(16, 16, 32, 32), (32, 32, 32, 16)],
}


def camera(name):
    """the case's own camera (`deep` has one, made for 64x48; its view does not depend on the frame size)"""
    cams = C.case(name)["cams"]
    return cams.get(FRAME[0], cams[64])


def lights_of(name, n_lights):
    """no light, or the first n of the case's own and, beyond those, of the eight of the transparency cases"""
    if not n_lights:
        return None
    own = np.asarray(C.case(name)["lights"], dtype=np.float32).reshape(-1, 7)
    more = C.lights_of(name, "eight")
    return np.ascontiguousarray(np.concatenate([own, more])[:n_lights])


@functools.lru_cache(maxsize=None)
def transp_ref(name, opaque=False):
    return IT.InstTranspRef(C.materials_ref(name, True, opaque))


@functools.lru_cache(maxsize=None)
def reference(name, mode=O.MODE_IEEE, n_lights=2, max_depth=GPU_DEPTH, bounce=True, mutation=None, frame=FRAME, xy=None, opaque=False):
    """the restatement's packet bytes [n,256,3], TreeStats, truncated lanes, counters, packet list and per-packet call records: computed once per
    argument list, shared, never changed.  xy: a packet list as a tuple of pairs, or None = the frame's grid."""
    resx, resy = frame
    pk = S.frame_packets(resx, resy) if xy is None else np.array(xy, dtype=np.int32).reshape(-1, 2)
    fr = R.InstTreeFrames(transp_ref(name, opaque), bounce=bounce, mutation=mutation)
    rec = []
    bgr, st, trunc, d = fr.render_packets(camera(name).as_array13(), resx, resy, pk, lights_of(name, n_lights), mode=mode, max_depth=max_depth, diag=R.TreeDiag(), record=rec)
    for a in (bgr, st, pk):
        a.setflags(write=False)
    return bgr, st, int(trunc), d, pk, rec


@functools.lru_cache(maxsize=None)
def tiles_ref(name, max_depth=GPU_DEPTH):
    """RenderTask::Work around the tree (4x AA, tint, planar store), memoised per argument list inside"""
    return R.InstTreeTilesRef(transp_ref(name), max_depth=max_depth)
