"""Test-side restatement of RenderTask::Work (src/render.cpp:47-211) around the full-shading branch of Scene<BVH>::RayTrace: per 16x16 packet
the float colour of tests/materials_ref.py (MaterialsRef.ray_trace), with gVals[7] that of tests/materials_bounce_ref.py
(BounceRef.ray_trace), with gVals[1] the depth shading of src/scene_trace.cpp:128-137 on the oracle's primary walk (it returns before the
full-shading branch: no lights, no bounce, the primary walk's counters alone); with gVals[9] the 2x2 reduction of the four double-resolution
packets, each a RayTrace call of its own; with gVals[8] the rank tint; then ConvColor and the interleaved or planar store.  The reduction, the
tint, ConvColor, both stores and the loops over packets, tiles and frames are those of tests/dbvh_tiles_ref.py (TilesRef), taken by
inheritance: only the packet's colour is stated here.  Written from src/render.cpp and include/snail_materials_tiles.h, not from the kernels.
Test infrastructure only."""
from __future__ import annotations

import numpy as np

from tests import dbvh_ref as R
from tests import dbvh_tiles_ref as T
from tests import materials_bounce_ref as B
from tests import materials_ref as M
from tests import oracle_lib as O

F = np.float32
REFLECTIONS, DEPTH, AA4 = T.REFLECTIONS, T.DEPTH, T.AA4
aa_reduce, apply_tint, planar_from_packets, tile_packets, rank_tint = T.aa_reduce, T.apply_tint, T.planar_from_packets, T.tile_packets, T.rank_tint


def new_diag(flags):
    """the diagnostics object the frames of `flags` fill: BounceDiag with the bounce, materials_ref.Diag without (depth frames fill none)"""
    return B.BounceDiag() if (flags & REFLECTIONS) and not (flags & DEPTH) else M.Diag()


class MaterialTilesRef(T.TilesRef):
    """colors / packets / frame / tiles of TilesRef (their `color` argument is without effect: the default material's colour is the set's)."""

    def __init__(self, ref: M.MaterialsRef):
        self.ref = ref
        self.bounce = B.BounceRef(ref)
        self.osc = ref.osc
        self._memo = {}

    def _packet(self, cam, resx, resy, px, py, L, depth, mode, stats, diag, pkt):
        """Scene::RayTrace of the packet at (px, py) of a resx x resy frame -> colours [64, 4, 3]"""
        lights, ambient, _, refl = L
        if depth:
            # gVals[1] (src/scene_trace.cpp:112-137): the primary walk, then Condition(t > inf, 0, Inv(t)) * (20, 250, 2) (the condition is never true)
            dd, ii = O.gen_packet(cam, resx, resy, px, py, mode)
            org = np.repeat(cam[:3].reshape(1, 3, 1), 4, axis=2).astype(np.float32)
            dist = np.full((64, 4), np.inf, dtype=np.float32); obj = np.zeros((64, 4), dtype=np.int32); bary = np.zeros((64, 8), dtype=np.float32)
            stats[2] += 256
            stats += self.osc.trace_rays(np.ascontiguousarray(org.reshape(12)), dd, ii, None, dist, obj, bary, 1, 64, True, mode)
            with np.errstate(all="ignore"):
                iv = R.inv(dist, mode)
                return np.stack([iv * F(20.0), iv * F(250.0), iv * F(2.0)], axis=-1).astype(np.float32)
        if refl:
            return self.bounce.ray_trace(cam, resx, resy, px, py, (lights, ambient), mode, stats, diag if diag is not None else B.BounceDiag(), pkt)[0]
        return self.ref.ray_trace(cam, resx, resy, px, py, (lights, ambient), mode, stats, diag if diag is not None else M.Diag(), pkt)[0]
