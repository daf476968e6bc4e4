"""Test-side restatement of per-packet TreeStats and the gVals[5] heat-map under full shading of an INSTANCED scene
(include/snail_instances_materials_heatmap.h): the instanced twin of tests/materials_heat_ref.py.

A packet's Scene<DBVH>::RayTrace call is independent of every other packet's, and its TreeStats is what the call added up
(src/scene_trace.cpp:116-120, :459, :476, :496-502): so the counters of packet p ARE the TreeStats of tests/instances_materials_tree_ref.py's
InstTreeFrames.render_packets over the one-packet list [p], and its truncated lanes that run's count.  With 4x AA the same over the four
double-resolution sub-packets (sub-packet k of the packet at (x, y) lies at (2x + 16 (k & 1), 2y + 16 (k >> 1)) of the doubled frame), each a
RayTrace call with a tree of its own.  The colour of the counters and ConvColor are tests/heat_ref.py's; the tint and the planar store are
tests/dbvh_tiles_ref.py's.  Written from the reference's text and the header, not from the kernels.  Test infrastructure only."""
from __future__ import annotations

import functools

import numpy as np

from tests import dbvh_tiles_ref as DT
from tests import heat_ref as H
from tests import instances_materials_tree_ref as R
from tests import oracle_lib as O

F = np.float32
REFLECTIONS, AA4 = R.REFLECTIONS, R.AA4


class InstMaterialsHeatRef:
    """Counters and heat bytes of one InstTranspRef (a material set on an instanced scene); one RayTrace call per (frame, packet, lights, bounce,
    mode, depth), memoised: the tests share every call."""

    def __init__(self, tr):
        self.tr = tr
        self._memo = {}

    def packet(self, cam13, resx, resy, px, py, lights7, bounce, mode, max_depth):
        """-> (TreeStats uint64 [4] of the RayTrace call of the packet at (px, py), its truncated lanes)"""
        cam = np.ascontiguousarray(cam13, dtype=np.float32)
        lights = np.asarray(lights7 if lights7 is not None else np.zeros((0, 7)), dtype=np.float32).reshape(-1, 7)
        key = (cam.tobytes(), resx, resy, int(px), int(py), lights.tobytes(), bool(bounce), mode, max_depth)
        if key not in self._memo:
            fr = R.InstTreeFrames(self.tr, bounce=bool(bounce))
            _, st, trunc, _ = fr.render_packets(cam, resx, resy, np.array([[px, py]], dtype=np.int32), lights, mode=mode, max_depth=max_depth)
            st = np.asarray(st, dtype=np.uint64).copy()
            st.setflags(write=False)
            self._memo[key] = (st, int(trunc))
        return self._memo[key]

    def packet_stats(self, cam13, resx, resy, packet_xy, lights7=None, flags=0, mode=O.MODE_IEEE, max_depth=8):
        """-> (counters uint64 [n, 4], or [n, 4, 4] with AA4; the call's truncated lanes: every listed entry counts, a packet listed twice twice)"""
        xy = np.asarray(packet_xy, dtype=np.int32).reshape(-1, 2)
        bounce = bool(flags & REFLECTIONS)
        out, trunc = [], 0
        for px, py in xy.tolist():
            if flags & AA4:
                four = []
                for k in range(4):
                    st, t = self.packet(cam13, 2 * resx, 2 * resy, 2 * px + 16 * (k & 1), 2 * py + 16 * (k >> 1), lights7, bounce, mode, max_depth)
                    four.append(st); trunc += t
                out.append(np.stack(four))
            else:
                st, t = self.packet(cam13, resx, resy, px, py, lights7, bounce, mode, max_depth)
                out.append(st); trunc += t
        return np.stack(out).astype(np.uint64), trunc

    def heat_packets(self, cam13, resx, resy, packet_xy, lights7=None, flags=0, tint=None, mode=O.MODE_IEEE, max_depth=8):
        """-> (packet-major B,G,R bytes [n, 256, 3], counters, truncated)"""
        ps, trunc = self.packet_stats(cam13, resx, resy, packet_xy, lights7, flags, mode, max_depth)
        return heat_bytes(ps, bool(flags & AA4), tint), ps, trunc

    def heat_frame(self, cam13, resx, resy, lights7=None, flags=0, mode=O.MODE_IEEE, max_depth=8):
        """-> (frame uint8 [resy, resx, 3] (B,G,R), TreeStats uint64 [4]: the counters' sum, truncated)"""
        from tests import dbvh_shade_ref as S
        xy = np.asarray(S.frame_packets(resx, resy), dtype=np.int32).reshape(-1, 2)
        bgr, ps, trunc = self.heat_packets(cam13, resx, resy, xy, lights7, flags, None, mode, max_depth)
        return H.packets_to_frame(bgr, xy, resx, resy), ps.reshape(-1, 4).sum(axis=0), trunc

    def heat_tiles(self, cam13, resx, resy, tiles, lights7=None, flags=0, tint=None, mode=O.MODE_IEEE, max_depth=8):
        """-> ([planes R, G-R, B-R of tile k: uint8 [3 w h]], TreeStats uint64 [4], truncated)"""
        t = np.asarray(tiles, dtype=np.int32).reshape(-1, 4)
        bgr, ps, trunc = self.heat_packets(cam13, resx, resy, DT.tile_packets(t), lights7, flags, tint, mode, max_depth)
        out, k = [], 0
        for x, y, w, h in t.tolist():
            n = ((w + 15) // 16) * ((h + 15) // 16)
            out.append(DT.planar_from_packets(bgr[k:k + n], w, h, resx - x, resy - y))
            k += n
        return out, ps.reshape(-1, 4).sum(axis=0), trunc


def heat_bytes(pstats, aa=False, tint=None):
    """counters [n, 4] (aa: [n, 4, 4]) -> packet-major B,G,R bytes [n, 256, 3]: the heat colour, with aa the 2x2 reduction of four equal colours per
    8x8 quadrant (k & 1, k >> 1), then the tint c = (c + 0.1) * tint, then ConvColor"""
    if tint is None:
        return H.heat_aa_packets(pstats) if aa else H.heat_packets(pstats)
    ps = np.asarray(pstats).reshape(-1, 4, 4) if aa else np.asarray(pstats).reshape(-1, 1, 4)
    out = np.zeros((len(ps), 16, 16, 3), dtype=np.uint8)
    for i, subs in enumerate(ps):
        for k, s in enumerate(subs):
            c = H.heat_rgb(s)
            if aa:
                c = ((c + c) * F(0.25) + (c + c) * F(0.25)).astype(np.float32)
            b = H.conv_color(DT.apply_tint(c, tint))
            if aa:
                out[i, 8 * (k >> 1):8 * (k >> 1) + 8, 8 * (k & 1):8 * (k & 1) + 8] = b
            else:
                out[i] = b
    return out.reshape(len(ps), 256, 3)


@functools.lru_cache(maxsize=None)
def case_ref(name, opaque=False):
    """the InstMaterialsHeatRef of a case of tests/instances_materials_tree_cases.py (opaque: with its opaque stand-ins), shared by the tests"""
    from tests import instances_materials_tree_cases as K
    return InstMaterialsHeatRef(K.transp_ref(name, opaque))
