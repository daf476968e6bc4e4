"""Test-side restatement of RenderTask::Work (src/render.cpp:47-211) for the instanced scenes of tests/dbvh_ref.py, on top of
tests/dbvh_shade_ref.py's Scene<DBVH>::RayTrace: per 16x16 packet the float colours (or, with gVals[1], the depth shading of
src/scene_trace.cpp:128-137), with gVals[9] the 2x2 reduction of the four double-resolution packets (:71-110) in the reference's operation
order, with gVals[8] the rank tint (:118-132), then ConvColor and the interleaved (:171-198) or planar (:140-169) store.  float32 numpy,
every operation rounded separately.  Written from the reference's text and include/snail_instances_tiles.h, not from the kernels.
Test infrastructure only."""
from __future__ import annotations

import numpy as np

from tests import dbvh_ref as R
from tests import dbvh_shade_ref as S
from tests import oracle_lib as O

F = np.float32
REFLECTIONS, DEPTH, AA4 = 1, 2, 4          # SNAIL_RENDER_* (include/snail_hip.h)

# Vec3f ncolors[] of src/render.cpp:119-128 (entry 15's green is 1.7 there)
NCOLORS = np.array([(0.6, 0.6, 0.6), (0.6, 0.6, 1.0), (0.6, 1.0, 0.6), (0.6, 1.0, 1.0), (1.0, 0.6, 0.6), (1.0, 0.6, 1.0), (1.0, 1.0, 0.6), (1.0, 1.0, 1.0),
                    (0.3, 0.3, 0.3), (0.3, 0.3, 1.0), (0.3, 0.7, 0.3), (0.3, 0.7, 0.7), (0.7, 0.3, 0.3), (0.7, 0.3, 0.7), (0.7, 0.7, 0.3), (0.7, 1.7, 0.7)],
                   dtype=np.float32)


def rank_tint(rank: int) -> np.ndarray:
    return NCOLORS[rank % len(NCOLORS)].copy()


def aa_reduce(sub):
    """src/render.cpp:72-109.  sub = the four double-resolution packets' colours [4][64, 4, 3] (quad, lane, channel), k at offsets
    (0, 0), (16, 0), (0, 16), (16, 16) -> the packet's colours [64, 4, 3]"""
    out = np.zeros((64, 4, 3), dtype=np.float32)
    coff = (0, 2, 32, 34)
    line = 4
    with np.errstate(all="ignore"):
        for k in range(4):
            tc = np.asarray(sub[k], dtype=np.float32)
            dst = coff[k]
            for tq in range(0, 64, line * 2):
                for t in range(0, line, 2):
                    q = tq + t
                    for i in range(2):
                        col = ((tc[q + i] + tc[q + i + line]) * F(0.25)).astype(np.float32)      # [lane, channel]
                        out[dst, i * 2 + 0] = col[0] + col[1]
                        out[dst, i * 2 + 1] = col[2] + col[3]
                    dst += 1
                dst += line // 2
    return out


def apply_tint(col, tint):
    """colors[q] = (colors[q] + Vec3q(0.1, 0.1, 0.1)) * color (src/render.cpp:130-131): an add and a multiply, each rounded"""
    with np.errstate(all="ignore"):
        c = (np.asarray(col, dtype=np.float32) + F(0.1)).astype(np.float32)
        return (c * np.asarray(tint, dtype=np.float32)).astype(np.float32)


def planar_from_packets(bgr, w, h, vis_w=None, vis_h=None):
    """src/render.cpp:146-168 for a w x h tile whose packets (B,G,R bytes [n, 256, 3], RenderTask::Work order) are traced whole: the
    planes R, G-R, B-R (mod 256) of the pixels inside the rect.  vis_w x vis_h = the part of the tile inside the image: the rest stays zero
    (include/snail_instances_tiles.h; the reference's tiles never leave the image, src/server.cpp:227-231)"""
    planes = np.zeros((3, h, w), dtype=np.uint8)
    vis_w = w if vis_w is None else max(0, min(w, vis_w)); vis_h = h if vis_h is None else max(0, min(h, vis_h))
    k = 0
    for y in range(0, h, 16):
        for x in range(0, w, 16):
            t = bgr[k].reshape(16, 16, 3)
            k += 1
            hh, ww = max(0, min(16, vis_h - y)), max(0, min(16, vis_w - x))
            r = t[:hh, :ww, 2]
            planes[0, y:y + hh, x:x + ww] = r
            planes[1, y:y + hh, x:x + ww] = t[:hh, :ww, 1] - r
            planes[2, y:y + hh, x:x + ww] = t[:hh, :ww, 0] - r
    assert k == len(bgr)
    return planes.reshape(-1)


def tile_packets(tiles):
    out = []
    for x, y, w, h in np.asarray(tiles).reshape(-1, 4).tolist():
        out += [(px, py) for py in range(y, y + h, 16) for px in range(x, x + w, 16)]
    return np.array(out, dtype=np.int32).reshape(-1, 2)


class TilesRef:
    def __init__(self, ref: R.Ref):
        self.ref = ref
        self.shade = S.ShadeRef(ref)
        self._memo = {}

    def _packet(self, cam, resx, resy, px, py, L, depth, mode, stats, diag, pkt):
        """Scene::RayTrace of the packet at (px, py) of a resx x resy frame -> colours [64, 4, 3]"""
        org = np.repeat(cam[:3].reshape(1, 3, 1), 4, axis=2).astype(np.float32)
        dd, ii = O.gen_packet(cam, resx, resy, px, py, mode)
        d = dd.reshape(64, 3, 4).copy(); idir = ii.reshape(64, 3, 4).copy()
        if not depth:
            return self.shade.ray_trace(org, d, idir, None, True, 0, L, mode, stats, diag, pkt)
        # gVals[1] (src/scene_trace.cpp:112-137): the primary walk, then Condition(t > inf, 0, Inv(t)) * (20, 250, 2) (the condition is never true)
        dist = np.full((64, 4), np.inf, dtype=np.float32)
        obj = np.zeros((64, 4), dtype=np.int32); elem = np.zeros((64, 4), dtype=np.int32)
        stats[2] += 256
        stats += self.ref.traverse(org, d, idir, None, dist, obj, elem, None, True, False, mode)
        if diag is not None:
            diag.hit_pixels += int((dist < np.inf).sum())
        with np.errstate(all="ignore"):
            iv = R.inv(dist, mode)
            return np.stack([iv * F(20.0), iv * F(250.0), iv * F(2.0)], axis=-1).astype(np.float32)

    def colors(self, cam13, resx, resy, packet_xy, lights7=None, flags=0, ambient=(0.1, 0.1, 0.1), color=(1.0, 1.0, 1.0), mode=O.MODE_IEEE, diag=None):
        """-> (float colours [n, 64, 4, 3] before tint and ConvColor, TreeStats).  Memoised per (frame, packet list, lights, flags, mode) when
        no Diag is asked for: the tinted and untinted bytes of a test come from one run."""
        cam = np.ascontiguousarray(cam13, dtype=np.float32)
        lights = np.asarray(lights7 if lights7 is not None else np.zeros((0, 7)), dtype=np.float32).reshape(-1, 7)
        xy = np.asarray(packet_xy, dtype=np.int32).reshape(-1, 2)
        key = (cam.tobytes(), resx, resy, xy.tobytes(), lights.tobytes(), flags, tuple(ambient), tuple(color), mode)
        if diag is None and key in self._memo:
            c, st = self._memo[key]
            return c.copy(), st.copy()
        depth = bool(flags & DEPTH)
        L = (lights, np.asarray(ambient, dtype=np.float32), np.asarray(color, dtype=np.float32), bool(flags & REFLECTIONS))
        out = np.zeros((len(xy), 64, 4, 3), dtype=np.float32)
        stats = np.zeros(4, dtype=np.uint64)
        for p, (px, py) in enumerate(xy.tolist()):
            if flags & AA4:
                offx, offy = (0, 16, 0, 16), (0, 0, 16, 16)
                sub = [self._packet(cam, resx * 2, resy * 2, px * 2 + offx[k], py * 2 + offy[k], L, depth, mode, stats, diag, 4 * p + k) for k in range(4)]
                out[p] = aa_reduce(sub)
            else:
                out[p] = self._packet(cam, resx, resy, px, py, L, depth, mode, stats, diag, p)
        self._memo[key] = (out.copy(), stats.copy())
        return out, stats

    def packets(self, cam13, resx, resy, packet_xy, lights7=None, flags=0, tint=None, **kw):
        """-> (packet-major B,G,R bytes [n, 256, 3], TreeStats)"""
        col, stats = self.colors(cam13, resx, resy, packet_xy, lights7, flags, **kw)
        if tint is not None:
            col = apply_tint(col, tint)
        return S.conv_color(col).reshape(len(col), 256, 3), stats

    def frame(self, cam13, resx, resy, lights7=None, flags=0, tint=None, **kw):
        """the image form: (frame uint8 [resy, resx, 3] (B,G,R), TreeStats)"""
        xy = S.frame_packets(resx, resy)
        bgr, stats = self.packets(cam13, resx, resy, xy, lights7, flags, tint, **kw)
        return S.packets_to_frame(xy, bgr, resx, resy), stats

    def tiles(self, cam13, resx, resy, tiles, lights7=None, flags=0, tint=None, **kw):
        """the tile list: ([planes R, G-R, B-R of tile k: uint8 [3 w h]], TreeStats)"""
        t = np.asarray(tiles, dtype=np.int32).reshape(-1, 4)
        bgr, stats = self.packets(cam13, resx, resy, tile_packets(t), lights7, flags, tint, **kw)
        out, k = [], 0
        for x, y, w, h in t.tolist():
            n = ((w + 15) // 16) * ((h + 15) // 16)
            out.append(planar_from_packets(bgr[k:k + n], w, h, resx - x, resy - y))
            k += n
        return out, stats
