"""Test-side restatement of Scene<DBVH>::RayTrace in the simple-shading configuration (src/scene_trace.cpp:86-520, TraceLight :523-601,
TraceReflection :603-618) for the instanced scenes of tests/dbvh_ref.py, in float32 numpy: every operation rounded separately, in the
order the reference writes it.  The traversals are Ref.traverse; Inv / FastInv / RSqrt follow the arithmetic through dbvh_ref.inv and
oracle_lib.raw_approx, Sqrt is IEEE.  Written from the reference's text and include/snail_instances_shade.h, not from the kernels.
Conventions shared with the library (include/snail_hip.h): lanes the reference leaves uninitialised (misses) are zeros and masked.
Test infrastructure only."""
from __future__ import annotations

import numpy as np

from tests import dbvh_ref as R
from tests import oracle_lib as O

F = np.float32
INF = F(np.inf)


def fast_inv(x, mode):
    """FastInv(f32x4) (veclib/sse/f32.h:101): raw rcpps; the scalar definition is 1 / x (veclib/vecbase.h:57)"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        if mode == O.MODE_IEEE:
            return (F(1.0) / x).astype(np.float32)
    return O.raw_approx(0, np.ascontiguousarray(x).view(np.uint32).reshape(-1), mode == O.MODE_TABLE).view(np.float32).reshape(x.shape)


def dot3(a, b):
    """veclib/vec3.h:92-106: (x*x' + y*y') + z*z'; a, b [..., 3, 4] -> [..., 4]"""
    return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]).astype(np.float32)


def conv_color(col):
    """ConvColor (src/render.cpp:11-17): Trunc(Clamp(c * 255, 0, 255)) per channel, stored B, G, R.  col [..., 3] (r, g, b) -> uint8 [..., 3]"""
    with np.errstate(all="ignore"):
        v = (np.asarray(col, dtype=np.float32) * F(255.0)).astype(np.float32)
        v = np.where(v > 0, v, F(0.0))          # Max(o, lo) = o > lo ? o : lo
        v = np.where(v < F(255.0), v, F(255.0))
    return v.astype(np.int32).astype(np.uint8)[..., ::-1]


class Diag:
    """What the frame exercised (for the tests' non-vacuity conditions), counted over the PRIMARY packets unless said otherwise."""

    def __init__(self):
        self.hit_pixels = 0
        self.lit_pixels = 0                # hit lanes to which some light contributed
        self.occluded_pixels = 0           # hit lanes with a cast shadow ray (N.L > 0) that ended occluded, for some light
        self.culled = set()                # (packet, light) with hits and the light culled at packet level
        self.not_culled = set()            # (packet, light) with hits and the light traced
        self.mirrored_hits = 0             # mirrored lanes that hit something
        self.cross_instance_occluders = 0  # occluded lanes whose nearest occluder (from the light) lies in another instance than the hit


class ShadeRef:
    def __init__(self, ref: R.Ref, want_cross: bool = False):
        self.ref = ref
        self.want_cross = want_cross

    # ObjectInstance::GetNormal = TransformVec(blas.GetNormal(elem)) (src/dbvh/tree.h:21-26,178-181)
    def normals(self, obj, elem, hit):
        nrm = np.zeros((64, 3, 4), dtype=np.float32)
        if not hit.any():
            return nrm
        pl = np.zeros((64, 4, 3), dtype=np.float32)
        bi = self.ref.bi[np.where(hit, obj, 0)]
        for b in np.unique(bi[hit]):
            sel = hit & (bi == b)
            pl[sel] = self.ref.blas[b].tris["plane"][elem[sel], :3]
        rot = self.ref.xf[np.where(hit, obj, 0)][..., :9].reshape(64, 4, 3, 3)      # [q, l, row, col]
        for c in range(3):
            n = (pl[..., 0] * rot[..., c, 0] + pl[..., 1] * rot[..., c, 1]) + pl[..., 2] * rot[..., c, 2]
            nrm[:, c, :] = np.where(hit, n, F(0.0))
        return nrm

    def ray_trace(self, org, d, idir, mask, shared, depth, L, mode, stats, diag=None, pkt=None):
        """Scene::RayTrace of one packet of 64 quads -> outColor [64, 4, 3] (r, g, b).  org [1 or 64, 3, 4]; mask uint8 [64] or None."""
        lights, ambient, color, reflections = L
        ref = self.ref
        bits = np.full((64, 4), True) if mask is None else ((mask.reshape(64, 1).astype(np.int32) >> np.arange(4).reshape(1, 4)) & 1).astype(bool)
        dist = np.where(bits, INF, -INF).astype(np.float32)          # src/scene_trace.cpp:112-115
        stats[2] += int(bits.sum())                                  # stats.TracingRays(CountMaskBits(...)), :116-117
        obj = np.zeros((64, 4), dtype=np.int32); elem = np.zeros((64, 4), dtype=np.int32)
        stats += ref.traverse(org, d, idir, mask, dist, obj, elem, None, shared, False, mode)

        # samples (:366-379, 397-452; shading/simple_material.h:19-28)
        hit = (dist < INF) & bits
        o = np.repeat(org[:1], 64, axis=0) if shared else org
        with np.errstate(all="ignore"):
            pos = (d * dist.reshape(64, 1, 4) + o).astype(np.float32)
        nrm = self.normals(obj, elem, hit)
        with np.errstate(all="ignore"):
            sdn = np.where(hit, np.abs(dot3(d, nrm)), F(0.0)).astype(np.float32)
        sdiff = np.stack([F(color[c]) * sdn for c in range(3)], axis=-1).astype(np.float32)     # [64, 4, 3]
        sspec = sdiff.copy()
        if diag is not None and depth == 0:
            diag.hit_pixels += int(hit.sum())
        if diag is not None and depth == 1:
            diag.mirrored_hits += int(hit.sum())

        # reflections (:454-466, TraceReflection :603-618, Reflect src/rtbase_math.h:54-58)
        if reflections and depth < 1:
            with np.errstate(all="ignore"):
                dt = dot3(nrm, d)
                dt2 = (dt + dt).reshape(64, 1, 4)
                r = (d - nrm * dt2).astype(np.float32)
                h3 = hit.reshape(64, 1, 4)
                rd = np.where(h3, r, F(0.0)).astype(np.float32)
                ro = np.where(h3, pos + r * F(0.001), F(0.0)).astype(np.float32)
                ri = R.inv(rd + F(0.00000001), mode)
            sel = (hit.astype(np.uint8) << np.arange(4, dtype=np.uint8).reshape(1, 4)).sum(axis=1).astype(np.uint8)
            refl = self.ray_trace(np.ascontiguousarray(ro), np.ascontiguousarray(rd), np.ascontiguousarray(ri), sel, False, depth + 1, L, mode, stats, diag, pkt)
            with np.errstate(all="ignore"):
                sdiff = np.where(hit.reshape(64, 4, 1), sdiff + (refl - sdiff) * F(0.3), sdiff).astype(np.float32)

        # lights (:484-512)
        n_lights = len(lights)
        lDiff = np.empty((64, 4, 3), dtype=np.float32); lDiff[...] = np.asarray(ambient, dtype=np.float32)
        lSpec = np.zeros((64, 4, 3), dtype=np.float32)
        if hit.any():
            tmin = [pos[:, c, :][hit].min() for c in range(3)]
            tmax = [pos[:, c, :][hit].max() for c in range(3)]
        else:
            tmin, tmax = [INF] * 3, [-INF] * 3
        lit_any = np.zeros((64, 4), dtype=bool); occ_any = np.zeros((64, 4), dtype=bool)
        for n in range(n_lights):
            lp = [F(lights[n][k]) for k in range(3)]
            lc = [F(lights[n][3 + k]) for k in range(3)]
            radius = F(lights[n][6])
            with np.errstate(all="ignore"):
                i_radius, rad_sq = F(1.0) / radius, radius * radius          # src/light.h:9-13
            sq = F(0.0)                                                      # BoxPointDistanceSq (src/funcs.cpp:8-49)
            for k in range(3):
                if lp[k] < tmin[k]:
                    dl = lp[k] - tmin[k]; sq = sq + dl * dl
                elif lp[k] > tmax[k]:
                    dl = lp[k] - tmax[k]; sq = sq + dl * dl
            if sq > rad_sq:
                if diag is not None and depth == 0 and hit.any():
                    diag.culled.add((pkt, n))
                continue
            if diag is not None and depth == 0 and hit.any():
                diag.not_culled.add((pkt, n))
            # Scene::TraceLight (:523-601)
            with np.errstate(all="ignore"):
                lv = (pos - np.array(lp, dtype=np.float32).reshape(1, 3, 1)).astype(np.float32)
                close = dot3(lv, lv) < F(0.0001)
                lv = np.where(close.reshape(64, 1, 4), np.array([0.0, 1.0, 0.0], dtype=np.float32).reshape(1, 3, 1), lv).astype(np.float32)
                distance = np.sqrt(dot3(lv, lv)).astype(np.float32)
                h3 = hit.reshape(64, 1, 4)
                fl = np.where(h3, lv * R.inv(distance, mode).reshape(64, 1, 4), F(0.0)).astype(np.float32)
                sidir = np.where(h3, R.inv(fl + F(0.00000001), mode), F(0.0)).astype(np.float32)
                distance = np.where(hit, distance, F(0.0)).astype(np.float32)
                dotv = np.where(hit, dot3(nrm, fl), F(0.0)).astype(np.float32)
                cast = hit & (dotv > 0)
                sdist = np.where(cast, distance * F(0.9999), -INF).astype(np.float32)
            stats[2] += int(cast.sum())
            lorg = np.repeat(np.array(lp, dtype=np.float32).reshape(1, 3, 1), 4, axis=2)
            fl = np.ascontiguousarray(fl); sidir = np.ascontiguousarray(sidir)
            before = sdist.copy()
            stats += ref.traverse(lorg, fl, sidir, None, sdist, None, None, None, True, True, mode)
            after = sdist > 0
            if diag is not None and depth == 0:
                occluded = cast & ~after
                lit_any |= after; occ_any |= occluded
                if self.want_cross and diag.cross_instance_occluders == 0 and occluded.any():
                    oo = np.full((64, 4), -1, dtype=np.int32); oe = np.zeros((64, 4), dtype=np.int32)
                    ref.traverse(lorg, fl, sidir, None, before.copy(), oo, oe, None, True, False, mode)
                    diag.cross_instance_occluders += int((occluded & (oo >= 0) & (oo != obj)).sum())
            with np.errstate(all="ignore"):
                atten = (distance * i_radius).astype(np.float32)
                x = ((F(1.0) - atten) * F(0.2) + fast_inv(F(16.0) * atten * atten, mode)) - F(0.0625)
                atten = np.where(F(0.0) > x, F(0.0), x).astype(np.float32)          # Max(0, x)
                diff_mul = (dotv * atten).astype(np.float32)
                spec_mul = dotv.copy()
                for _ in range(4):
                    spec_mul = (spec_mul * spec_mul).astype(np.float32)
                spec_mul = (spec_mul * atten).astype(np.float32)
                for c in range(3):
                    lDiff[..., c] = np.where(after, lDiff[..., c] + lc[c] * diff_mul, lDiff[..., c])
                    lSpec[..., c] = np.where(after, lSpec[..., c] + lc[c] * spec_mul, lSpec[..., c])
        if diag is not None and depth == 0:
            diag.lit_pixels += int(lit_any.sum()); diag.occluded_pixels += int(occ_any.sum())
        with np.errstate(all="ignore"):
            return (sdiff * lDiff + sspec * lSpec).astype(np.float32) if n_lights else sdiff

    def render_packets(self, cam13, resx, resy, packet_xy, lights7, ambient=(0.1, 0.1, 0.1), color=(1.0, 1.0, 1.0), reflections=False, mode=O.MODE_IEEE,
                       diag=None):
        """-> (packet-major B,G,R bytes [n, 256, 3], TreeStats uint64[4]) of the packets at the given pixel origins"""
        cam = np.asarray(cam13, dtype=np.float32)
        lights = np.asarray(lights7 if lights7 is not None else np.zeros((0, 7)), dtype=np.float32).reshape(-1, 7)
        L = (lights, np.asarray(ambient, dtype=np.float32), np.asarray(color, dtype=np.float32), bool(reflections))
        org = np.repeat(cam[:3].reshape(1, 3, 1), 4, axis=2).astype(np.float32)
        xy = np.asarray(packet_xy, dtype=np.int32).reshape(-1, 2)
        out = np.zeros((len(xy), 256, 3), dtype=np.uint8)
        stats = np.zeros(4, dtype=np.uint64)
        for p, (px, py) in enumerate(xy.tolist()):
            dd, ii = O.gen_packet(cam, resx, resy, px, py, mode)
            col = self.ray_trace(org, dd.reshape(64, 3, 4).copy(), ii.reshape(64, 3, 4).copy(), None, True, 0, L, mode, stats, diag, p)
            out[p] = conv_color(col).reshape(256, 3)
        return out, stats

    def render(self, cam13, resx, resy, lights7, ambient=(0.1, 0.1, 0.1), color=(1.0, 1.0, 1.0), reflections=False, mode=O.MODE_IEEE, diag=None):
        """-> (frame uint8 [resy, resx, 3] (B,G,R), TreeStats uint64[4]); the packets row-major over the 16x16 grid"""
        xy = frame_packets(resx, resy)
        bgr, stats = self.render_packets(cam13, resx, resy, xy, lights7, ambient, color, reflections, mode, diag)
        return packets_to_frame(xy, bgr, resx, resy), stats


def frame_packets(resx, resy):
    return np.array([(x, y) for y in range(0, resy, 16) for x in range(0, resx, 16)], dtype=np.int32)


def packets_to_frame(xy, bgr, resx, resy):
    """quad q of a packet = row q >> 2, pixels 4 (q & 3) .. + 3 (RayGenerator::Generate level 3, src/ray_generator.cpp:23-47)"""
    frame = np.zeros((resy, resx, 3), dtype=np.uint8)
    for p, (px, py) in enumerate(np.asarray(xy).reshape(-1, 2).tolist()):
        tile = bgr[p].reshape(16, 16, 3)
        h, w = min(16, resy - py), min(16, resx - px)
        if h > 0 and w > 0:
            frame[py:py + h, px:px + w] = tile[:h, :w]
    return frame
