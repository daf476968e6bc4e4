"""Test-side restatement of Scene<BVH>::RayTrace with full shading (gVals[6] && HasShadingData(), src/scene_trace.cpp:145-358) for primary
packets, then the lights (:484-512, TraceLight :523-601), in float32 numpy: every operation rounded separately, in the order the reference
writes it.  Written from the reference's text (src/scene_trace.cpp, src/shading/*.h, src/sampling/point_sampler.cpp:126-210,
src/mipmap_texture.cpp:256-285, src/triangle.h:181-230) and include/snail_materials.h, not from the kernels.  The walks are the oracle's
(oracle_lib.gen_packet / trace_rays / trace_shadow); Inv / FastInv follow the arithmetic through dbvh_ref.inv and oracle_lib.raw_approx.
Conventions shared with the library: values the reference reads before it writes them are zeros, and so is everything of a lane that
missed.  Test infrastructure only."""
from __future__ import annotations

from collections import Counter

import numpy as np

from tests import dbvh_ref as R
from tests import dbvh_shade_ref as S
from tests import oracle_lib as O

F = np.float32
INF = F(np.inf)
SIMPLE, TEX, UBER, TRANSPARENT = 0, 1, 2, 3


# ---- data ----------------------------------------------------------------------------------------------------------------------------
def pack_shtris(uv, nrm, mat_index, flat, perm):
    """The ShTriangle constructor (src/triangle.h:188-208) and the builder's permutation: -> (uv [n,3,2], nrm [n,3,3] with elements 1, 2 as
    differences, matId int64 [n] incl. the flat bit) in triId order"""
    uv = np.asarray(uv, dtype=np.float32).reshape(-1, 3, 2)[perm].copy()
    nr = np.asarray(nrm, dtype=np.float32).reshape(-1, 3, 3)[perm].copy()
    uv[:, 1] -= uv[:, 0]; uv[:, 2] -= uv[:, 0]
    nr[:, 1] -= nr[:, 0]; nr[:, 2] -= nr[:, 0]
    mid = np.asarray(mat_index, dtype=np.int64)[perm] | (np.asarray(flat).astype(bool)[perm].astype(np.int64) << 31)
    return uv, nr, mid


def shtris_bytes(uv, nr, mid):
    """the 64-byte records of the three arrays above"""
    n = len(uv)
    rec = np.zeros((n, 16), dtype=np.uint32)
    rec[:, 0:6] = uv.reshape(n, 6).view(np.uint32)
    rec[:, 6:15] = nr.reshape(n, 9).view(np.uint32)
    rec[:, 15] = mid.astype(np.uint32)
    return rec.view(np.uint8).reshape(n, 64)


def level_shapes(w, h):
    """MipmapTexture::Set (src/mipmap_texture.cpp:103-126): min(32, Log2(max(w, h)) + 1) levels of max(w >> m, 1) x max(h >> m, 1)"""
    n = min(32, max(w, h).bit_length())
    return [(max(w >> m, 1), max(h >> m, 1)) for m in range(n)]


def gen_mips(level0):
    """MipmapTexture::GenMips for rgb8 (src/mipmap_texture.cpp:256-285), literally, in ONE buffer with tight pitches: uint8 [h, w, 3] -> the
    whole chain (uint8, flat)"""
    a = np.ascontiguousarray(level0, dtype=np.uint8)
    h, w = a.shape[:2]
    shapes = level_shapes(w, h)
    offs = [0]
    for lw, lh in shapes:
        offs.append(offs[-1] + 3 * lw * lh)
    buf = [0] * (offs[-1] + 8)
    buf[:3 * w * h] = a.reshape(-1).tolist()
    for mip in range(1, len(shapes)):
        (srcW, srcH), (dstW, dstH) = shapes[mip - 1], shapes[mip]
        srcPitch, dstPitch = 3 * srcW, 3 * dstW
        src, dst = offs[mip - 1], offs[mip]
        if srcH == dstH:
            for x in range(dstW):
                for i in range(3):
                    buf[dst + i] = (buf[src + i] + buf[src + 4 + i]) // 2
                dst += 3; src += 6
        elif srcW == dstW:
            for y in range(dstH):
                for i in range(3):
                    buf[dst + i] = (buf[src + i] + buf[src + i + srcPitch]) // 2
                src += srcPitch * 2; dst += dstPitch
        else:
            for y in range(dstH):
                s, d = src + y * 2 * srcPitch, dst + y * dstPitch
                for x in range(dstW):
                    for i in range(3):
                        buf[d + i] = (buf[s + i] + buf[s + 3 + i] + buf[s + i + srcPitch] + buf[s + i + 3 + srcPitch]) // 4
                    d += 3; s += 6
    return np.array(buf[:offs[-1]], dtype=np.uint8)


class RefTexture:
    def __init__(self, level0):
        a = np.ascontiguousarray(level0, dtype=np.uint8)
        self.h, self.w = a.shape[:2]
        self.shapes = level_shapes(self.w, self.h)
        self.levels = gen_mips(a)
        self.data = np.concatenate([self.levels, np.zeros(4, dtype=np.uint8)]).astype(np.int64)
        off = [0]
        for lw, lh in self.shapes:
            off.append(off[-1] + 3 * lw * lh)
        self.off = np.array(off[:-1], dtype=np.int64)
        self.pitch = np.array([3 * lw for lw, _ in self.shapes], dtype=np.int64)

    def sample(self, cu, cv, tdx, tdy):
        """PointSampler::Sample (src/sampling/point_sampler.cpp:126-210) for arrays of rays -> (rgb [..., 3] = temp1, the mips chosen)"""
        w, h = self.w, self.h
        wmul, hmul = F(w - 1), F(h - 1)
        cu = np.asarray(cu, dtype=np.float32); cv = np.asarray(cv, dtype=np.float32)
        with np.errstate(all="ignore"):
            ux = (cu - np.trunc(cu).astype(np.float32)).astype(np.float32)          # ClampTexCoord
            uy = (cv - np.trunc(cv).astype(np.float32)).astype(np.float32)
            ux = np.where(ux < 0, ux + F(1.0), ux).astype(np.float32)
            uy = np.where(uy < 0, uy + F(1.0), uy).astype(np.float32)
            px = (ux * wmul).astype(np.float32); py = (uy * hmul).astype(np.float32)
            ax = (np.asarray(tdx, dtype=np.float32) * wmul).astype(np.float32); ay = (np.asarray(tdy, dtype=np.float32) * hmul).astype(np.float32)
            mn = np.where(ax < ay, ax, ay).astype(np.float32)                        # minps
            pixels = (mn * F(0.6)).astype(np.float32).astype(np.int64) & 0xffffffff  # uint(float)
        mip = np.zeros(pixels.shape, dtype=np.int64)
        p = pixels.copy()
        while (p > 0).any():
            mip += (p > 0)
            p >>= 1
        mip = np.minimum(mip, len(self.shapes) - 1)
        x1 = px.astype(np.int64); y1 = py.astype(np.int64)
        x2 = x1 + 1; y2 = y1 + 1
        dx = (px - x1.astype(np.float32)).astype(np.float32); dy = (py - y1.astype(np.float32)).astype(np.float32)
        y1 = h - y1; y2 = h - y2
        x1 >>= mip; y1 >>= mip; x2 >>= mip; y2 >>= mip
        xm = (w - 1) >> mip; ym = (h - 1) >> mip
        x1 &= xm; y1 &= ym; x2 &= xm; y2 &= ym
        x1 = x1 * 3; x2 = x2 * 3
        pitch = self.pitch[mip]
        y1 = y1 * pitch; y2 = y2 * pitch
        base = self.off[mip]
        o = [base + x1 + y1, base + x2 + y1, base + x1 + y2, base + x2 + y2]
        out = np.zeros(cu.shape + (3,), dtype=np.float32)
        for c in range(3):
            t = [self.data[o[k] + c].astype(np.float32) for k in range(4)]
            top = (t[0] + (t[1] - t[0]) * dx).astype(np.float32)                      # Lerp(a, b, x) = a + (b - a) * x
            bot = (t[2] + (t[3] - t[2]) * dx).astype(np.float32)
            out[..., c] = ((top + (bot - top) * dy).astype(np.float32) * (F(1.0) / F(255.0))).astype(np.float32)
        return out, mip


class RefMaterial:
    def __init__(self, kind, ndotr=True, diffuse=(1, 1, 1), specular=(0, 0, 0), dissolve=0.0, texture=0):
        self.kind, self.ndotr, self.texture, self.dissolve = kind, bool(ndotr), texture, dissolve
        self.diffuse = np.asarray(diffuse, dtype=np.float32).copy()
        self.specular = np.asarray(specular, dtype=np.float32).copy()
        if kind == UBER:                       # UberMaterial::UberMaterial: Swap(diffuse.x, diffuse.z)
            self.diffuse[0], self.diffuse[2] = self.diffuse[2], self.diffuse[0]


DEFAULT_MAT = RefMaterial(SIMPLE, True, (1.0, 1.0, 1.0))          # Scene::defaultMat, src/scene.cpp:6


class Diag:
    """What the frame exercised (for the tests' non-vacuity conditions)."""

    def __init__(self):
        self.blocks_a = 0                  # single-triangle blocks (:178-225)
        self.blocks_b = 0                  # per-quad blocks that end in the unmasked Shade of ONE material (:301-308)
        self.blocks_c = 0                  # per-quad blocks with SEVERAL materials among their selected lanes (:310-355)
        self.blocks_masked_one = 0         # per-quad blocks with misses and one material (the masked path as well; counted apart)
        self.mips = Counter()              # (texture, mip level) -> textured lanes that chose it
        self.quirk_lanes = 0               # lane 0 missed, lane k hit triId 0: default material, zero normal
        self.default_meets_others = 0      # blocks of (c) in which the default material stands beside others
        self.uber_unmasked = 0             # UBER lanes: specular = diffuse
        self.uber_masked = 0               # UBER lanes: specular = spec
        self.normals_right = 0             # blocks with nrm0 + (nrm1 bx + nrm2 by)  (:204)
        self.normals_left_a = 0            # blocks of (a) with (nrm0 + nrm1 bx) + nrm2 by  (:220)
        self.normals_flat = 0
        self.hit_pixels = 0
        self.lit_pixels = 0
        self.occluded_pixels = 0
        self.culled = set()                # (packet, light)
        self.not_culled = set()


def lerp_left(a, b, c, x, y):
    return ((a + b * x).astype(np.float32) + (c * y).astype(np.float32)).astype(np.float32)


def lerp_right(a, b, c, x, y):
    return (a + ((b * x).astype(np.float32) + (c * y).astype(np.float32)).astype(np.float32)).astype(np.float32)


class MaterialsRef:
    def __init__(self, osc, uv, nrm, mat_index, flat, material_map, materials, textures):
        """osc: oracle_lib.OracleScene (its perm permutes the INPUT triangles' shading data); materials: RefMaterial list; textures: RefTexture list"""
        self.osc = osc
        self.uv, self.nr, self.mid = pack_shtris(uv, nrm, mat_index, flat, osc.perm)
        self.map = np.asarray(material_map, dtype=np.int64)
        self.materials, self.textures = list(materials), list(textures)

    def mat(self, m):
        return DEFAULT_MAT if m == -1 else self.materials[m]

    def mat_id(self, tri):
        return int(self.map[int(self.mid[tri]) & 0x7fffffff])          # BVH::GetMaterialId, src/bvh/tree.h:82-84

    # mat->Shade(samples + b4, RayGroup(..)) for one block: d, nrm [4,3,4]; tc [4,2,4]; tdiff [4,2]; mask bool [4,4] or None (unmasked)
    def shade(self, m, d, nrm, tc, tdiff, mask, diffuse, specular, diag):
        mt = self.mat(m)
        with np.errstate(all="ignore"):
            dn = S.dot3(d, nrm)                                          # rays.Dir(q) | s.normal
            if mt.kind == TEX:
                t1, mips = self.textures[mt.texture].sample(tc[:, 0], tc[:, 1], np.repeat(tdiff[:, 0:1], 4, axis=1), np.repeat(tdiff[:, 1:2], 4, axis=1))
                dif = [(t1[..., c] * dn).astype(np.float32) if mt.ndotr else t1[..., c] for c in range(3)]
                spc = dif
                sel = np.full((4, 4), True) if mask is None else mask
                for v in mips[sel].tolist():
                    diag.mips[(mt.texture, v)] += 1
            elif mt.kind == UBER:
                dif = [(mt.diffuse[c] * np.abs(dn)).astype(np.float32) for c in range(3)]
                spc = dif if mask is None else [np.full((4, 4), mt.specular[c], dtype=np.float32) for c in range(3)]
                n = 16 if mask is None else int(mask.sum())
                if mask is None:
                    diag.uber_unmasked += n
                else:
                    diag.uber_masked += n
            else:
                dif = [(mt.diffuse[c] * np.abs(dn)).astype(np.float32) if mt.ndotr else np.full((4, 4), mt.diffuse[c], dtype=np.float32) for c in range(3)]
                spc = dif
        for c in range(3):
            if mask is None:
                diffuse[:, c, :] = dif[c]; specular[:, c, :] = spc[c]
            else:
                diffuse[:, c, :] = np.where(mask, dif[c], diffuse[:, c, :]); specular[:, c, :] = np.where(mask, spc[c], specular[:, c, :])

    def samples(self, d, dist, obj, bary, diag):
        """:145-358 for one packet: d [64,3,4], dist / obj [64,4], bary [64,8] -> (hit, nrm, diffuse, specular), the last three [64,3,4]"""
        hit = dist < INF
        objc = np.where(hit, obj, 0)
        bx, by = bary[:, 0:4], bary[:, 4:8]
        nrm = np.zeros((64, 3, 4), dtype=np.float32); tc = np.zeros((64, 2, 4), dtype=np.float32); tdiff = np.zeros((64, 2), dtype=np.float32)
        diffuse = np.zeros((64, 3, 4), dtype=np.float32); specular = np.zeros((64, 3, 4), dtype=np.float32)
        mid = np.full((64, 4), -1, dtype=np.int64)
        uvT, nrT = self.uv, self.nr
        with np.errstate(all="ignore"):
            for b in range(16):
                qs = slice(4 * b, 4 * b + 4)
                if not hit[qs].any():
                    continue
                full = bool(hit[qs].all())
                obj0 = int(objc[4 * b, 0])
                if full and bool((objc[qs] == obj0).all()):
                    # (a) 4x4 full, single triangle
                    diag.blocks_a += 1
                    m = self.mat_id(obj0)
                    flat = bool(int(self.mid[obj0]) >> 31)
                    mt = self.mat(m)
                    if mt.kind != TEX:
                        if flat:
                            diag.normals_flat += 1
                            for c in range(3):
                                nrm[qs, c, :] = nrT[obj0, 0, c]
                        else:
                            diag.normals_right += 1
                            for c in range(3):
                                nrm[qs, c, :] = lerp_right(nrT[obj0, 0, c], nrT[obj0, 1, c], nrT[obj0, 2, c], bx[qs], by[qs])
                    else:
                        diag.normals_left_a += 1
                        for c in range(2):
                            tc[qs, c, :] = lerp_left(uvT[obj0, 0, c], uvT[obj0, 1, c], uvT[obj0, 2, c], bx[qs], by[qs])
                        tdiff[qs] = tc[qs].max(axis=2) - tc[qs].min(axis=2)
                        for c in range(3):
                            nrm[qs, c, :] = lerp_left(nrT[obj0, 0, c], nrT[obj0, 1, c], nrT[obj0, 2, c], bx[qs], by[qs])
                    mid[qs] = m
                    self.shade(m, d[qs], nrm[qs], tc[qs], tdiff[qs], None, diffuse[qs], specular[qs], diag)
                    continue
                # (b) per quad
                for q in range(4 * b, 4 * b + 4):
                    if not hit[q].any():
                        continue
                    o0 = int(objc[q, 0])
                    if hit[q, 0]:
                        m = self.mat_id(o0)
                        mid[q] = np.where(hit[q], m, mid[q])
                        for c in range(2):
                            tc[q, c, :] = lerp_left(uvT[o0, 0, c], uvT[o0, 1, c], uvT[o0, 2, c], bx[q], by[q])
                        for c in range(3):
                            nrm[q, c, :] = lerp_left(nrT[o0, 0, c], nrT[o0, 1, c], nrT[o0, 2, c], bx[q], by[q])
                    for k in range(1, 4):
                        o = int(objc[q, k])
                        if not hit[q, k]:
                            continue
                        if o == o0:
                            if not hit[q, 0]:
                                diag.quirk_lanes += 1
                            continue
                        mid[q, k] = self.mat_id(o)
                        for c in range(2):
                            tc[q, c, k] = lerp_left(uvT[o, 0, c], uvT[o, 1, c], uvT[o, 2, c], bx[q, k], by[q, k])
                        for c in range(3):
                            nrm[q, c, k] = lerp_left(nrT[o, 0, c], nrT[o, 1, c], nrT[o, 2, c], bx[q, k], by[q, k])
                tdiff[qs] = F(0.0)
                m0 = int(mid[4 * b, 0])
                if full and bool((mid[qs] == m0).all()):
                    diag.blocks_b += 1
                    self.shade(m0, d[qs], nrm[qs], tc[qs], tdiff[qs], None, diffuse[qs], specular[qs], diag)
                else:
                    # (c): one masked Shade per material id among the selected lanes (the default's last).  A lane has ONE id, so the masks are
                    # disjoint and the order cannot show.
                    ids = []
                    for v in mid[qs][hit[qs]].tolist():
                        if v not in ids:
                            ids.append(v)
                    if len(ids) > 1:
                        diag.blocks_c += 1
                        if -1 in ids:
                            diag.default_meets_others += 1
                    else:
                        diag.blocks_masked_one += 1
                    for m in [v for v in ids if v != -1] + ([-1] if -1 in ids else []):
                        self.shade(m, d[qs], nrm[qs], tc[qs], tdiff[qs], (mid[qs] == m) & hit[qs], diffuse[qs], specular[qs], diag)
        h3 = hit.reshape(64, 1, 4)
        nrm = np.where(h3, nrm, F(0.0)).astype(np.float32)
        return hit, nrm, np.where(h3, diffuse, F(0.0)).astype(np.float32), np.where(h3, specular, F(0.0)).astype(np.float32)

    def ray_trace(self, cam, resx, resy, px, py, L, mode, stats, diag, pkt):
        """Scene::RayTrace of one primary packet -> (outColor [64,4,3], samples [9,64,4])"""
        lights, ambient = L
        osc = self.osc
        dd, ii = O.gen_packet(cam, resx, resy, px, py, mode)
        d = dd.reshape(64, 3, 4).copy()
        org = np.repeat(cam[:3].reshape(1, 3, 1), 4, axis=2).astype(np.float32)
        dist = np.full((64, 4), np.inf, dtype=np.float32); obj = np.zeros((64, 4), dtype=np.int32); bary = np.zeros((64, 8), dtype=np.float32)
        stats[2] += 256
        stats += osc.trace_rays(np.ascontiguousarray(org.reshape(12)), dd, ii, None, dist, obj, bary, 1, 64, True, mode)
        hit, nrm, sdiff, sspec = self.samples(d, dist, obj, bary, diag)
        diag.hit_pixels += int(hit.sum())
        with np.errstate(all="ignore"):
            pos = (d * dist.reshape(64, 1, 4) + org).astype(np.float32)
        smp = np.concatenate([nrm.transpose(1, 0, 2), sdiff.transpose(1, 0, 2), sspec.transpose(1, 0, 2)], axis=0)
        sdiff = sdiff.transpose(0, 2, 1); sspec = sspec.transpose(0, 2, 1)           # [64, 4, 3]

        # lights (:484-512), as tests/dbvh_shade_ref.py with the plain scene's shadow walk
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
                i_radius, rad_sq = F(1.0) / radius, radius * radius
            sq = F(0.0)                                                      # BoxPointDistanceSq (src/funcs.cpp:8-49)
            for k in range(3):
                if lp[k] < tmin[k]:
                    dl = lp[k] - tmin[k]; sq = sq + dl * dl
                elif lp[k] > tmax[k]:
                    dl = lp[k] - tmax[k]; sq = sq + dl * dl
            if sq > rad_sq:
                if hit.any():
                    diag.culled.add((pkt, n))
                continue
            if hit.any():
                diag.not_culled.add((pkt, n))
            with np.errstate(all="ignore"):                                  # Scene::TraceLight (:523-601)
                lv = (pos - np.array(lp, dtype=np.float32).reshape(1, 3, 1)).astype(np.float32)
                close = S.dot3(lv, lv) < F(0.0001)
                lv = np.where(close.reshape(64, 1, 4), np.array([0.0, 1.0, 0.0], dtype=np.float32).reshape(1, 3, 1), lv).astype(np.float32)
                distance = np.sqrt(S.dot3(lv, lv)).astype(np.float32)
                h3 = hit.reshape(64, 1, 4)
                fl = np.where(h3, lv * R.inv(distance, mode).reshape(64, 1, 4), F(0.0)).astype(np.float32)
                sidir = np.where(h3, R.inv(fl + F(0.00000001), mode), F(0.0)).astype(np.float32)
                distance = np.where(hit, distance, F(0.0)).astype(np.float32)
                dotv = np.where(hit, S.dot3(nrm, fl), F(0.0)).astype(np.float32)
                cast = hit & (dotv > 0)
                sdist = np.where(cast, distance * F(0.9999), -INF).astype(np.float32)
            stats[2] += int(cast.sum())
            stats += osc.trace_shadow(np.array(lp, dtype=np.float32), np.ascontiguousarray(fl.reshape(-1)), np.ascontiguousarray(sidir.reshape(-1)), sdist, 1, 64, mode)
            after = sdist > 0
            lit_any |= after; occ_any |= cast & ~after
            with np.errstate(all="ignore"):
                atten = (distance * i_radius).astype(np.float32)
                x = ((F(1.0) - atten) * F(0.2) + S.fast_inv(F(16.0) * atten * atten, mode)) - F(0.0625)
                atten = np.where(F(0.0) > x, F(0.0), x).astype(np.float32)
                diff_mul = (dotv * atten).astype(np.float32)
                spec_mul = dotv.copy()
                for _ in range(4):
                    spec_mul = (spec_mul * spec_mul).astype(np.float32)
                spec_mul = (spec_mul * atten).astype(np.float32)
                for c in range(3):
                    lDiff[..., c] = np.where(after, lDiff[..., c] + lc[c] * diff_mul, lDiff[..., c])
                    lSpec[..., c] = np.where(after, lSpec[..., c] + lc[c] * spec_mul, lSpec[..., c])
        diag.lit_pixels += int(lit_any.sum()); diag.occluded_pixels += int(occ_any.sum())
        with np.errstate(all="ignore"):
            col = (sdiff * lDiff + sspec * lSpec).astype(np.float32) if n_lights else sdiff
        return col, smp

    def render_packets(self, cam13, resx, resy, packet_xy, lights7=None, ambient=(0.1, 0.1, 0.1), mode=O.MODE_IEEE, diag=None):
        """-> (packet-major B,G,R bytes [n,256,3], TreeStats uint64[4], samples float32 [n,9,64,4])"""
        cam = np.asarray(cam13, dtype=np.float32)
        lights = np.asarray(lights7 if lights7 is not None else np.zeros((0, 7)), dtype=np.float32).reshape(-1, 7)
        L = (lights, np.asarray(ambient, dtype=np.float32))
        diag = diag if diag is not None else Diag()
        xy = np.asarray(packet_xy, dtype=np.int32).reshape(-1, 2)
        out = np.zeros((len(xy), 256, 3), dtype=np.uint8)
        smp = np.zeros((len(xy), 9, 64, 4), dtype=np.float32)
        stats = np.zeros(4, dtype=np.uint64)
        for p, (px, py) in enumerate(xy.tolist()):
            col, smp[p] = self.ray_trace(cam, resx, resy, px, py, L, mode, stats, diag, p)
            out[p] = S.conv_color(col).reshape(256, 3)
        return out, stats, smp

    def render(self, cam13, resx, resy, lights7=None, ambient=(0.1, 0.1, 0.1), mode=O.MODE_IEEE, diag=None):
        """-> (frame uint8 [resy,resx,3] (B,G,R), TreeStats, samples, packet list)"""
        xy = S.frame_packets(resx, resy)
        bgr, stats, smp = self.render_packets(cam13, resx, resy, xy, lights7, ambient, mode, diag)
        return S.packets_to_frame(xy, bgr, resx, resy), stats, smp, xy
