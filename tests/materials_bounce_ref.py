"""Test-side restatement of the one mirrored bounce of gVals[7] under full shading: Scene<BVH>::RayTrace's call of Scene::TraceReflection
(src/scene_trace.cpp:454-466, :603-618) and the nested RayTrace<0, hasMask> of the mirrored packets with the full-shading branch (:145-358),
in float32 numpy, every operation rounded separately in the order the reference writes it.  Written from the reference's text and
include/snail_materials_bounce.h, not from the kernels.  It builds on tests/materials_ref.py by composition: the primary samples, Shade,
the textures and the data are MaterialsRef's; the nested sample stage is restated here, because the primary one hard-codes the unmasked
Shade in branch (a) and takes dist < inf for the hit mask, and a masked lane of a generic packet carries -inf.  The walks are the oracle's
(OracleScene.trace_rays / trace_shadow).  Test infrastructure only."""
from __future__ import annotations

import numpy as np

from tests import dbvh_ref as R
from tests import dbvh_shade_ref as S
from tests import materials_ref as M
from tests import oracle_lib as O

F = np.float32
INF = F(np.inf)


class BounceDiag:
    """What a frame exercised: `primary` and `nested` are materials_ref.Diag objects of the primary packets and of the nested calls (one
    nested call per primary packet); the rest is counted per nested call."""

    def __init__(self):
        self.primary = M.Diag()
        self.nested = M.Diag()
        self.packets_masked = 0            # nested packets shaded as RayGroup<0, 1> (some lane not selected, some selected)
        self.packets_unmasked = 0          # nested packets shaded as RayGroup<0, 0> (all 256 lanes selected)
        self.packets_empty = 0             # nested packets without a selected lane
        self.a_masked = 0                  # single-triangle blocks in masked / unmasked nested packets
        self.a_unmasked = 0
        self.a_uber_masked = 0             # ... whose material is UBER: specular = `specular` / = the sample's diffuse
        self.a_uber_unmasked = 0
        self.a_tex_masked = 0              # ... whose material is TEX, in masked packets
        self.a_tex_mip_above_0 = 0         # single-triangle nested blocks with a TEX material in which a lane chose a mip above 0
        self.mirrored_lanes = 0            # selected lanes of the mirrored packets
        self.mirrored_hits = 0
        self.mirrored_misses = 0           # selected lanes whose mirrored ray hit nothing


def light_loop(osc, pos, hit, nrm, L, mode, stats, diag, pkt):
    """:484-502 and Scene::TraceLight (:523-601) on one packet's samples: pos, nrm [64,3,4], hit [64,4] -> (lDiffuse, lSpecular) [64,4,3]"""
    lights, ambient = L
    lDiff = np.empty((64, 4, 3), dtype=np.float32); lDiff[...] = np.asarray(ambient, dtype=np.float32)
    lSpec = np.zeros((64, 4, 3), dtype=np.float32)
    if hit.any():
        tmin = [pos[:, c, :][hit].min() for c in range(3)]
        tmax = [pos[:, c, :][hit].max() for c in range(3)]
    else:
        tmin, tmax = [INF] * 3, [-INF] * 3
    lit_any = np.zeros((64, 4), dtype=bool); occ_any = np.zeros((64, 4), dtype=bool)
    for n in range(len(lights)):
        lp = [F(lights[n][k]) for k in range(3)]
        lc = [F(lights[n][3 + k]) for k in range(3)]
        radius = F(lights[n][6])
        with np.errstate(all="ignore"):
            i_radius, rad_sq = F(1.0) / radius, radius * radius
        sq = F(0.0)                                                      # BoxPointDistanceSq (src/funcs.cpp:8-49)
        with np.errstate(all="ignore"):
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
        with np.errstate(all="ignore"):
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
    return lDiff, lSpec


class BounceRef:
    def __init__(self, ref: M.MaterialsRef):
        self.ref = ref
        self.osc = ref.osc

    def samples_rays(self, d, dist, obj, bary, bits, diag: BounceDiag):
        """:145-358 for one generic packet, RayGroup<0, hasMask> with hasMask = not all 256 lanes selected: d [64,3,4], dist / obj [64,4],
        bary [64,8], bits bool [64,4] (the packet's selector) -> (hit, nrm, diffuse, specular), the last three [64,3,4]"""
        ref, nd = self.ref, diag.nested
        has_mask = not bool(bits.all())
        hit = (dist < INF) & bits                                         # mask = tDistance < maxDist && selector (:157)
        objc = np.where(hit, obj, 0)
        bx, by = bary[:, 0:4], bary[:, 4:8]
        nrm = np.zeros((64, 3, 4), dtype=np.float32); tc = np.zeros((64, 2, 4), dtype=np.float32); tdiff = np.zeros((64, 2), dtype=np.float32)
        diffuse = np.zeros((64, 3, 4), dtype=np.float32); specular = np.zeros((64, 3, 4), dtype=np.float32)
        mid = np.full((64, 4), -1, dtype=np.int64)
        uvT, nrT = ref.uv, ref.nr
        all16 = np.full((4, 4), True)
        with np.errstate(all="ignore"):
            for b in range(16):
                qs = slice(4 * b, 4 * b + 4)
                if not hit[qs].any():
                    continue
                full = bool(hit[qs].all())
                obj0 = int(objc[4 * b, 0])
                if full and bool((objc[qs] == obj0).all()):
                    # (a) 4x4 full, single triangle: Shade with the PACKET's hasMask (:224)
                    nd.blocks_a += 1
                    m = ref.mat_id(obj0)
                    flat = bool(int(ref.mid[obj0]) >> 31)
                    mt = ref.mat(m)
                    if mt.kind != M.TEX:
                        if flat:
                            nd.normals_flat += 1
                            for c in range(3):
                                nrm[qs, c, :] = nrT[obj0, 0, c]
                        else:
                            nd.normals_right += 1
                            for c in range(3):
                                nrm[qs, c, :] = M.lerp_right(nrT[obj0, 0, c], nrT[obj0, 1, c], nrT[obj0, 2, c], bx[qs], by[qs])
                    else:
                        nd.normals_left_a += 1
                        for c in range(2):
                            tc[qs, c, :] = M.lerp_left(uvT[obj0, 0, c], uvT[obj0, 1, c], uvT[obj0, 2, c], bx[qs], by[qs])
                        tdiff[qs] = tc[qs].max(axis=2) - tc[qs].min(axis=2)
                        for c in range(3):
                            nrm[qs, c, :] = M.lerp_left(nrT[obj0, 0, c], nrT[obj0, 1, c], nrT[obj0, 2, c], bx[qs], by[qs])
                    mid[qs] = m
                    before = sum(v for (t, l), v in nd.mips.items() if l > 0)
                    # a full block of a masked packet: rays.SSEMask(q) selects all 16 lanes, the MASKED Shade_ writes them all
                    ref.shade(m, d[qs], nrm[qs], tc[qs], tdiff[qs], all16 if has_mask else None, diffuse[qs], specular[qs], nd)
                    if has_mask:
                        diag.a_masked += 1
                        diag.a_uber_masked += mt.kind == M.UBER
                        diag.a_tex_masked += mt.kind == M.TEX
                    else:
                        diag.a_unmasked += 1
                        diag.a_uber_unmasked += mt.kind == M.UBER
                    if mt.kind == M.TEX and sum(v for (t, l), v in nd.mips.items() if l > 0) > before:
                        diag.a_tex_mip_above_0 += 1
                    continue
                # (b) per quad
                for q in range(4 * b, 4 * b + 4):
                    if not hit[q].any():
                        continue
                    o0 = int(objc[q, 0])
                    if hit[q, 0]:
                        m = ref.mat_id(o0)
                        mid[q] = np.where(hit[q], m, mid[q])
                        for c in range(2):
                            tc[q, c, :] = M.lerp_left(uvT[o0, 0, c], uvT[o0, 1, c], uvT[o0, 2, c], bx[q], by[q])
                        for c in range(3):
                            nrm[q, c, :] = M.lerp_left(nrT[o0, 0, c], nrT[o0, 1, c], nrT[o0, 2, c], bx[q], by[q])
                    for k in range(1, 4):
                        o = int(objc[q, k])
                        if not hit[q, k]:
                            continue
                        if o == o0:
                            if not hit[q, 0]:
                                nd.quirk_lanes += 1
                            continue
                        mid[q, k] = ref.mat_id(o)
                        for c in range(2):
                            tc[q, c, k] = M.lerp_left(uvT[o, 0, c], uvT[o, 1, c], uvT[o, 2, c], bx[q, k], by[q, k])
                        for c in range(3):
                            nrm[q, c, k] = M.lerp_left(nrT[o, 0, c], nrT[o, 1, c], nrT[o, 2, c], bx[q, k], by[q, k])
                tdiff[qs] = F(0.0)
                m0 = int(mid[4 * b, 0])
                if full and bool((mid[qs] == m0).all()):
                    nd.blocks_b += 1                                   # RayGroup<sharedOrigin, 0> whatever the packet is (:308)
                    ref.shade(m0, d[qs], nrm[qs], tc[qs], tdiff[qs], None, diffuse[qs], specular[qs], nd)
                else:
                    ids = []
                    for v in mid[qs][hit[qs]].tolist():
                        if v not in ids:
                            ids.append(v)
                    if len(ids) > 1:
                        nd.blocks_c += 1
                        if -1 in ids:
                            nd.default_meets_others += 1
                    else:
                        nd.blocks_masked_one += 1
                    for m in [v for v in ids if v != -1] + ([-1] if -1 in ids else []):
                        ref.shade(m, d[qs], nrm[qs], tc[qs], tdiff[qs], (mid[qs] == m) & hit[qs], diffuse[qs], specular[qs], nd)
        h3 = hit.reshape(64, 1, 4)
        nrm = np.where(h3, nrm, F(0.0)).astype(np.float32)
        return hit, nrm, np.where(h3, diffuse, F(0.0)).astype(np.float32), np.where(h3, specular, F(0.0)).astype(np.float32)

    def mirror(self, d, pos, nrm, hit, mode):
        """Scene::TraceReflection's rays (:603-618) -> dict(origin, dir, idir [64,3,4], mask uint8 [64], distance [64,4], object [64,4]) in the
        convention of the mirrored packets: zeros for masked lanes, distance inf / -inf (:112-115), object 0"""
        with np.errstate(all="ignore"):
            dt = S.dot3(nrm, d)                                           # Reflect (src/rtbase_math.h:54-58): ray - nrm * (dot + dot)
            dt2 = (dt + dt).reshape(64, 1, 4)
            r = (d - nrm * dt2).astype(np.float32)
            h3 = hit.reshape(64, 1, 4)
            rd = np.where(h3, r, F(0.0)).astype(np.float32)
            ro = np.where(h3, pos + r * F(0.001), F(0.0)).astype(np.float32)
            ri = R.inv(rd + F(0.00000001), mode)                          # SafeInv (src/rtbase.h:117-120)
        sel = (hit.astype(np.uint8) << np.arange(4, dtype=np.uint8).reshape(1, 4)).sum(axis=1).astype(np.uint8)
        return dict(origin=np.ascontiguousarray(ro), dir=np.ascontiguousarray(rd), idir=np.ascontiguousarray(ri), mask=sel,
                    distance=np.where(hit, INF, -INF).astype(np.float32), object=np.zeros((64, 4), dtype=np.int32))

    def nested(self, mp, L, mode, stats, diag: BounceDiag, pkt):
        """the nested RayTrace<0, hasMask> of one mirrored packet (never bounces again: cache.reflections < 1) -> (outColor [64,4,3] float,
        dict(t, u, v, tri_id [64,4], samples [9,64,4]))"""
        bits = ((mp["mask"].reshape(64, 1).astype(np.int32) >> np.arange(4).reshape(1, 4)) & 1).astype(bool)
        n_sel = int(bits.sum())
        if n_sel == 256:
            diag.packets_unmasked += 1
        elif n_sel:
            diag.packets_masked += 1
        else:
            diag.packets_empty += 1
        dist = mp["distance"].copy(); obj = mp["object"].copy(); bary = np.zeros((64, 8), dtype=np.float32)
        stats[2] += n_sel                                                 # stats.TracingRays(CountMaskBits(mask)), :116-117
        stats += self.osc.trace_rays(mp["origin"], mp["dir"], mp["idir"], mp["mask"], dist, obj, bary, 1, 64, False, mode)
        d, org = mp["dir"], mp["origin"]
        hit, nrm, sdiff, sspec = self.samples_rays(d, dist, obj, bary, bits, diag)
        diag.mirrored_lanes += n_sel; diag.mirrored_hits += int(hit.sum()); diag.mirrored_misses += n_sel - int(hit.sum())
        diag.nested.hit_pixels += int(hit.sum())
        with np.errstate(all="ignore"):
            pos = (d * dist.reshape(64, 1, 4) + org).astype(np.float32)
        smp = np.concatenate([nrm.transpose(1, 0, 2), sdiff.transpose(1, 0, 2), sspec.transpose(1, 0, 2)], axis=0)
        sdiff = sdiff.transpose(0, 2, 1); sspec = sspec.transpose(0, 2, 1)
        lDiff, lSpec = light_loop(self.osc, pos, hit, nrm, L, mode, stats, diag.nested, pkt)
        with np.errstate(all="ignore"):
            col = (sdiff * lDiff + sspec * lSpec).astype(np.float32) if len(L[0]) else sdiff
        return col, dict(t=dist, u=bary[:, 0:4].copy(), v=bary[:, 4:8].copy(), tri_id=obj, samples=smp)

    def ray_trace(self, cam, resx, resy, px, py, L, mode, stats, diag: BounceDiag, pkt):
        """Scene::RayTrace of one primary packet with gVals[6] and gVals[7] -> (outColor [64,4,3], dict of the stages' intermediates)"""
        osc, ref = self.osc, self.ref
        dd, ii = O.gen_packet(cam, resx, resy, px, py, mode)
        d = dd.reshape(64, 3, 4).copy()
        org = np.repeat(cam[:3].reshape(1, 3, 1), 4, axis=2).astype(np.float32)
        dist = np.full((64, 4), np.inf, dtype=np.float32); obj = np.zeros((64, 4), dtype=np.int32); bary = np.zeros((64, 8), dtype=np.float32)
        stats[2] += 256
        stats += osc.trace_rays(np.ascontiguousarray(org.reshape(12)), dd, ii, None, dist, obj, bary, 1, 64, True, mode)
        hit, nrm, sdiff, sspec = ref.samples(d, dist, obj, bary, diag.primary)
        diag.primary.hit_pixels += int(hit.sum())
        with np.errstate(all="ignore"):
            pos = (d * dist.reshape(64, 1, 4) + org).astype(np.float32)
        smp = np.concatenate([nrm.transpose(1, 0, 2), sdiff.transpose(1, 0, 2), sspec.transpose(1, 0, 2)], axis=0)
        sdiff = sdiff.transpose(0, 2, 1); sspec = sspec.transpose(0, 2, 1)           # [64, 4, 3]
        # :454-466: reflSel = selector (the hit lanes), the nested call, the blend -- before the lights, specular untouched
        mp = self.mirror(d, pos, nrm, hit, mode)
        refl, nst = self.nested(mp, L, mode, stats, diag, pkt)
        with np.errstate(all="ignore"):
            sdiff = np.where(hit.reshape(64, 4, 1), sdiff + (refl - sdiff) * F(0.3), sdiff).astype(np.float32)
        lDiff, lSpec = light_loop(osc, pos, hit, nrm, L, mode, stats, diag.primary, pkt)
        with np.errstate(all="ignore"):
            col = (sdiff * lDiff + sspec * lSpec).astype(np.float32) if len(L[0]) else sdiff
        return col, dict(samples=smp, t=dist, mirrored=mp, nested=nst, refl=refl)

    def render_packets(self, cam13, resx, resy, packet_xy, lights7=None, ambient=(0.1, 0.1, 0.1), mode=O.MODE_IEEE, diag=None):
        """-> (packet-major B,G,R bytes [n,256,3], TreeStats uint64[4], per-packet intermediates (list of dicts))"""
        cam = np.asarray(cam13, dtype=np.float32)
        lights = np.asarray(lights7 if lights7 is not None else np.zeros((0, 7)), dtype=np.float32).reshape(-1, 7)
        L = (lights, np.asarray(ambient, dtype=np.float32))
        diag = diag if diag is not None else BounceDiag()
        xy = np.asarray(packet_xy, dtype=np.int32).reshape(-1, 2)
        out = np.zeros((len(xy), 256, 3), dtype=np.uint8)
        stats = np.zeros(4, dtype=np.uint64)
        inter = []
        for p, (px, py) in enumerate(xy.tolist()):
            col, it = self.ray_trace(cam, resx, resy, px, py, L, mode, stats, diag, p)
            out[p] = S.conv_color(col).reshape(256, 3)
            inter.append(it)
        return out, stats, inter

    def render(self, cam13, resx, resy, lights7=None, ambient=(0.1, 0.1, 0.1), mode=O.MODE_IEEE, diag=None):
        """-> (frame uint8 [resy,resx,3] (B,G,R), TreeStats, per-packet intermediates, packet list)"""
        xy = S.frame_packets(resx, resy)
        bgr, stats, inter = self.render_packets(cam13, resx, resy, xy, lights7, ambient, mode, diag)
        return S.packets_to_frame(xy, bgr, resx, resy), stats, inter, xy


def stack(inter, *keys):
    """one array over the packets of an intermediate, e.g. stack(inter, "mirrored", "dir") -> [n, 64, 3, 4]"""
    def pick(it):
        for k in keys:
            it = it[k]
        return it
    return np.ascontiguousarray(np.stack([pick(it) for it in inter], axis=0))
