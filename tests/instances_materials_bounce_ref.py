"""Test-side restatement of the one mirrored bounce of gVals[7] under full shading of an instanced scene
(include/snail_instances_materials_bounce.h): Scene<DBVH>::RayTrace's call of Scene::TraceReflection (src/scene_trace.cpp:454-466, :603-618)
and the nested RayTrace<0, hasMask> of the mirrored packets with the full-shading branch (:145-358), in float32 numpy, every operation
rounded separately in the order the reference writes it.  A composition: the primary samples, GetSElement / Transform, Shade and the data
are tests/instances_materials_ref.py's InstMaterialsRef; Reflect, light_loop and the blend are tests/materials_bounce_ref.py's; the walks
are tests/dbvh_ref.py's.  The nested sample stage is restated here: it has materials_bounce_ref's input side (a hit = t < inf AND the
selector, the packet's hasMask in branch (a)) around instances_materials_ref's keys (slot, triId).  Written from the reference's text and
the header, not from the kernels.  Test infrastructure only.

Three mutations show that the tests can fail (never used for an expected value):
  raw_nested      the nested records are not passed through ShTriangle::Transform
  tri_only        the nested equalities are taken on triId alone
  primary_normal  the nested lights take the primary sample's normal"""
from __future__ import annotations

import numpy as np

from tests import dbvh_shade_ref as S
from tests import instances_materials_ref as IM
from tests import materials_bounce_ref as B
from tests import materials_ref as M
from tests import oracle_lib as O

F = np.float32
INF = F(np.inf)
MUTATIONS = ("raw_nested", "tri_only", "primary_normal")


class BounceDiag(B.BounceDiag):
    """materials_bounce_ref.BounceDiag with instances_materials_ref.Diag objects, and what only the nested call of an instanced scene
    can exercise"""

    def __init__(self):
        super().__init__()
        self.primary = IM.Diag()
        self.nested = IM.Diag()
        self.nested_slots = {}             # slot -> nested hit lanes
        self.multi_slot_blocks = 0         # nested blocks whose hit lanes lie in more than one slot
        self.multi_slot_quads = 0          # nested quads whose hit lanes lie in more than one slot


class _ShadowWalk:
    """what materials_bounce_ref.light_loop asks of a scene: trace_shadow of ONE packet of 64 quads, by DBVH::TraverseShadow"""

    def __init__(self, ref):
        self.ref = ref

    def trace_shadow(self, lp, fl, sidir, sdist, n_packets, size, mode):
        assert n_packets == 1 and size == 64
        lorg = np.repeat(np.asarray(lp, dtype=np.float32).reshape(1, 3, 1), 4, axis=2)
        return self.ref.traverse(lorg, np.ascontiguousarray(fl.reshape(64, 3, 4)), np.ascontiguousarray(sidir.reshape(64, 3, 4)), None, sdist, None, None, None,
                                 True, True, mode)


class InstBounceRef:
    def __init__(self, ref: IM.InstMaterialsRef, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.ref = ref                     # the primary call's records
        self.walk = _ShadowWalk(ref.ref)
        self.mutation = mutation
        self.nref = ref                    # the nested call's records
        if mutation == "raw_nested":
            self.nref = IM.InstMaterialsRef.__new__(IM.InstMaterialsRef)
            self.nref.__dict__.update(ref.__dict__)
            self.nref.do_transform, self.nref._cache = False, {}

    def samples_rays(self, d, dist, slot, tri, bary, bits, diag: BounceDiag):
        """:145-358 for one generic packet of a DBVH, RayGroup<0, hasMask> with hasMask = not all 256 lanes selected: d [64,3,4], dist / slot /
        tri [64,4], bary [64,8], bits bool [64,4] (the packet's selector) -> (hit, nrm, diffuse, specular), the last three [64,3,4]"""
        ref, nd = self.nref, diag.nested
        has_mask = not bool(bits.all())
        hit = (dist < INF) & bits                                         # mask = tDistance < maxDist && selector (:157)
        objc = np.where(hit, slot, 0)                                     # object  = Condition(mask, tObject, 0), :161
        elc = np.where(hit, tri, 0)                                       # element = Condition(mask, tElement, 0), :162
        keyo = np.zeros_like(objc) if self.mutation == "tri_only" else objc      # what the equalities compare beside the element
        bx, by = bary[:, 0:4], bary[:, 4:8]
        nrm = np.zeros((64, 3, 4), dtype=np.float32); tc = np.zeros((64, 2, 4), dtype=np.float32); tdiff = np.zeros((64, 2), dtype=np.float32)
        diffuse = np.zeros((64, 3, 4), dtype=np.float32); specular = np.zeros((64, 3, 4), dtype=np.float32)
        mid = np.full((64, 4), -1, dtype=np.int64)
        all16 = np.full((4, 4), True)
        ident = np.eye(3, dtype=np.float32).reshape(9)
        rotated = np.array([not np.array_equal(x[:9], ident) for x in ref.ref.xf])
        nd.rotated_lanes += int((hit & rotated[objc]).sum())
        for s, n in zip(*np.unique(objc[hit], return_counts=True)):
            diag.nested_slots[int(s)] = diag.nested_slots.get(int(s), 0) + int(n)
        with np.errstate(all="ignore"):
            for b in range(16):
                qs = slice(4 * b, 4 * b + 4)
                if not hit[qs].any():
                    continue
                full = bool(hit[qs].all())
                diag.multi_slot_blocks += len(np.unique(objc[qs][hit[qs]])) > 1
                obj0, el0 = int(objc[4 * b, 0]), int(elc[4 * b, 0])
                if full and bool(((keyo[qs] == keyo[4 * b, 0]) & (elc[qs] == el0)).all()):
                    # (a) 4x4 full, single triangle of a single instance: Shade with the PACKET's hasMask (:224)
                    nd.blocks_a += 1
                    uvT, nrT, flat, m = ref.selement(obj0, el0)
                    mt = ref.mat(m)
                    if mt.kind != M.TEX:
                        if flat:
                            nd.normals_flat += 1
                            for c in range(3):
                                nrm[qs, c, :] = nrT[0, c]
                        else:
                            nd.normals_right += 1
                            for c in range(3):
                                nrm[qs, c, :] = M.lerp_right(nrT[0, c], nrT[1, c], nrT[2, c], bx[qs], by[qs])
                    else:
                        nd.normals_left_a += 1
                        for c in range(2):
                            tc[qs, c, :] = M.lerp_left(uvT[0, c], uvT[1, c], uvT[2, c], bx[qs], by[qs])
                        tdiff[qs] = tc[qs].max(axis=2) - tc[qs].min(axis=2)
                        for c in range(3):
                            nrm[qs, c, :] = M.lerp_left(nrT[0, c], nrT[1, c], nrT[2, c], bx[qs], by[qs])
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
                    diag.multi_slot_quads += len(np.unique(objc[q][hit[q]])) > 1
                    o0, k0, e0 = int(objc[q, 0]), int(keyo[q, 0]), int(elc[q, 0])
                    if hit[q, 0]:
                        uvT, nrT, _flat, m = ref.selement(o0, e0)
                        mid[q] = np.where(hit[q], m, mid[q])
                        for c in range(2):
                            tc[q, c, :] = M.lerp_left(uvT[0, c], uvT[1, c], uvT[2, c], bx[q], by[q])
                        for c in range(3):
                            nrm[q, c, :] = M.lerp_left(nrT[0, c], nrT[1, c], nrT[2, c], bx[q], by[q])
                    for k in range(1, 4):
                        if not hit[q, k]:
                            continue
                        o, e = int(objc[q, k]), int(elc[q, k])
                        if int(keyo[q, k]) == k0 and e == e0:
                            if not hit[q, 0]:
                                nd.quirk_lanes += 1          # (slot 0, triId 0) beside a lane 0 that missed or is masked
                            continue
                        uvT, nrT, _flat, mid[q, k] = ref.selement(o, e)
                        for c in range(2):
                            tc[q, c, k] = M.lerp_left(uvT[0, c], uvT[1, c], uvT[2, c], bx[q, k], by[q, k])
                        for c in range(3):
                            nrm[q, c, k] = M.lerp_left(nrT[0, c], nrT[1, c], nrT[2, c], bx[q, k], by[q, k])
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
        """materials_bounce_ref's mirrored packet, with what the instanced walk needs defined besides: element 0, bary 0"""
        mp = B.BounceRef.mirror(None, d, pos, nrm, hit, mode)
        mp["element"] = np.zeros((64, 4), dtype=np.int32)
        mp["bary"] = np.zeros((64, 8), dtype=np.float32)
        return mp

    def nested(self, mp, L, mode, stats, diag: BounceDiag, pkt, primary_nrm=None):
        """the nested RayTrace<0, hasMask> of one mirrored packet (never bounces again: cache.reflections < 1) -> (outColor [64,4,3] float,
        dict(t, inst, tri_id [64,4], bary [64,8], samples [9,64,4]))"""
        bits = ((mp["mask"].reshape(64, 1).astype(np.int32) >> np.arange(4).reshape(1, 4)) & 1).astype(bool)
        n_sel = int(bits.sum())
        if n_sel == 256:
            diag.packets_unmasked += 1
        elif n_sel:
            diag.packets_masked += 1
        else:
            diag.packets_empty += 1
        dist = mp["distance"].copy(); obj = mp["object"].copy(); elem = mp["element"].copy(); bary = mp["bary"].copy()
        stats[2] += n_sel                                                 # stats.TracingRays(CountMaskBits(mask)), :116-117
        stats += self.ref.ref.traverse(mp["origin"], mp["dir"], mp["idir"], mp["mask"], dist, obj, elem, bary, False, False, mode)
        d, org = mp["dir"], mp["origin"]
        hit, nrm, sdiff, sspec = self.samples_rays(d, dist, obj, elem, bary, bits, diag)
        diag.mirrored_lanes += n_sel; diag.mirrored_hits += int(hit.sum()); diag.mirrored_misses += n_sel - int(hit.sum())
        diag.nested.hit_pixels += int(hit.sum())
        with np.errstate(all="ignore"):
            pos = (d * dist.reshape(64, 1, 4) + org).astype(np.float32)
        smp = np.concatenate([nrm.transpose(1, 0, 2), sdiff.transpose(1, 0, 2), sspec.transpose(1, 0, 2)], axis=0)
        sdiff = sdiff.transpose(0, 2, 1); sspec = sspec.transpose(0, 2, 1)
        lnrm = np.where(hit.reshape(64, 1, 4), primary_nrm, F(0.0)).astype(np.float32) if self.mutation == "primary_normal" else nrm
        lDiff, lSpec = B.light_loop(self.walk, pos, hit, lnrm, L, mode, stats, diag.nested, pkt)
        with np.errstate(all="ignore"):
            col = (sdiff * lDiff + sspec * lSpec).astype(np.float32) if len(L[0]) else sdiff
        return col, dict(t=dist, inst=obj, tri_id=elem, bary=bary, samples=smp)

    def ray_trace(self, cam, resx, resy, px, py, L, mode, stats, diag: BounceDiag, pkt):
        """Scene<DBVH>::RayTrace of one primary packet with gVals[6] and gVals[7] -> (outColor [64,4,3], dict of the stages' intermediates)"""
        ref = self.ref
        dd, ii = O.gen_packet(cam, resx, resy, px, py, mode)
        d = dd.reshape(64, 3, 4).copy(); idir = ii.reshape(64, 3, 4).copy()
        org = np.repeat(cam[:3].reshape(1, 3, 1), 4, axis=2).astype(np.float32)
        dist = np.full((64, 4), np.inf, dtype=np.float32)
        obj = np.zeros((64, 4), dtype=np.int32); elem = np.zeros((64, 4), dtype=np.int32); bary = np.zeros((64, 8), dtype=np.float32)
        stats[2] += 256
        stats += ref.ref.traverse(org, d, idir, None, dist, obj, elem, bary, True, False, mode)
        hit, nrm, sdiff, sspec = ref.samples(d, dist, obj, elem, bary, diag.primary)
        diag.primary.hit_pixels += int(hit.sum())
        with np.errstate(all="ignore"):
            pos = (d * dist.reshape(64, 1, 4) + org).astype(np.float32)
        smp = np.concatenate([nrm.transpose(1, 0, 2), sdiff.transpose(1, 0, 2), sspec.transpose(1, 0, 2)], axis=0)
        sdiff = sdiff.transpose(0, 2, 1); sspec = sspec.transpose(0, 2, 1)           # [64, 4, 3]
        # :454-466: reflSel = selector (the hit lanes), the nested call, the blend -- before the lights, specular untouched
        mp = self.mirror(d, pos, nrm, hit, mode)
        refl, nst = self.nested(mp, L, mode, stats, diag, pkt, primary_nrm=nrm)
        with np.errstate(all="ignore"):
            sdiff = np.where(hit.reshape(64, 4, 1), sdiff + (refl - sdiff) * F(0.3), sdiff).astype(np.float32)
        lDiff, lSpec = B.light_loop(self.walk, pos, hit, nrm, L, mode, stats, diag.primary, pkt)
        with np.errstate(all="ignore"):
            col = (sdiff * lDiff + sspec * lSpec).astype(np.float32) if len(L[0]) else sdiff
        return col, dict(samples=smp, t=dist, u=bary[:, 0:4].copy(), v=bary[:, 4:8].copy(), inst=obj, tri_id=elem, mirrored=mp, nested=nst, refl=refl)

    def render_packets(self, cam13, resx, resy, packet_xy, lights7=None, ambient=(0.1, 0.1, 0.1), mode=O.MODE_IEEE, diag=None):
        """-> (packet-major B,G,R bytes [n,256,3], TreeStats uint64[4], per-packet intermediates (list of dicts, with each packet's own bytes
        and TreeStats under "bgr" and "stats"))"""
        cam = np.asarray(cam13, dtype=np.float32)
        lights = np.asarray(lights7 if lights7 is not None else np.zeros((0, 7)), dtype=np.float32).reshape(-1, 7)
        L = (lights, np.asarray(ambient, dtype=np.float32))
        diag = diag if diag is not None else BounceDiag()
        xy = np.asarray(packet_xy, dtype=np.int32).reshape(-1, 2)
        out = np.zeros((len(xy), 256, 3), dtype=np.uint8)
        stats = np.zeros(4, dtype=np.uint64)
        inter = []
        for p, (px, py) in enumerate(xy.tolist()):
            before = stats.copy()
            col, it = self.ray_trace(cam, resx, resy, px, py, L, mode, stats, diag, p)
            out[p] = S.conv_color(col).reshape(256, 3)
            it["bgr"], it["stats"] = out[p].copy(), stats - before      # the packet's own bytes and TreeStats: a packet depends on no other
            inter.append(it)
        return out, stats, inter

    def render(self, cam13, resx, resy, lights7=None, ambient=(0.1, 0.1, 0.1), mode=O.MODE_IEEE, diag=None):
        """-> (frame uint8 [resy,resx,3] (B,G,R), TreeStats, per-packet intermediates, packet list)"""
        xy = S.frame_packets(resx, resy)
        bgr, stats, inter = self.render_packets(cam13, resx, resy, xy, lights7, ambient, mode, diag)
        return S.packets_to_frame(xy, bgr, resx, resy), stats, inter, xy


stack = B.stack
