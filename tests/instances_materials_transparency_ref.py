"""Test-side restatement of the transparency continuation under full shading of an instanced scene
(include/snail_instances_materials_transparency.h): Scene<DBVH>::RayTrace's transSel selector (src/scene_trace.cpp:190, :306, :347-349), its
opacity filter (:472), Scene::TraceTransparency's packets (:620-634) and the nested RayTrace<0, hasMask> of every level, blended back up
(:468-483), in float32 numpy, every operation rounded separately in the order the reference writes it.  A composition: the records,
GetSElement / Transform and the data are tests/instances_materials_ref.py's InstMaterialsRef; the input side of a generic packet (a hit = t <
inf AND the selector, the packet's hasMask in branch (a)) and the shadow walk are tests/instances_materials_bounce_ref.py's; TranspMaterial,
`flagged`, Shade with Sample::opacity, the generator and the selector rule are tests/materials_transparency_ref.py's; the walks are
tests/dbvh_ref.py's.  The sample stage is restated here once, for primary and generic packets alike: it has the keys (slot, triId) of the
one, the selector of the other.  Written from the reference's text and the header, not from the kernels.  Test infrastructure only.

Four mutations show that the tests can fail (never used for an expected value):
  tri_only        the equalities are taken on triId alone
  first_wins      in branch (c) the FIRST flagged material of the block's list keeps the selector
  walk_dropped    a packet without a selected lane is walked anyway (its TreeStats are booked)
  blend_late      the blend with the deeper level's colour comes after the lights, on the lit colour"""
from __future__ import annotations

import numpy as np

from tests import dbvh_shade_ref as S
from tests import instances_materials_bounce_ref as IB
from tests import instances_materials_ref as IM
from tests import materials_bounce_ref as B
from tests import materials_ref as M
from tests import materials_transparency_ref as T
from tests import oracle_lib as O

F = np.float32
INF = F(np.inf)
MUTATIONS = ("tri_only", "first_wins", "walk_dropped", "blend_late")


class SampleDiag(T.TranspDiag):
    """materials_transparency_ref.TranspDiag with an instances_materials_ref.Diag for the Shade calls, and what only the selector of an
    instanced scene can exercise"""

    def __init__(self):
        super().__init__()
        self.shade = IM.Diag()
        self.c_deselected_lanes = 0        # lanes an earlier flagged material of a (c) block had selected and the last one took out
        self.same_tri_two_slots_b = 0      # full blocks of 16 hit lanes with ONE triId in at least two slots: (b), not (a)
        self.two_blas_one_material = 0     # full blocks ending in the unmasked Shade of one material whose lanes lie in two BLASes
        self.two_blas_one_flagged = 0      # ... that material carrying fTransparency: ONE candidate for the selector
        self.transparent_opaque_lanes = 0  # lanes of a TRANSPARENT material in the selector before the filter whose opacity sample is >= 1
        self.slots = {}                    # slot -> hit lanes


class FrameDiag(T.FrameDiag):
    def __init__(self):
        super().__init__()
        self.samples = SampleDiag()
        self.level_selected = {}           # level L >= 1 -> the lanes that went into it
        self.level_hit_slots = {}          # level -> set of slots its hits lie in
        self.pane_shadow_lanes = 0         # shadow lanes occluded in the scene and not in `without` (the scene less some instances), all levels

    def light_diag(self, level):
        return self.lights.setdefault(level, IM.Diag())


class _ShadowWalk(IB._ShadowWalk):
    """instances_materials_bounce_ref's shadow walk; with `without` (a dbvh_ref.Ref of the scene less some instances) it also counts the lanes
    that only those instances occlude.  The second walk enters no result."""

    def __init__(self, ref, without=None, diag=None):
        super().__init__(ref)
        self.without, self.diag = without, diag

    def trace_shadow(self, lp, fl, sidir, sdist, n_packets, size, mode):
        if self.without is not None and self.diag is not None:
            other = sdist.copy()
            IB._ShadowWalk(self.without).trace_shadow(lp, fl, sidir, other, n_packets, size, mode)
            st = super().trace_shadow(lp, fl, sidir, sdist, n_packets, size, mode)
            self.diag.pane_shadow_lanes += int(((other > 0) & ~(sdist > 0)).sum())
            return st
        return super().trace_shadow(lp, fl, sidir, sdist, n_packets, size, mode)


class InstTranspRef:
    def __init__(self, ref: IM.InstMaterialsRef, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.ref = ref
        self.mutation = mutation
        self.tr = T.TranspRef.__new__(T.TranspRef)      # its Shade with Sample::opacity asks for the materials, textures and Shade of `ref` alone
        self.tr.ref = ref

    def samples(self, d, dist, slot, tri, bary, bits, diag: SampleDiag):
        """:145-358 and :472 for one packet of a DBVH -- bits None: a primary packet (RayGroup<1, 0>); bits bool [64,4]: a generic one,
        RayGroup<0, hasMask> with hasMask = not all 256 lanes selected.  d [64,3,4], dist / slot / tri [64,4], bary [64,8] ->
        (hit [64,4], nrm, diffuse, specular [64,3,4], opacity [64,4], transSel bool [64,4] after the opacity filter)"""
        ref, nd = self.ref, diag.shade
        has_mask = bits is not None and not bool(bits.all())
        hit = (dist < INF) if bits is None else ((dist < INF) & bits)    # mask = tDistance < maxDist && selector (:157)
        objc = np.where(hit, slot, 0)                                     # object  = Condition(mask, tObject, 0), :161
        elc = np.where(hit, tri, 0)                                       # element = Condition(mask, tElement, 0), :162
        keyo = np.zeros_like(objc) if self.mutation == "tri_only" else objc
        bx, by = bary[:, 0:4], bary[:, 4:8]
        nrm = np.zeros((64, 3, 4), dtype=np.float32); tc = np.zeros((64, 2, 4), dtype=np.float32); tdiff = np.zeros((64, 2), dtype=np.float32)
        diffuse = np.zeros((64, 3, 4), dtype=np.float32); specular = np.zeros((64, 3, 4), dtype=np.float32)
        opacity = np.zeros((64, 4), dtype=np.float32)                    # (read before written: zeros, the library's convention)
        sel = np.zeros((64, 4), dtype=bool)                              # transSel.Clear() (:126)
        mid = np.full((64, 4), -1, dtype=np.int64)
        all16 = np.full((4, 4), True)
        bi = ref.ref.bi
        for s, n in zip(*np.unique(objc[hit], return_counts=True)):
            diag.slots[int(s)] = diag.slots.get(int(s), 0) + int(n)
        with np.errstate(all="ignore"):
            for b in range(16):
                qs = slice(4 * b, 4 * b + 4)
                if not hit[qs].any():
                    continue
                full = bool(hit[qs].all())
                obj0, el0 = int(objc[4 * b, 0]), int(elc[4 * b, 0])
                if full and bool(((keyo[qs] == keyo[4 * b, 0]) & (elc[qs] == el0)).all()):
                    # (a) 4x4 full, single triangle of a single instance: Shade with the PACKET's hasMask (:224); transSel.Mask4(b) from the flag (:190)
                    nd.blocks_a += 1
                    uvT, nrT, flat, m = ref.selement(obj0, el0)
                    mt = ref.mat(m)
                    if mt.kind not in (M.TEX, M.TRANSPARENT):            # mat->flags & fTexCoords
                        for c in range(3):
                            nrm[qs, c, :] = nrT[0, c] if flat else M.lerp_right(nrT[0, c], nrT[1, c], nrT[2, c], bx[qs], by[qs])
                    else:
                        for c in range(2):
                            tc[qs, c, :] = M.lerp_left(uvT[0, c], uvT[1, c], uvT[2, c], bx[qs], by[qs])
                        tdiff[qs] = tc[qs].max(axis=2) - tc[qs].min(axis=2)
                        for c in range(3):
                            nrm[qs, c, :] = M.lerp_left(nrT[0, c], nrT[1, c], nrT[2, c], bx[qs], by[qs])
                    mid[qs] = m
                    if T.flagged(mt):
                        sel[qs] = True
                        diag.blocks_a_flag += 1
                    if mt.kind == M.TRANSPARENT:
                        diag.a_transparent += 1
                        tx = ref.textures[mt.texture]
                        with_mips = tx.sample(tc[qs, 0], tc[qs, 1], np.repeat(tdiff[qs, 0:1], 4, axis=1), np.repeat(tdiff[qs, 1:2], 4, axis=1))[1]
                        diag.a_transparent_texdiff += bool(with_mips.any())
                    self.tr.shade(m, d[qs], nrm[qs], tc[qs], tdiff[qs], all16 if has_mask else None, diffuse[qs], specular[qs], opacity[qs], diag)
                    continue
                if full and bool((elc[qs] == el0).all()) and len(np.unique(objc[qs])) > 1:
                    diag.same_tri_two_slots_b += 1
                # (b) per quad
                for q in range(4 * b, 4 * b + 4):
                    if not hit[q].any():
                        continue
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
                    # one material, 16 rays: RayGroup<sharedOrigin, 0> whatever the packet is (:308); transSel.Mask4(b) from its flag (:306).  The
                    # ids index ONE scene-wide list: two BLASes' triangles of one entry meet here, as one candidate
                    nd.blocks_b += 1
                    two = len(np.unique(bi[objc[qs]])) > 1
                    diag.two_blas_one_material += two
                    if T.flagged(ref.mat(m0)):
                        sel[qs] = True
                        diag.blocks_b_flag += 1
                        diag.two_blas_one_flagged += two
                    self.tr.shade(m0, d[qs], nrm[qs], tc[qs], tdiff[qs], None, diffuse[qs], specular[qs], opacity[qs], diag)
                else:
                    # (c) the block's material list: first appearance over q, then k, among the selected lanes; the default's entry last (:312-332).
                    # Per entry a masked Shade, and for a flagged material transSel[b4 + q] = mask[q] for ALL four quads (:347-349): assigned,
                    # so the last flagged entry of the list is what the block's selector holds
                    ids = []
                    for v in mid[qs][hit[qs]].tolist():
                        if v not in ids:
                            ids.append(v)
                    if len(ids) > 1:
                        nd.blocks_c += 1
                    else:
                        nd.blocks_masked_one += 1
                    prev = None
                    any_flag = False
                    for m in [v for v in ids if v != -1] + ([-1] if -1 in ids else []):
                        mask = (mid[qs] == m) & hit[qs]
                        self.tr.shade(m, d[qs], nrm[qs], tc[qs], tdiff[qs], mask, diffuse[qs], specular[qs], opacity[qs], diag)
                        mt = ref.mat(m)
                        if T.flagged(mt):
                            any_flag = True
                            if prev is not None:
                                diag.c_overwritten += 1
                                diag.c_overwritten_by_opaque_uber += mt.kind == M.UBER and F(mt.dissolve) >= F(1.0)
                                diag.c_lost_selectable += int((prev & (opacity[qs] < F(1.0))).sum())
                                diag.c_deselected_lanes += int(prev.sum())
                                if self.mutation == "first_wins":
                                    continue
                            sel[qs] = mask
                            prev = mask
                    diag.blocks_c_flag += any_flag
        h3 = hit.reshape(64, 1, 4)
        kinds = np.array([ref.mat(int(v)).kind for v in mid.reshape(-1)]).reshape(64, 4)
        diag.transparent_opaque_lanes += int((sel & (kinds == M.TRANSPARENT) & ~(opacity < F(1.0))).sum())
        diag.flagged_opaque_lanes += int((sel & ~(opacity < F(1.0))).sum())
        sel = sel & (opacity < F(1.0))                                   # transSel[q] &= ForWhich(samples[q].opacity < 1.0f) (:472)
        diag.opacity_zero_lanes += int((sel & (opacity == 0)).sum())
        n_sel = int(sel.sum())
        diag.selected_lanes += n_sel
        if n_sel == 256:
            diag.packets_all += 1
        elif n_sel:
            diag.packets_some += 1
        else:
            diag.packets_none += 1
        assert not (sel & ~hit).any()
        return (hit, np.where(h3, nrm, F(0.0)).astype(np.float32), np.where(h3, diffuse, F(0.0)).astype(np.float32), np.where(h3, specular, F(0.0)).astype(np.float32),
                np.where(hit, opacity, F(0.0)).astype(np.float32), sel)

    @staticmethod
    def continue_packets(d, org, idir, dist, sel, mode):
        """materials_transparency_ref's generator, with what the instanced walk needs defined besides: element 0, bary 0"""
        cp = T.TranspRef.continue_packets(d, org, idir, dist, sel, mode)
        cp["element"] = np.zeros((64, 4), dtype=np.int32)
        cp["bary"] = np.zeros((64, 8), dtype=np.float32)
        return cp


def planes(s):
    """samples() -> the nine planes [9, 64, 4]"""
    return np.concatenate([s[1].transpose(1, 0, 2), s[2].transpose(1, 0, 2), s[3].transpose(1, 0, 2)], axis=0)


class InstTranspFrames:
    """Scene<DBVH>::RayTrace with gVals[6] and the transparency continuation, by genuine recursion, as
    materials_transparency_ref.TranspFrames: RayTrace(level) walks, samples, and where a lane is selected calls TraceTransparency ->
    RayTrace(level + 1) -- unless level == max_depth: the lanes are counted as truncated and keep their diffuse -- blends, then runs its own
    lights.  `without`: a dbvh_ref.Ref of the scene less some instances, for FrameDiag.pane_shadow_lanes alone.  `record`: a list that
    receives, per packet, the levels' records (the stage tests' inputs and expected outputs)."""

    def __init__(self, sr: InstTranspRef, without=None):
        self.sr = sr
        self.scene = sr.ref.ref
        self.without = without

    def ray_trace(self, rays, level, L, mode, max_depth, stats, diag: FrameDiag, pkt, walk, rec):
        sr, scene = self.sr, self.scene
        diag.deepest = max(diag.deepest, level)
        d, org = rays["dir"], rays["origin"]
        bary = np.zeros((64, 8), dtype=np.float32)
        obj = np.zeros((64, 4), dtype=np.int32); elem = np.zeros((64, 4), dtype=np.int32)
        if level == 0:
            dist = np.full((64, 4), np.inf, dtype=np.float32)
            bits = None
            stats[2] += 256
            stats += scene.traverse(org, d, rays["idir0"], None, dist, obj, elem, bary, True, False, mode)
        else:
            bits = ((rays["mask"].reshape(64, 1).astype(np.int32) >> np.arange(4).reshape(1, 4)) & 1).astype(bool)
            dist = rays["distance"].copy()
            stats[2] += int(bits.sum())                                   # stats.TracingRays(CountMaskBits(mask)), :116-117
            diag.level_selected[level] = diag.level_selected.get(level, 0) + int(bits.sum())
            stats += scene.traverse(rays["origin"], rays["dir"], rays["idir"], rays["mask"], dist, obj, elem, bary, False, False, mode)
        before = diag.samples.c_overwritten_by_opaque_uber
        smp = sr.samples(d, dist, obj, elem, bary, bits, diag.samples)
        hit, nrm, sdiff, sspec, opacity, sel = smp
        diag.opaque_uber_overwrites[level] = diag.opaque_uber_overwrites.get(level, 0) + int(diag.samples.c_overwritten_by_opaque_uber - before)
        diag.level_hit_slots.setdefault(level, set()).update(int(s) for s in np.unique(obj[hit]))
        if level:
            diag.continuation_hits += int(hit.sum()); diag.continuation_misses += int(bits.sum()) - int(hit.sum())
        if rec is not None:
            rec.append(dict(level=level, rays=rays, t=dist, inst=obj, tri_id=elem, bary=bary, samples=planes(smp), opacity=opacity, sel=T.sel_bytes(sel)))
        sdiff = sdiff.transpose(0, 2, 1).copy(); sspec = sspec.transpose(0, 2, 1)           # [64, 4, 3]
        if sel.any() and level == max_depth:
            diag.truncated += int(sel.sum())
            sel = np.zeros_like(sel)
        trans = None
        if sel.any():                                                     # :474-482
            cp = InstTranspRef.continue_packets(d, org, rays["idir"], dist, sel, mode)
            T._bump(diag.nested_full if bool(sel.all()) else diag.nested_masked, level + 1)
            trans = self.ray_trace(cp, level + 1, L, mode, max_depth, stats, diag, pkt, walk, rec)
            if sr.mutation != "blend_late":
                with np.errstate(all="ignore"):                           # VLerp(transColor, diffuse, opacity) = a + (b - a) * x
                    sdiff = np.where(sel.reshape(64, 4, 1), trans + (sdiff - trans) * opacity.reshape(64, 4, 1), sdiff).astype(np.float32)
        else:
            T._bump(diag.nested_none, level + 1)
            if sr.mutation == "walk_dropped" and level < max_depth:
                cp = InstTranspRef.continue_packets(d, org, rays["idir"], dist, sel, mode)
                stats += scene.traverse(cp["origin"], cp["dir"], cp["idir"], cp["mask"], cp["distance"].copy(), cp["object"].copy(), cp["element"].copy(), cp["bary"].copy(),
                                        False, False, mode)
        with np.errstate(all="ignore"):
            pos = (d * dist.reshape(64, 1, 4) + org).astype(np.float32)
        lDiff, lSpec = B.light_loop(walk, pos, hit, nrm, L, mode, stats, diag.light_diag(level), pkt)
        with np.errstate(all="ignore"):
            col = (sdiff * lDiff + sspec * lSpec).astype(np.float32) if len(L[0]) else sdiff
            if trans is not None and sr.mutation == "blend_late":
                col = np.where(sel.reshape(64, 4, 1), trans + (col - trans) * opacity.reshape(64, 4, 1), col).astype(np.float32)
        return col

    def render_packets(self, cam13, resx, resy, packet_xy, lights7=None, ambient=(0.1, 0.1, 0.1), mode=O.MODE_IEEE, max_depth=8, diag=None, record=None):
        """-> (packet-major B,G,R bytes [n,256,3], TreeStats uint64[4], truncated lanes, FrameDiag)"""
        cam = np.asarray(cam13, dtype=np.float32)
        lights = np.asarray(lights7 if lights7 is not None else np.zeros((0, 7)), dtype=np.float32).reshape(-1, 7)
        L = (lights, np.asarray(ambient, dtype=np.float32))
        diag = diag if diag is not None else FrameDiag()
        walk = _ShadowWalk(self.scene, self.without, diag)
        xy = np.asarray(packet_xy, dtype=np.int32).reshape(-1, 2)
        out = np.zeros((len(xy), 256, 3), dtype=np.uint8)
        stats = np.zeros(4, dtype=np.uint64)
        before = diag.truncated
        for p, (px, py) in enumerate(xy.tolist()):
            dd, ii = O.gen_packet(cam, resx, resy, px, py, mode)
            org = np.repeat(cam[:3].reshape(1, 3, 1), 4, axis=2).astype(np.float32)
            rays = dict(dir=dd.reshape(64, 3, 4).copy(), origin=org, idir=None, idir0=ii.reshape(64, 3, 4).copy())
            rec = None
            if record is not None:
                rec = []
                record.append(rec)
            st0, tr0 = stats.copy(), diag.truncated
            out[p] = S.conv_color(self.ray_trace(rays, 0, L, mode, max_depth, stats, diag, p, walk, rec)).reshape(256, 3)
            if rec is not None:      # the packet's own bytes, TreeStats and truncated lanes: a packet depends on no other
                rec.append(dict(level=-1, bgr=out[p].copy(), stats=stats - st0, truncated=diag.truncated - tr0))
        return out, stats, diag.truncated - before, diag

    def render(self, cam13, resx, resy, lights7=None, ambient=(0.1, 0.1, 0.1), mode=O.MODE_IEEE, max_depth=8, diag=None, record=None):
        """-> (frame uint8 [resy,resx,3] (B,G,R), TreeStats, truncated lanes, FrameDiag, packet list)"""
        xy = S.frame_packets(resx, resy)
        bgr, stats, trunc, diag = self.render_packets(cam13, resx, resy, xy, lights7, ambient, mode, max_depth, diag, record)
        return S.packets_to_frame(xy, bgr, resx, resy), stats, trunc, diag, xy
