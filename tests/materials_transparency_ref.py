"""Test-side restatement of transparent materials under full shading (include/snail_materials_transparency.h): TransparentMaterial<NDotR>::Shade_
(src/shading/transparent_material.h), UberMaterial's opacity (src/shading/uber_material.h, .cpp:5), the transSel selector of Scene::RayTrace
(src/scene_trace.cpp:190, :306, :347-349), its opacity filter (:472) and Scene::TraceTransparency's packets (:620-634), in float32 numpy, every
operation rounded separately in the order the reference writes it.  Written from the reference's text and the header, not from the kernels.
It builds on tests/materials_ref.py and tests/materials_bounce_ref.py by composition: the data, the textures and Shade of the kinds they know
are MaterialsRef's; the sample stage is restated once more here, for primary and generic packets alike, because theirs decide fTexCoords by
`kind == TEX` and know neither Sample::opacity nor the selector.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

from tests import dbvh_ref as R
from tests import dbvh_shade_ref as S
from tests import materials_ref as M
from tests import oracle_lib as O

F = np.float32
INF = F(np.inf)


class TranspMaterial(M.RefMaterial):
    """TransparentMaterial<NDotR>(cSampler, tSampler): `texture` is the colour map, `opacity_texture` the opacity map"""

    def __init__(self, texture, opacity_texture, ndotr=True):
        super().__init__(M.TRANSPARENT, ndotr, texture=texture)
        self.opacity_texture = opacity_texture


def flagged(mt):
    """Material::fTransparency: TransparentMaterial always (transparent_material.h:12), UberMaterial iff dissolveFactor > 0 (uber_material.cpp:5)"""
    return mt.kind == M.TRANSPARENT or (mt.kind == M.UBER and F(mt.dissolve) > F(0.0))


def can_select(mt):
    """... and opacity < 1 can hold for one of its lanes"""
    return mt.kind == M.TRANSPARENT or (mt.kind == M.UBER and F(0.0) < F(mt.dissolve) < F(1.0))


class TranspDiag:
    """What a list of packets exercised (the tests' non-vacuity conditions); `shade` is the materials_ref.Diag of the Shade calls."""

    def __init__(self):
        self.shade = M.Diag()
        self.blocks_a_flag = 0             # single-triangle blocks whose material carries fTransparency (:190)
        self.blocks_b_flag = 0             # one-material full blocks ... (:306)
        self.blocks_c_flag = 0             # blocks on the masked path with at least one flagged material (:347-349)
        self.a_transparent = 0             # ... of the TRANSPARENT kind in particular: the only (a) blocks with texDiff != 0 sampled at level 0
        self.a_transparent_texdiff = 0     # (a) blocks of a TRANSPARENT material whose texDiff would have chosen a level above 0 with mip-mapping on
        self.c_overwritten = 0             # (c) blocks where a later flagged material took an earlier one's lanes out of the selector
        self.c_overwritten_by_opaque_uber = 0   # ... the later one being UBER with dissolve >= 1 (and only that: UBER 0.5 taking lanes is counted above alone)
        self.c_lost_selectable = 0         # lanes with opacity < 1 that the overwrite de-selected
        self.flagged_opaque_lanes = 0      # lanes of the selector before the filter with opacity >= 1
        self.opacity_zero_lanes = 0        # selected lanes with opacity == 0
        self.selected_lanes = 0
        self.packets_none = 0              # packets without a selected lane / with some / with all 256
        self.packets_some = 0
        self.packets_all = 0


class TranspRef:
    def __init__(self, ref: M.MaterialsRef):
        self.ref = ref
        self.osc = ref.osc

    # mat->Shade for one block, with Sample::opacity: d, nrm [4,3,4]; tc [4,2,4]; tdiff [4,2]; mask bool [4,4] or None (unmasked)
    def shade(self, m, d, nrm, tc, tdiff, mask, diffuse, specular, opacity, diag: TranspDiag):
        ref = self.ref
        mt = ref.mat(m)
        if mt.kind != M.TRANSPARENT:
            ref.shade(m, d, nrm, tc, tdiff, mask, diffuse, specular, diag.shade)
            if mt.kind == M.UBER:                                        # s.opacity = floatq(dissFactor), under the mask on the masked path
                opacity[...] = F(mt.dissolve) if mask is None else np.where(mask, F(mt.dissolve), opacity)
            return
        with np.errstate(all="ignore"):
            dn = S.dot3(d, nrm)
            zero = np.zeros((4, 4), dtype=np.float32)
            # cSampler->Sample(samples, sc, 0); tSampler->Sample(samples, sc, 0): mip-mapping off, level 0 whatever texDiff is
            col, mips = ref.textures[mt.texture].sample(tc[:, 0], tc[:, 1], zero, zero)
            opq, mips2 = ref.textures[mt.opacity_texture].sample(tc[:, 0], tc[:, 1], zero, zero)
            assert not mips.any() and not mips2.any()
            dif = [(col[..., c] * dn).astype(np.float32) if mt.ndotr else col[..., c] for c in range(3)]
        for c in range(3):                                               # s.diffuse = s.specular = diffuse; s.opacity = s.temp1.x
            if mask is None:
                diffuse[:, c, :] = dif[c]; specular[:, c, :] = dif[c]
            else:
                diffuse[:, c, :] = np.where(mask, dif[c], diffuse[:, c, :]); specular[:, c, :] = np.where(mask, dif[c], specular[:, c, :])
        opacity[...] = opq[..., 0] if mask is None else np.where(mask, opq[..., 0], opacity)

    def samples(self, d, dist, obj, bary, bits, diag: TranspDiag):
        """:145-358 and :472 for one packet -- bits None: a primary packet (RayGroup<1, 0>); bits bool [64,4]: a generic one, RayGroup<0, hasMask>
        with hasMask = not all 256 lanes selected.  d [64,3,4], dist / obj [64,4], bary [64,8] ->
        (hit [64,4], nrm, diffuse, specular [64,3,4], opacity [64,4], transSel bool [64,4] after the opacity filter)"""
        ref = self.ref
        has_mask = bits is not None and not bool(bits.all())
        hit = (dist < INF) if bits is None else ((dist < INF) & bits)    # mask = tDistance < maxDist && selector (:157)
        objc = np.where(hit, obj, 0)
        bx, by = bary[:, 0:4], bary[:, 4:8]
        nrm = np.zeros((64, 3, 4), dtype=np.float32); tc = np.zeros((64, 2, 4), dtype=np.float32); tdiff = np.zeros((64, 2), dtype=np.float32)
        diffuse = np.zeros((64, 3, 4), dtype=np.float32); specular = np.zeros((64, 3, 4), dtype=np.float32)
        opacity = np.zeros((64, 4), dtype=np.float32)                    # (read before written: zeros, the library's convention)
        sel = np.zeros((64, 4), dtype=bool)                              # transSel.Clear() (:126)
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
                    # (a) 4x4 full, single triangle: Shade with the PACKET's hasMask (:224); transSel.Mask4(b) from the material's flag (:190)
                    m = ref.mat_id(obj0)
                    flat = bool(int(ref.mid[obj0]) >> 31)
                    mt = ref.mat(m)
                    if mt.kind not in (M.TEX, M.TRANSPARENT):            # mat->flags & fTexCoords
                        for c in range(3):
                            nrm[qs, c, :] = nrT[obj0, 0, c] if flat else M.lerp_right(nrT[obj0, 0, c], nrT[obj0, 1, c], nrT[obj0, 2, c], bx[qs], by[qs])
                    else:
                        for c in range(2):
                            tc[qs, c, :] = M.lerp_left(uvT[obj0, 0, c], uvT[obj0, 1, c], uvT[obj0, 2, c], bx[qs], by[qs])
                        tdiff[qs] = tc[qs].max(axis=2) - tc[qs].min(axis=2)
                        for c in range(3):
                            nrm[qs, c, :] = M.lerp_left(nrT[obj0, 0, c], nrT[obj0, 1, c], nrT[obj0, 2, c], bx[qs], by[qs])
                    mid[qs] = m
                    if flagged(mt):
                        sel[qs] = True
                        diag.blocks_a_flag += 1
                    if mt.kind == M.TRANSPARENT:
                        diag.a_transparent += 1
                        tx = ref.textures[mt.texture]
                        with_mips = tx.sample(tc[qs, 0], tc[qs, 1], np.repeat(tdiff[qs, 0:1], 4, axis=1), np.repeat(tdiff[qs, 1:2], 4, axis=1))[1]
                        diag.a_transparent_texdiff += bool(with_mips.any())
                    self.shade(m, d[qs], nrm[qs], tc[qs], tdiff[qs], all16 if has_mask else None, diffuse[qs], specular[qs], opacity[qs], diag)
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
                        if not hit[q, k] or o == o0:
                            continue
                        mid[q, k] = ref.mat_id(o)
                        for c in range(2):
                            tc[q, c, k] = M.lerp_left(uvT[o, 0, c], uvT[o, 1, c], uvT[o, 2, c], bx[q, k], by[q, k])
                        for c in range(3):
                            nrm[q, c, k] = M.lerp_left(nrT[o, 0, c], nrT[o, 1, c], nrT[o, 2, c], bx[q, k], by[q, k])
                tdiff[qs] = F(0.0)
                m0 = int(mid[4 * b, 0])
                if full and bool((mid[qs] == m0).all()):
                    # one material, 16 rays: RayGroup<sharedOrigin, 0> whatever the packet is (:308); transSel.Mask4(b) from its flag (:306)
                    if flagged(ref.mat(m0)):
                        sel[qs] = True
                        diag.blocks_b_flag += 1
                    self.shade(m0, d[qs], nrm[qs], tc[qs], tdiff[qs], None, diffuse[qs], specular[qs], opacity[qs], diag)
                else:
                    # (c) the block's material list: first appearance over q, then k, among the selected lanes; the default's entry last (:312-332).
                    # Per entry a masked Shade, and for a flagged material transSel[b4 + q] = mask[q] for ALL four quads (:347-349): assigned,
                    # so the last flagged entry of the list is what the block's selector holds
                    ids = []
                    for v in mid[qs][hit[qs]].tolist():
                        if v not in ids:
                            ids.append(v)
                    prev = None
                    any_flag = False
                    for m in [v for v in ids if v != -1] + ([-1] if -1 in ids else []):
                        mask = (mid[qs] == m) & hit[qs]
                        self.shade(m, d[qs], nrm[qs], tc[qs], tdiff[qs], mask, diffuse[qs], specular[qs], opacity[qs], diag)
                        mt = ref.mat(m)
                        if flagged(mt):
                            any_flag = True
                            if prev is not None:
                                diag.c_overwritten += 1
                                diag.c_overwritten_by_opaque_uber += mt.kind == M.UBER and F(mt.dissolve) >= F(1.0)
                                diag.c_lost_selectable += int((prev & (opacity[qs] < F(1.0))).sum())
                            sel[qs] = mask
                            prev = mask
                    diag.blocks_c_flag += any_flag
        h3 = hit.reshape(64, 1, 4)
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
        """Scene::TraceTransparency's rays (:620-634) of one packet: d, org [64,3,4]; idir [64,3,4] or None (the primary RayGroup's: SafeInv(dir));
        dist [64,4]; sel bool [64,4] -> dict(origin, dir, idir [64,3,4], mask uint8 [64], distance [64,4], object [64,4], order_on bool) in the
        convention of the mirrored packets: zeros for masked lanes (SafeInv(0) in idir), distance inf / -inf (:112-115), object 0"""
        on = sel & (dist < INF)
        with np.errstate(all="ignore"):
            tl = (dist + F(0.001)).astype(np.float32).reshape(64, 1, 4)
            h3 = on.reshape(64, 1, 4)
            rd = np.where(h3, d, F(0.0)).astype(np.float32)
            ro = np.where(h3, ((d * tl).astype(np.float32) + org).astype(np.float32), F(0.0)).astype(np.float32)
            si = R.inv(rd + F(0.00000001), mode)                         # SafeInv (src/rtbase.h:117-120)
            ri = si if idir is None else np.where(h3, idir, si).astype(np.float32)
        mask = (on.astype(np.uint8) << np.arange(4, dtype=np.uint8).reshape(1, 4)).sum(axis=1).astype(np.uint8)
        return dict(origin=np.ascontiguousarray(ro), dir=np.ascontiguousarray(rd), idir=np.ascontiguousarray(ri), mask=mask,
                    distance=np.where(on, INF, -INF).astype(np.float32), object=np.zeros((64, 4), dtype=np.int32), order_on=bool(on.any()))


def descend(tr: TranspRef, cam13, resx, resy, packet_xy, mode, diag: TranspDiag):
    """The way down of Scene::RayTrace with transparency for a packet list, two generators deep, with the oracle's walks: the primary walk and
    samples (level 0), TraceTransparency's packets of the selected lanes (level 1: generator, walk of RayGroup<0, hasMask>, samples) and the
    packets level 1 would hand on (level 2: generator alone).  A packet without a selected lane makes no nested call (:474): it is in a level's
    `packets` list only if it does.  -> (levels, TreeStats uint64[4]): levels[0] = dict(t, u, v, tri [n,256], samples, opacity, sel);
    levels[1] = dict(cont: the generator's outputs for ALL n packets + order, packets: the indices that nest, dist / obj [m,256], bary [m,64,8],
    samples, opacity, sel of those m); levels[2] = dict(cont: the generator's outputs for those m packets + order (positions in the m))"""
    cam = np.asarray(cam13, dtype=np.float32)
    xy = np.asarray(packet_xy, dtype=np.int32).reshape(-1, 2)
    stats = np.zeros(4, dtype=np.uint64)
    osc = tr.osc
    keys = ("origin", "dir", "idir", "mask", "distance", "object")
    l0, c1, l1, c2, act = [], [], [], [], []
    for p, (px, py) in enumerate(xy.tolist()):
        dd, ii = O.gen_packet(cam, resx, resy, px, py, mode)
        d = dd.reshape(64, 3, 4).copy()
        org = np.repeat(cam[:3].reshape(1, 3, 1), 4, axis=2).astype(np.float32)
        dist = np.full((64, 4), np.inf, dtype=np.float32); obj = np.zeros((64, 4), dtype=np.int32); bary = np.zeros((64, 8), dtype=np.float32)
        stats[2] += 256
        stats += osc.trace_rays(np.ascontiguousarray(org.reshape(12)), dd, ii, None, dist, obj, bary, 1, 64, True, mode)
        s0 = tr.samples(d, dist, obj, bary, None, diag)
        l0.append((dist, bary, obj, s0))
        cp = TranspRef.continue_packets(d, org, None, dist, s0[5], mode)
        c1.append(cp)
        if not cp["order_on"]:
            continue                                                       # transSel.Any() is false: no TraceTransparency (:474)
        act.append(p)
        bits = ((cp["mask"].reshape(64, 1).astype(np.int32) >> np.arange(4).reshape(1, 4)) & 1).astype(bool)
        stats[2] += int(bits.sum())                                        # stats.TracingRays(CountMaskBits(mask)) of the nested call, :116-117
        dist1 = cp["distance"].copy(); obj1 = cp["object"].copy(); bary1 = np.zeros((64, 8), dtype=np.float32)
        stats += osc.trace_rays(cp["origin"], cp["dir"], cp["idir"], cp["mask"], dist1, obj1, bary1, 1, 64, False, mode)
        s1 = tr.samples(cp["dir"], dist1, obj1, bary1, bits, diag)
        l1.append((dist1, bary1, obj1, s1))
        cp2 = TranspRef.continue_packets(cp["dir"], cp["origin"], cp["idir"], dist1, s1[5], mode)
        stats[2] += int((cp2["distance"] == INF).sum())                    # the generator books the next nested call's TracingRays
        c2.append(cp2)

    def planes(o):
        return np.concatenate([o[1].transpose(1, 0, 2), o[2].transpose(1, 0, 2), o[3].transpose(1, 0, 2)], axis=0)

    def sampled(ls):
        return dict(samples=np.stack([planes(x[3]) for x in ls]), opacity=np.stack([x[3][4] for x in ls]).reshape(len(ls), 256), sel=np.stack([sel_bytes(x[3][5]) for x in ls]))

    def cont(cs):
        r = {k: np.ascontiguousarray(np.stack([c[k] for c in cs])) for k in keys}
        r["order"] = np.array([i if c["order_on"] else -1 for i, c in enumerate(cs)], dtype=np.int32)
        return r

    n = len(xy)
    lv0 = dict(t=np.stack([x[0] for x in l0]).reshape(n, 256), u=np.stack([x[1][:, 0:4] for x in l0]).reshape(n, 256), v=np.stack([x[1][:, 4:8] for x in l0]).reshape(n, 256),
               tri=np.stack([x[2] for x in l0]).reshape(n, 256), **sampled(l0))
    lv1 = dict(cont=cont(c1), packets=np.array(act, dtype=np.int64))
    lv2 = {}
    if act:
        m = len(act)
        lv1.update(dist=np.stack([x[0] for x in l1]).reshape(m, 256), obj=np.stack([x[2] for x in l1]).reshape(m, 256), bary=np.stack([x[1] for x in l1]), **sampled(l1))
        lv2 = dict(cont=cont(c2))
    return [lv0, lv1, lv2], stats


class FrameDiag:
    """What a frame exercised.  `samples` is the TranspDiag of every sample stage of the frame (all levels); per level (0 = the primary packets):
    the materials_ref.Diag of its lights, and how its packets went on."""

    def __init__(self):
        self.samples = TranspDiag()
        self.lights = {}                   # level -> materials_ref.Diag (culled / not_culled (packet, light) pairs, lit and occluded pixels)
        self.deepest = 0                   # the deepest level whose RayTrace ran
        self.nested_full = {}              # level L >= 1 -> packets that went into level L as RayGroup<0, 0> (all 256 lanes selected)
        self.nested_masked = {}            # ... as RayGroup<0, 1>
        self.nested_none = {}              # ... packets of level L - 1 that made no nested call
        self.continuation_hits = 0         # selected lanes whose continuation hit something / hit nothing
        self.continuation_misses = 0
        self.truncated = 0                 # lanes that level max_depth still selected: counted, treated as not selected
        self.opaque_uber_overwrites = {}   # level -> (c) blocks of that level's sample stage where UBER with dissolve >= 1 took an earlier flagged material's lanes

    def light_diag(self, level):
        return self.lights.setdefault(level, M.Diag())


def _bump(d, k):
    d[k] = d.get(k, 0) + 1


class TranspFrames:
    """Scene::RayTrace with gVals[6] and the transparency continuation (:468-483, :620-634), by genuine recursion: RayTrace(level) samples,
    and where a lane is selected calls TraceTransparency -> RayTrace(level + 1) -- unless level == max_depth, the cut of
    include/snail_materials_transparency.h: the lanes are counted as truncated and keep their diffuse -- blends, then runs its own lights."""

    def __init__(self, tr: TranspRef):
        self.tr, self.osc = tr, tr.osc

    def ray_trace(self, rays, level, L, mode, max_depth, stats, diag: FrameDiag, pkt):
        """rays: dict(dir [64,3,4], origin [64,3,4], idir [64,3,4] or None, and for level 0 dd / ii / org12 of the generator; for a nested
        level mask, distance, object of the generated packet) -> outColor [64,4,3] float32"""
        from tests import materials_bounce_ref as B
        osc, tr = self.osc, self.tr
        diag.deepest = max(diag.deepest, level)
        d, org = rays["dir"], rays["origin"]
        bary = np.zeros((64, 8), dtype=np.float32)
        if level == 0:
            dist = np.full((64, 4), np.inf, dtype=np.float32); obj = np.zeros((64, 4), dtype=np.int32)
            bits = None
            stats[2] += 256
            stats += osc.trace_rays(rays["org12"], rays["dd"], rays["ii"], None, dist, obj, bary, 1, 64, True, mode)
        else:
            bits = ((rays["mask"].reshape(64, 1).astype(np.int32) >> np.arange(4).reshape(1, 4)) & 1).astype(bool)
            dist = rays["distance"].copy(); obj = rays["object"].copy()
            stats[2] += int(bits.sum())                                   # stats.TracingRays(CountMaskBits(mask)), :116-117
            stats += osc.trace_rays(rays["origin"], rays["dir"], rays["idir"], rays["mask"], dist, obj, bary, 1, 64, False, mode)
        before = diag.samples.c_overwritten_by_opaque_uber
        hit, nrm, sdiff, sspec, opacity, sel = tr.samples(d, dist, obj, bary, bits, diag.samples)
        diag.opaque_uber_overwrites[level] = diag.opaque_uber_overwrites.get(level, 0) + int(diag.samples.c_overwritten_by_opaque_uber - before)
        if level:
            diag.continuation_hits += int(hit.sum()); diag.continuation_misses += int(bits.sum()) - int(hit.sum())
        sdiff = sdiff.transpose(0, 2, 1).copy(); sspec = sspec.transpose(0, 2, 1)           # [64, 4, 3]
        if sel.any() and level == max_depth:
            diag.truncated += int(sel.sum())
            sel = np.zeros_like(sel)
        if sel.any():                                                     # :474-482
            cp = TranspRef.continue_packets(d, org, rays["idir"], dist, sel, mode)
            _bump(diag.nested_full if bool(sel.all()) else diag.nested_masked, level + 1)
            trans = self.ray_trace(cp, level + 1, L, mode, max_depth, stats, diag, pkt)
            with np.errstate(all="ignore"):                               # VLerp(transColor, diffuse, opacity) = a + (b - a) * x
                sdiff = np.where(sel.reshape(64, 4, 1), trans + (sdiff - trans) * opacity.reshape(64, 4, 1), sdiff).astype(np.float32)
        else:
            _bump(diag.nested_none, level + 1)
        with np.errstate(all="ignore"):
            pos = (d * dist.reshape(64, 1, 4) + org).astype(np.float32)
        lDiff, lSpec = B.light_loop(osc, pos, hit, nrm, L, mode, stats, diag.light_diag(level), pkt)
        with np.errstate(all="ignore"):
            return (sdiff * lDiff + sspec * lSpec).astype(np.float32) if len(L[0]) else sdiff

    def render_packets(self, cam13, resx, resy, packet_xy, lights7=None, ambient=(0.1, 0.1, 0.1), mode=O.MODE_IEEE, max_depth=8, diag=None):
        """-> (packet-major B,G,R bytes [n,256,3], TreeStats uint64[4], truncated lanes, FrameDiag)"""
        cam = np.asarray(cam13, dtype=np.float32)
        lights = np.asarray(lights7 if lights7 is not None else np.zeros((0, 7)), dtype=np.float32).reshape(-1, 7)
        L = (lights, np.asarray(ambient, dtype=np.float32))
        diag = diag if diag is not None else FrameDiag()
        xy = np.asarray(packet_xy, dtype=np.int32).reshape(-1, 2)
        out = np.zeros((len(xy), 256, 3), dtype=np.uint8)
        stats = np.zeros(4, dtype=np.uint64)
        before = diag.truncated
        for p, (px, py) in enumerate(xy.tolist()):
            dd, ii = O.gen_packet(cam, resx, resy, px, py, mode)
            org = np.repeat(cam[:3].reshape(1, 3, 1), 4, axis=2).astype(np.float32)
            rays = dict(dir=dd.reshape(64, 3, 4).copy(), origin=org, idir=None, dd=dd, ii=ii, org12=np.ascontiguousarray(org.reshape(12)))
            out[p] = S.conv_color(self.ray_trace(rays, 0, L, mode, max_depth, stats, diag, p)).reshape(256, 3)
        return out, stats, diag.truncated - before, diag

    def render(self, cam13, resx, resy, lights7=None, ambient=(0.1, 0.1, 0.1), mode=O.MODE_IEEE, max_depth=8, diag=None):
        """-> (frame uint8 [resy,resx,3] (B,G,R), TreeStats, truncated lanes, FrameDiag, packet list)"""
        xy = S.frame_packets(resx, resy)
        bgr, stats, trunc, diag = self.render_packets(cam13, resx, resy, xy, lights7, ambient, mode, max_depth, diag)
        return S.packets_to_frame(xy, bgr, resx, resy), stats, trunc, diag, xy


def sel_bytes(sel):
    """bool [..., 64, 4] -> one byte per quad, low 4 bits = lanes"""
    return (sel.astype(np.uint8) << np.arange(4, dtype=np.uint8)).sum(axis=-1).astype(np.uint8)
