"""Test-side restatement of the transparency continuation TOGETHER with the one mirrored bounce of gVals[7] under full shading of an instanced
scene (include/snail_instances_materials_tree.h): Scene<DBVH>::RayTrace with cache.reflections == 0 calls TraceReflection -- RayTrace with
cache.reflections == 1 on the mirrored rays of its hit lanes -- and blends diffuse += (refl - diffuse) * 0.3 there (src/scene_trace.cpp:454-466,
:603-618), THEN calls TraceTransparency -- RayTrace with cache.reflections == 0 again -- and blends VLerp (:468-483, :620-634), then runs its
lights; a call with cache.reflections == 1 never mirrors and does continue, still with reflections == 1.  By genuine recursion.  A composition,
by import and without an edit: the sample stage with the (slot, triId) keys, the generator, the shadow walk and the frame loop are
tests/instances_materials_transparency_ref.py's (InstTranspRef, InstTranspFrames); the mirror generator with what the instanced walk needs
besides is tests/instances_materials_bounce_ref.py's; the order of the triangle, both blends and the counters (TreeDiag) are
tests/materials_tree_ref.py's, restated here around those; the 2x2 reduction, the tint, ConvColor, the planar store and the clipping are
tests/dbvh_tiles_ref.py's (TilesRef, whose depth shading is SNAIL_RENDER_DEPTH's).  Written from the reference's text and the headers, not from
the kernels.  Test infrastructure only.

Five mutations show that the tests can fail (never used for an expected value):
  miss_not_mirrored     a packet of chain A with no hit lane is not mirrored (reflSel.Any() put back, :454)
  transp_blend_first    the transparency blend runs before the reflection blend
  b_mirrors_again       a call of chain B mirrors once more
  b_not_continued       a call of chain B does not continue through its transparent lanes
  b_lights_a_normals    the lights of a B level read the normals of the A level that started the chain"""
from __future__ import annotations

import numpy as np

from tests import dbvh_tiles_ref as DT
from tests import instances_materials_bounce_ref as IB
from tests import instances_materials_transparency_ref as IT
from tests import materials_bounce_ref as B
from tests import materials_transparency_ref as T
from tests import materials_tree_ref as MT
from tests import oracle_lib as O

F = np.float32
REFLECTIONS, DEPTH, AA4 = DT.REFLECTIONS, DT.DEPTH, DT.AA4
MUTATIONS = ("miss_not_mirrored", "transp_blend_first", "b_mirrors_again", "b_not_continued", "b_lights_a_normals")


class TreeDiag(MT.TreeDiag):
    """materials_tree_ref.TreeDiag (chain A in FrameDiag's fields, chain B keyed (k, depth)) with the instanced sample counters"""

    def __init__(self):
        super().__init__()
        self.samples = IT.SampleDiag()
        self.level_selected = {}           # level >= 1 of chain A -> the lanes that went into it
        self.b_selected = {}               # (k, depth) -> the lanes of B_{k, depth - 1} selected for continuation
        self.pane_shadow_lanes = 0         # (instances_materials_transparency_ref._ShadowWalk's counter; unused without `without`)

    def light_diag(self, level):
        return self.lights.setdefault(level, IT.IM.Diag())

    def b_light_diag(self, k, depth):
        return self.b_lights.setdefault((k, depth), IT.IM.Diag())


class InstTreeFrames(IT.InstTranspFrames):
    """InstTranspFrames with a `reflections` state and a `bounce` switch.  bounce=False and no mutation: exactly InstTranspFrames.
    record: per packet the calls' records in call order, each with `chain` (None: chain A) and `level`, the call's rays, hits and samples,
    and for a call that mirrored its mirrored packet under `mirrored`."""

    def __init__(self, sr: IT.InstTranspRef, bounce=True, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        super().__init__(sr)
        self.bounce = bounce
        self.mutation = mutation
        self.mirror = IB.InstBounceRef(sr.ref).mirror

    def ray_trace(self, rays, level, L, mode, max_depth, stats, diag, pkt, walk, rec, reflections=0, chain=None, a_nrm=None):
        """rays as InstTranspFrames.ray_trace's (the primary packet carries idir0, every other one mask, distance, object, element, bary);
        level = the continuations on the path; reflections = cache.reflections; chain = k for the calls of the B chain that A_k started;
        a_nrm = that A_k's normals -> outColor [64,4,3]"""
        sr, scene, mut = self.sr, self.scene, self.mutation
        primary = "idir0" in rays
        d, org = rays["dir"], rays["origin"]
        if chain is None:
            diag.deepest = max(diag.deepest, level)
            T._bump(diag.a_calls, level)
        else:
            T._bump(diag.b_calls, (chain, level))
        if primary:
            dist = np.full((64, 4), np.inf, dtype=np.float32)
            obj = np.zeros((64, 4), dtype=np.int32); elem = np.zeros((64, 4), dtype=np.int32); bary = np.zeros((64, 8), dtype=np.float32)
            bits = None
            stats[2] += 256
            stats += scene.traverse(org, d, rays["idir0"], None, dist, obj, elem, bary, True, False, mode)
        else:
            bits = ((rays["mask"].reshape(64, 1).astype(np.int32) >> np.arange(4).reshape(1, 4)) & 1).astype(bool)
            dist = rays["distance"].copy(); obj = rays["object"].copy(); elem = rays["element"].copy(); bary = rays["bary"].copy()
            stats[2] += int(bits.sum())                                   # stats.TracingRays(CountMaskBits(mask)), :116-117
            stats += scene.traverse(rays["origin"], rays["dir"], rays["idir"], rays["mask"], dist, obj, elem, bary, False, False, mode)
        smp = sr.samples(d, dist, obj, elem, bary, bits, diag.samples)
        hit, nrm, sdiff, sspec, opacity, sel = smp
        if chain is None and level:
            diag.continuation_hits += int(hit.sum()); diag.continuation_misses += int(bits.sum()) - int(hit.sum())
        r = None
        if rec is not None:
            r = dict(chain=chain, level=level, rays=rays, t=dist, inst=obj, tri_id=elem, bary=bary, samples=IT.planes(smp), opacity=opacity, sel=T.sel_bytes(sel))
            rec.append(r)
        sdiff = sdiff.transpose(0, 2, 1).copy(); sspec = sspec.transpose(0, 2, 1)           # [64, 4, 3]
        with np.errstate(all="ignore"):
            pos = (d * dist.reshape(64, 1, 4) + org).astype(np.float32)
        refl = None
        mirrors = self.bounce and (reflections == 0 or (mut == "b_mirrors_again" and reflections == 1))
        if mirrors and not (mut == "miss_not_mirrored" and not hit.any()):
            # :454-466: reflSel = the hit lanes; the nested call takes place whether or not one is set; the blend comes before the continuation
            n_hit = int(hit.sum())
            if chain is None:
                T._bump(diag.mirrored_full if n_hit == 256 else diag.mirrored_masked if n_hit else diag.mirrored_all_miss, level)
            mp = self.mirror(d, pos, nrm, hit, mode)
            if r is not None:
                r["mirrored"] = mp
            refl = self.ray_trace(mp, level, L, mode, max_depth, stats, diag, pkt, walk, rec, reflections=reflections + 1, chain=level if chain is None else chain,
                                  a_nrm=nrm)
            if mut != "transp_blend_first":
                with np.errstate(all="ignore"):
                    sdiff = np.where(hit.reshape(64, 4, 1), sdiff + (refl - sdiff) * F(0.3), sdiff).astype(np.float32)
        if chain is not None and mut == "b_not_continued":
            sel = np.zeros_like(sel)
        if sel.any() and level == max_depth:
            n = int(sel.sum())
            diag.truncated += n
            if chain is None:
                diag.truncated_a += n
            else:
                diag.truncated_b += n
                diag.truncated_at[(chain, level)] = diag.truncated_at.get((chain, level), 0) + n
            sel = np.zeros_like(sel)
        if sel.any():                                                     # :474-482
            cp = IT.InstTranspRef.continue_packets(d, org, rays["idir"], dist, sel, mode)
            if chain is None:
                T._bump(diag.nested_full if bool(sel.all()) else diag.nested_masked, level + 1)
                diag.level_selected[level + 1] = diag.level_selected.get(level + 1, 0) + int(sel.sum())
            else:
                diag.b_selected[(chain, level + 1)] = diag.b_selected.get((chain, level + 1), 0) + int(sel.sum())
            trans = self.ray_trace(cp, level + 1, L, mode, max_depth, stats, diag, pkt, walk, rec, reflections=reflections, chain=chain, a_nrm=a_nrm)
            with np.errstate(all="ignore"):                               # VLerp(transColor, diffuse, opacity) = a + (b - a) * x
                sdiff = np.where(sel.reshape(64, 4, 1), trans + (sdiff - trans) * opacity.reshape(64, 4, 1), sdiff).astype(np.float32)
        elif chain is None:
            T._bump(diag.nested_none, level + 1)
        if refl is not None and mut == "transp_blend_first":
            with np.errstate(all="ignore"):
                sdiff = np.where(hit.reshape(64, 4, 1), sdiff + (refl - sdiff) * F(0.3), sdiff).astype(np.float32)
        lnrm = nrm
        if chain is not None and mut == "b_lights_a_normals":
            lnrm = np.where(hit.reshape(64, 1, 4), a_nrm, F(0.0)).astype(np.float32)
        ld = diag.light_diag(level) if chain is None else diag.b_light_diag(chain, level)
        lDiff, lSpec = B.light_loop(walk, pos, hit, lnrm, L, mode, stats, ld, pkt)
        with np.errstate(all="ignore"):
            return (sdiff * lDiff + sspec * lSpec).astype(np.float32) if len(L[0]) else sdiff

    def packet_colour(self, cam, resx, resy, px, py, L, mode, max_depth, stats, diag, pkt, walk=None, rec=None):
        """Scene::RayTrace of the primary packet at (px, py) -> outColor [64,4,3] float32"""
        dd, ii = O.gen_packet(cam, resx, resy, px, py, mode)
        org = np.repeat(cam[:3].reshape(1, 3, 1), 4, axis=2).astype(np.float32)
        rays = dict(dir=dd.reshape(64, 3, 4).copy(), origin=org, idir=None, idir0=ii.reshape(64, 3, 4).copy())
        walk = walk if walk is not None else IT._ShadowWalk(self.scene)
        return self.ray_trace(rays, 0, L, mode, max_depth, stats, diag, pkt, walk, rec)

    def render_packets(self, cam13, resx, resy, packet_xy, lights7=None, ambient=(0.1, 0.1, 0.1), mode=O.MODE_IEEE, max_depth=8, diag=None, record=None):
        """-> (packet-major B,G,R bytes [n,256,3], TreeStats uint64[4], truncated lanes, TreeDiag)"""
        return super().render_packets(cam13, resx, resy, packet_xy, lights7, ambient, mode, max_depth, diag if diag is not None else TreeDiag(), record)


class InstTreeTilesRef(DT.TilesRef):
    """RenderTask::Work around InstTreeFrames: colors / packets / frame / tiles of dbvh_tiles_ref.TilesRef with the packet's colour from the tree,
    at one max_depth (SNAIL_RENDER_DEPTH: TilesRef's own depth shading, no level runs).  `truncated` is the count of the LAST colors / packets
    / frame / tiles call; `diag` (when set) is filled by the calls that are not memoised."""

    def __init__(self, sr: IT.InstTranspRef, max_depth=8, mutation=None):
        super().__init__(sr.ref.ref)
        self.frames = InstTreeFrames(sr, mutation=mutation)
        self.max_depth = max_depth
        self.truncated = 0
        self.diag = None
        self._trunc_memo = {}
        self._walk = IT._ShadowWalk(sr.ref.ref)

    def _packet(self, cam, resx, resy, px, py, L, depth, mode, stats, diag, pkt):
        lights, ambient, _, refl = L
        if depth:
            return super()._packet(cam, resx, resy, px, py, L, depth, mode, stats, None, pkt)
        self.frames.bounce = bool(refl)
        return self.frames.packet_colour(cam, resx, resy, px, py, (lights, ambient), mode, self.max_depth, stats, self._run, pkt, self._walk)

    def colors(self, cam13, resx, resy, packet_xy, lights7=None, flags=0, ambient=(0.1, 0.1, 0.1), color=(1.0, 1.0, 1.0), mode=O.MODE_IEEE, diag=None):
        cam = np.ascontiguousarray(cam13, dtype=np.float32)
        lights = np.asarray(lights7 if lights7 is not None else np.zeros((0, 7)), dtype=np.float32).reshape(-1, 7)
        xy = np.asarray(packet_xy, dtype=np.int32).reshape(-1, 2)
        key = (cam.tobytes(), resx, resy, xy.tobytes(), lights.tobytes(), flags, tuple(ambient), tuple(color), mode)
        if self.diag is None and key in self._trunc_memo:
            self.truncated = self._trunc_memo[key]
            return super().colors(cam13, resx, resy, packet_xy, lights7, flags, ambient, color, mode)
        self._run = self.diag if self.diag is not None else TreeDiag()
        before = self._run.truncated
        self._memo.pop(key, None)
        out = super().colors(cam13, resx, resy, packet_xy, lights7, flags, ambient, color, mode)
        self.truncated = self._trunc_memo[key] = self._run.truncated - before
        return out


def call_records(rec, chain, level):
    """render_packets' records of the calls (chain, level), stacked over the packets that made one -> (packet indices, list of records)"""
    idx, rows = [], []
    for p, calls in enumerate(rec):
        for r in calls:
            if r["level"] == level and r.get("chain", None) == chain and r["level"] >= 0:
                idx.append(p); rows.append(r)
    return np.array(idx, dtype=np.int64), rows
