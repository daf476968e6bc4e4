"""Test-side restatement of the transparency continuation TOGETHER with the one mirrored bounce of gVals[7] (include/snail_materials_tree.h):
Scene<BVH>::RayTrace with cache.reflections == 0 calls TraceReflection -- RayTrace with cache.reflections == 1 on the mirrored rays of its hit
lanes -- and blends diffuse += (refl - diffuse) * 0.3 there (src/scene_trace.cpp:454-466, :603-618), THEN calls TraceTransparency -- RayTrace with
cache.reflections == 0 again -- and blends VLerp (:468-483, :620-634), then runs its lights; a call with cache.reflections == 1 never mirrors and
does continue, still with reflections == 1.  By genuine recursion, on top of tests/materials_transparency_ref.py (TranspFrames: the sample stage,
the generator, the cut at max_depth) and tests/materials_bounce_ref.py (the mirror generator, the light loop), both imported and not edited; and
with tiles / 4x AA / tint / depth shading on top through the reduction and the stores of tests/materials_tiles_ref.py.  Written from the
reference's text and the header, not from the kernels.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

from tests import materials_bounce_ref as B
from tests import materials_ref as M
from tests import materials_tiles_ref as MT
from tests import materials_transparency_ref as T
from tests import oracle_lib as O

F = np.float32
REFLECTIONS, DEPTH, AA4 = MT.REFLECTIONS, MT.DEPTH, MT.AA4


class TreeDiag(T.FrameDiag):
    """FrameDiag (its fields describe chain A) + what the bounce adds.  A B-chain call is keyed (k, depth): the chain that A_k started, at
    `depth` continuations from the primary packet (depth == k: the mirrored call itself)."""

    def __init__(self):
        super().__init__()
        self.a_calls = {}                  # level k -> RayTrace calls of chain A made at that level (= packets that are part of A_k)
        self.b_calls = {}                  # (k, depth) -> RayTrace calls of chain B
        self.mirrored_full = {}            # k -> mirrored packets of A_k that went as RayGroup<0, 0> (all 256 lanes of A_k hit)
        self.mirrored_masked = {}          # ... as RayGroup<0, 1> with some lane selected
        self.mirrored_all_miss = {}        # ... with NO lane selected: the call takes place all the same (:454)
        self.truncated_a = 0               # lanes that A_D still selected / that a B_{k,D} still selected
        self.truncated_b = 0
        self.truncated_at = {}             # (k, D) -> lanes that B_{k,D} still selected
        self.b_lights = {}                 # (k, depth) -> materials_ref.Diag of that call's lights

    def b_light_diag(self, k, depth):
        return self.b_lights.setdefault((k, depth), M.Diag())


class TreeFrames(T.TranspFrames):
    """TranspFrames with a `reflections` state and a `bounce` switch.  bounce=False: exactly TranspFrames."""

    def __init__(self, tr: T.TranspRef, bounce=True):
        super().__init__(tr)
        self.bounce = bounce
        self.mirror = B.BounceRef(tr.ref).mirror

    def ray_trace(self, rays, level, L, mode, max_depth, stats, diag, pkt, reflections=0, chain=None):
        """rays as TranspFrames.ray_trace's (the primary packet carries dd / ii / org12, every other one mask, distance, object); level = the
        continuations on the path; reflections = cache.reflections; chain = k for the calls of the B chain that A_k started -> outColor [64,4,3]"""
        osc, tr = self.osc, self.tr
        primary = "dd" in rays
        d, org = rays["dir"], rays["origin"]
        bary = np.zeros((64, 8), dtype=np.float32)
        if chain is None:
            diag.deepest = max(diag.deepest, level)
            T._bump(diag.a_calls, level)
        else:
            T._bump(diag.b_calls, (chain, level))
        if primary:
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
        if chain is None:
            diag.opaque_uber_overwrites[level] = diag.opaque_uber_overwrites.get(level, 0) + int(diag.samples.c_overwritten_by_opaque_uber - before)
            if level:
                diag.continuation_hits += int(hit.sum()); diag.continuation_misses += int(bits.sum()) - int(hit.sum())
        sdiff = sdiff.transpose(0, 2, 1).copy(); sspec = sspec.transpose(0, 2, 1)           # [64, 4, 3]
        with np.errstate(all="ignore"):
            pos = (d * dist.reshape(64, 1, 4) + org).astype(np.float32)
        if self.bounce and reflections == 0:
            # :454-466: reflSel = the hit lanes; the nested call takes place whether or not one is set; the blend comes before the continuation
            n_hit = int(hit.sum())
            T._bump(diag.mirrored_full if n_hit == 256 else diag.mirrored_masked if n_hit else diag.mirrored_all_miss, level)
            mp = self.mirror(d, pos, nrm, hit, mode)
            refl = self.ray_trace(mp, level, L, mode, max_depth, stats, diag, pkt, reflections=1, chain=level)
            with np.errstate(all="ignore"):
                sdiff = np.where(hit.reshape(64, 4, 1), sdiff + (refl - sdiff) * F(0.3), sdiff).astype(np.float32)
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
            cp = T.TranspRef.continue_packets(d, org, rays["idir"], dist, sel, mode)
            if chain is None:
                T._bump(diag.nested_full if bool(sel.all()) else diag.nested_masked, level + 1)
            trans = self.ray_trace(cp, level + 1, L, mode, max_depth, stats, diag, pkt, reflections=reflections, chain=chain)
            with np.errstate(all="ignore"):                               # VLerp(transColor, diffuse, opacity) = a + (b - a) * x
                sdiff = np.where(sel.reshape(64, 4, 1), trans + (sdiff - trans) * opacity.reshape(64, 4, 1), sdiff).astype(np.float32)
        elif chain is None:
            T._bump(diag.nested_none, level + 1)
        ld = diag.light_diag(level) if chain is None else diag.b_light_diag(chain, level)
        lDiff, lSpec = B.light_loop(osc, pos, hit, nrm, L, mode, stats, ld, pkt)
        with np.errstate(all="ignore"):
            return (sdiff * lDiff + sspec * lSpec).astype(np.float32) if len(L[0]) else sdiff

    def packet_colour(self, cam, resx, resy, px, py, L, mode, max_depth, stats, diag, pkt):
        """Scene::RayTrace of the primary packet at (px, py) -> outColor [64,4,3] float32"""
        dd, ii = O.gen_packet(cam, resx, resy, px, py, mode)
        org = np.repeat(cam[:3].reshape(1, 3, 1), 4, axis=2).astype(np.float32)
        rays = dict(dir=dd.reshape(64, 3, 4).copy(), origin=org, idir=None, dd=dd, ii=ii, org12=np.ascontiguousarray(org.reshape(12)))
        return self.ray_trace(rays, 0, L, mode, max_depth, stats, diag, pkt)

    def render_packets(self, cam13, resx, resy, packet_xy, lights7=None, ambient=(0.1, 0.1, 0.1), mode=O.MODE_IEEE, max_depth=8, diag=None):
        """-> (packet-major B,G,R bytes [n,256,3], TreeStats uint64[4], truncated lanes, TreeDiag)"""
        return super().render_packets(cam13, resx, resy, packet_xy, lights7, ambient, mode, max_depth, diag if diag is not None else TreeDiag())


def generic_level(fr: TreeFrames, cam13, resx, resy, packet_xy, mode):
    """Level 1 of chain A for a packet list, as the stage test's input: per packet the generator's rays from the primary hits and selector, the
    walk and the samples -> (dict(origin, dir [n,64,3,4], mask [n,64], t [n,256], samples [n,9,64,4], order [n]: the packet's index when a lane
    of the primary packet was selected, else -1), per-packet sample tuples).  A packet outside the level keeps the generator's zeros."""
    cam = np.asarray(cam13, dtype=np.float32)
    xy = np.asarray(packet_xy, dtype=np.int32).reshape(-1, 2)
    tr, osc = fr.tr, fr.osc
    diag = T.TranspDiag()
    out = dict(origin=[], dir=[], mask=[], t=[], samples=[], order=[])
    smp = []
    for p, (px, py) in enumerate(xy.tolist()):
        dd, ii = O.gen_packet(cam, resx, resy, px, py, mode)
        d = dd.reshape(64, 3, 4).copy()
        org = np.repeat(cam[:3].reshape(1, 3, 1), 4, axis=2).astype(np.float32)
        dist = np.full((64, 4), np.inf, dtype=np.float32); obj = np.zeros((64, 4), dtype=np.int32); bary = np.zeros((64, 8), dtype=np.float32)
        osc.trace_rays(np.ascontiguousarray(org.reshape(12)), dd, ii, None, dist, obj, bary, 1, 64, True, mode)
        s0 = tr.samples(d, dist, obj, bary, None, diag)
        cp = T.TranspRef.continue_packets(d, org, None, dist, s0[5], mode)
        bits = ((cp["mask"].reshape(64, 1).astype(np.int32) >> np.arange(4).reshape(1, 4)) & 1).astype(bool)
        dist1 = cp["distance"].copy(); obj1 = cp["object"].copy(); bary1 = np.zeros((64, 8), dtype=np.float32)
        osc.trace_rays(cp["origin"], cp["dir"], cp["idir"], cp["mask"], dist1, obj1, bary1, 1, 64, False, mode)
        s1 = tr.samples(cp["dir"], dist1, obj1, bary1, bits, diag)
        smp.append((cp, dist1, s1))
        out["origin"].append(cp["origin"]); out["dir"].append(cp["dir"]); out["mask"].append(cp["mask"]); out["t"].append(dist1.reshape(256))
        out["samples"].append(np.concatenate([s1[1].transpose(1, 0, 2), s1[2].transpose(1, 0, 2), s1[3].transpose(1, 0, 2)], axis=0))
        out["order"].append(p if cp["order_on"] else -1)
    r = {k: np.ascontiguousarray(np.stack(v)) for k, v in out.items() if k != "order"}
    r["order"] = np.array(out["order"], dtype=np.int32)
    return r, smp


def mirror_level(fr: TreeFrames, smp, mode):
    """Scene::TraceReflection on generic_level's packets (ALL of them, whatever their order word) -> dict(origin, dir, idir [n,64,3,4], mask
    [n,64], distance, object [n,256])"""
    outs = []
    for cp, dist1, s1 in smp:
        hit, nrm = s1[0], s1[1]
        with np.errstate(all="ignore"):
            pos = (cp["dir"] * dist1.reshape(64, 1, 4) + cp["origin"]).astype(np.float32)
        outs.append(fr.mirror(cp["dir"], pos, nrm, hit, mode))
    r = {k: np.ascontiguousarray(np.stack([o[k] for o in outs])) for k in ("origin", "dir", "idir", "mask", "distance", "object")}
    r["distance"] = r["distance"].reshape(len(outs), 256); r["object"] = r["object"].reshape(len(outs), 256)
    return r


class TreeTilesRef(MT.MaterialTilesRef):
    """RenderTask::Work around TreeFrames: colors / packets / frame / tiles of TilesRef with the packet's colour from the tree, at one max_depth.
    `truncated` is the count of the LAST colors / packets / frame / tiles call; `diag` (when set) is filled by the calls that are not memoised."""

    def __init__(self, tr: T.TranspRef, max_depth=8):
        super().__init__(tr.ref)
        self.frames = TreeFrames(tr)
        self.max_depth = max_depth
        self.truncated = 0
        self.diag = None
        self._trunc_memo = {}

    def _packet(self, cam, resx, resy, px, py, L, depth, mode, stats, diag, pkt):
        lights, ambient, _, refl = L
        if depth:
            return super()._packet(cam, resx, resy, px, py, L, depth, mode, stats, diag, pkt)
        self.frames.bounce = bool(refl)
        return self.frames.packet_colour(cam, resx, resy, px, py, (lights, ambient), mode, self.max_depth, stats, self._run, pkt)

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

