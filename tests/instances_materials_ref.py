"""Test-side restatement of Scene<DBVH>::RayTrace with full shading (gVals[6], src/scene_trace.cpp:145-358, with DBVH::HasShadingData()
answering 1: the project's completion of the reference's TODO, include/snail_instances_materials.h) for primary packets, then the lights
(:484-512, TraceLight :523-601), in float32 numpy: every operation rounded separately, in the order the reference writes it.  Written from
the reference's text -- DBVH::GetSElement / GetMaterialId (src/dbvh/tree.h:211-215, :246-248), ShTriangle::Transform (src/triangle.h:206-219),
the (object, element) comparisons of src/scene_trace.cpp:162, :179-182, :252-253, :263 -- and the header, not from the kernels.  Materials,
textures and the Shade calls are tests/materials_ref.py's, the walks tests/dbvh_ref.py's, the light arithmetic tests/dbvh_shade_ref.py's.
Test infrastructure only."""
from __future__ import annotations

import numpy as np

from tests import dbvh_ref as R
from tests import dbvh_shade_ref as S
from tests import materials_ref as M
from tests import oracle_lib as O

F = np.float32
INF = F(np.inf)


class Diag(M.Diag):
    """materials_ref.Diag and what only an instanced scene can exercise.  quirk_lanes counts the (slot 0, triId 0) quirk here."""

    def __init__(self):
        super().__init__()
        self.cross_instance_same_tri = 0      # full blocks whose 16 lanes hit the same triId of the same BLAS in at least two slots
        self.shared_material_unmasked = 0     # blocks of (b) ending in the unmasked Shade whose lanes lie in at least two different BLASes
        self.rotated_lanes = 0                # hit lanes whose slot's rotation is not the identity
        self.cross_blas_same_tri = 0          # full blocks whose 16 lanes carry the same triId in slots of at least two BLASes
        self.shared_material_unmasked_uber = 0      # ... of shared_material_unmasked, the blocks whose one material is UBER


def rot_vec(rot, v):
    """ShTriangle::Rot (src/triangle.h:206-211): per row x * r.x + y * r.y + z * r.z, three products added left to right"""
    return np.array([(v[0] * rot[k, 0] + v[1] * rot[k, 1]) + v[2] * rot[k, 2] for k in range(3)], dtype=np.float32)


def transform(nr, rot):
    """ShTriangle::Transform (:213-219) on nrm [3, 3] = (nrm0, nrm1 - nrm0, nrm2 - nrm0): back to absolute, through Rot, differences again with
    the ROTATED nrm0.  The translation is not used; nothing is renormalised."""
    nr = np.asarray(nr, dtype=np.float32)
    rot = np.asarray(rot, dtype=np.float32)
    n1 = (nr[1] + nr[0]).astype(np.float32)
    n2 = (nr[2] + nr[0]).astype(np.float32)
    r0, r1, r2 = rot_vec(rot, nr[0]), rot_vec(rot, n1), rot_vec(rot, n2)
    return np.stack([r0, (r1 - r0).astype(np.float32), (r2 - r0).astype(np.float32)]).astype(np.float32)


class InstMaterialsRef(M.MaterialsRef):
    """per_blas[b] = (uv, nrm, mat_index, flat, material_map) of BLAS b's INPUT triangles (permuted by that oracle scene's perm); materials /
    textures: ONE list of RefMaterial / RefTexture for all BLASes.  transform=False skips ShTriangle::Transform: only to show that the
    tests can fail."""

    def __init__(self, ref: R.Ref, per_blas, materials, textures, transform=True):
        self.ref = ref
        self.tab = []
        for osc, (uv, nrm, mat_index, flat, material_map) in zip(ref.blas, per_blas):
            u, n, mid = M.pack_shtris(uv, nrm, mat_index, flat, osc.perm)
            self.tab.append((u, n, mid, np.asarray(material_map, dtype=np.int64)))
        assert len(self.tab) == len(ref.blas)
        self.materials, self.textures = list(materials), list(textures)
        self.do_transform = transform
        self._cache = {}

    def selement(self, slot, tri):
        """DBVH::GetSElement(slot, tri) and DBVH::GetMaterialId(shTri.MatId(), slot) -> (uv [3, 2], nrm [3, 3], flat, material id)"""
        key = (slot, tri)
        if key not in self._cache:
            u, n, mid, mp = self.tab[int(self.ref.bi[slot])]
            nr = transform(n[tri], self.ref.xf[slot][:9].reshape(3, 3)) if self.do_transform else n[tri]
            self._cache[key] = (u[tri], nr, bool(int(mid[tri]) >> 31), int(mp[int(mid[tri]) & 0x7fffffff]))
        return self._cache[key]

    def samples(self, d, dist, slot, tri, bary, diag):
        """:145-358 for one packet: d [64,3,4], dist / slot / tri [64,4], bary [64,8] -> (hit, nrm, diffuse, specular), the last three [64,3,4]"""
        hit = dist < INF
        objc = np.where(hit, slot, 0)          # object  = Condition(mask, tObject, 0), :161
        elc = np.where(hit, tri, 0)            # element = Condition(mask, tElement, 0), :162
        bx, by = bary[:, 0:4], bary[:, 4:8]
        nrm = np.zeros((64, 3, 4), dtype=np.float32); tc = np.zeros((64, 2, 4), dtype=np.float32); tdiff = np.zeros((64, 2), dtype=np.float32)
        diffuse = np.zeros((64, 3, 4), dtype=np.float32); specular = np.zeros((64, 3, 4), dtype=np.float32)
        mid = np.full((64, 4), -1, dtype=np.int64)
        ident = np.eye(3, dtype=np.float32).reshape(9)
        rotated = np.array([not np.array_equal(x[:9], ident) for x in self.ref.xf])
        diag.rotated_lanes += int((hit & rotated[objc]).sum())
        with np.errstate(all="ignore"):
            for b in range(16):
                qs = slice(4 * b, 4 * b + 4)
                if not hit[qs].any():
                    continue
                full = bool(hit[qs].all())
                obj0, el0 = int(objc[4 * b, 0]), int(elc[4 * b, 0])
                if full and bool((elc[qs] == el0).all()) and len(np.unique(self.ref.bi[objc[qs]])) == 1 and len(np.unique(objc[qs])) > 1:
                    diag.cross_instance_same_tri += 1
                if full and bool((elc[qs] == el0).all()) and len(np.unique(self.ref.bi[objc[qs]])) > 1:
                    diag.cross_blas_same_tri += 1
                if full and bool(((objc[qs] == obj0) & (elc[qs] == el0)).all()):
                    # (a) 4x4 full, single triangle of a single instance
                    diag.blocks_a += 1
                    uvT, nrT, flat, m = self.selement(obj0, el0)
                    mt = self.mat(m)
                    if mt.kind != M.TEX:
                        if flat:
                            diag.normals_flat += 1
                            for c in range(3):
                                nrm[qs, c, :] = nrT[0, c]
                        else:
                            diag.normals_right += 1
                            for c in range(3):
                                nrm[qs, c, :] = M.lerp_right(nrT[0, c], nrT[1, c], nrT[2, c], bx[qs], by[qs])
                    else:
                        diag.normals_left_a += 1
                        for c in range(2):
                            tc[qs, c, :] = M.lerp_left(uvT[0, c], uvT[1, c], uvT[2, c], bx[qs], by[qs])
                        tdiff[qs] = tc[qs].max(axis=2) - tc[qs].min(axis=2)
                        for c in range(3):
                            nrm[qs, c, :] = M.lerp_left(nrT[0, c], nrT[1, c], nrT[2, c], bx[qs], by[qs])
                    mid[qs] = m
                    self.shade(m, d[qs], nrm[qs], tc[qs], tdiff[qs], None, diffuse[qs], specular[qs], diag)
                    continue
                # (b) per quad
                for q in range(4 * b, 4 * b + 4):
                    if not hit[q].any():
                        continue
                    o0, e0 = int(objc[q, 0]), int(elc[q, 0])
                    if hit[q, 0]:
                        uvT, nrT, _flat, m = self.selement(o0, e0)
                        mid[q] = np.where(hit[q], m, mid[q])
                        for c in range(2):
                            tc[q, c, :] = M.lerp_left(uvT[0, c], uvT[1, c], uvT[2, c], bx[q], by[q])
                        for c in range(3):
                            nrm[q, c, :] = M.lerp_left(nrT[0, c], nrT[1, c], nrT[2, c], bx[q], by[q])
                    for k in range(1, 4):
                        if not hit[q, k]:
                            continue
                        o, e = int(objc[q, k]), int(elc[q, k])
                        if o == o0 and e == e0:
                            if not hit[q, 0]:
                                diag.quirk_lanes += 1          # (slot 0, triId 0) beside a lane 0 that missed
                            continue
                        uvT, nrT, _flat, mid[q, k] = self.selement(o, e)
                        for c in range(2):
                            tc[q, c, k] = M.lerp_left(uvT[0, c], uvT[1, c], uvT[2, c], bx[q, k], by[q, k])
                        for c in range(3):
                            nrm[q, c, k] = M.lerp_left(nrT[0, c], nrT[1, c], nrT[2, c], bx[q, k], by[q, k])
                tdiff[qs] = F(0.0)
                m0 = int(mid[4 * b, 0])
                if full and bool((mid[qs] == m0).all()):
                    diag.blocks_b += 1
                    if len(np.unique(self.ref.bi[objc[qs]])) > 1:
                        diag.shared_material_unmasked += 1
                        diag.shared_material_unmasked_uber += int(self.mat(m0).kind == M.UBER)
                    self.shade(m0, d[qs], nrm[qs], tc[qs], tdiff[qs], None, diffuse[qs], specular[qs], diag)
                else:
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
        """Scene<DBVH>::RayTrace of one primary packet -> (outColor [64,4,3], samples [9,64,4])"""
        lights, ambient = L
        ref = self.ref
        dd, ii = O.gen_packet(cam, resx, resy, px, py, mode)
        d = dd.reshape(64, 3, 4).copy(); idir = ii.reshape(64, 3, 4).copy()
        org = np.repeat(cam[:3].reshape(1, 3, 1), 4, axis=2).astype(np.float32)
        dist = np.full((64, 4), np.inf, dtype=np.float32)
        obj = np.zeros((64, 4), dtype=np.int32); elem = np.zeros((64, 4), dtype=np.int32); bary = np.zeros((64, 8), dtype=np.float32)
        stats[2] += 256
        stats += ref.traverse(org, d, idir, None, dist, obj, elem, bary, True, False, mode)
        hit, nrm, sdiff, sspec = self.samples(d, dist, obj, elem, bary, diag)
        diag.hit_pixels += int(hit.sum())
        with np.errstate(all="ignore"):
            pos = (d * dist.reshape(64, 1, 4) + org).astype(np.float32)
        smp = np.concatenate([nrm.transpose(1, 0, 2), sdiff.transpose(1, 0, 2), sspec.transpose(1, 0, 2)], axis=0)
        sdiff = sdiff.transpose(0, 2, 1); sspec = sspec.transpose(0, 2, 1)           # [64, 4, 3]

        # lights (:484-512): Scene::TraceLight on the samples' interpolated, rotated normals, DBVH::TraverseShadow
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
            lorg = np.repeat(np.array(lp, dtype=np.float32).reshape(1, 3, 1), 4, axis=2)
            stats += ref.traverse(lorg, np.ascontiguousarray(fl), np.ascontiguousarray(sidir), None, sdist, None, None, None, True, True, mode)
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

    # render_packets / render are MaterialsRef's: they call ray_trace above
    def render_packets(self, cam13, resx, resy, packet_xy, lights7=None, ambient=(0.1, 0.1, 0.1), mode=O.MODE_IEEE, diag=None):
        return super().render_packets(cam13, resx, resy, packet_xy, lights7, ambient, mode, diag if diag is not None else Diag())

    def render(self, cam13, resx, resy, lights7=None, ambient=(0.1, 0.1, 0.1), mode=O.MODE_IEEE, diag=None):
        return super().render(cam13, resx, resy, lights7, ambient, mode, diag if diag is not None else Diag())
