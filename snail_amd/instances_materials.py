"""Full shading of instanced scenes: per-BLAS ShTriangle records and material maps, ONE scene-wide material and texture list, over the C-ABI
of include/snail_instances_materials.h.

  InstancedMaterialSet(isc, per_blas, materials, textures)   <-> DBVH::GetSElement (the BLAS's ShTriangle through ShTriangle::Transform) and
                                                                 DBVH::GetMaterialId over Scene::materials
  .shade_packets / .render / .render_packets / .render_image_host   <-> Scene<DBVH>::RayTrace with gVals[6] and HasShadingData() = 1 (this
                                                                 project's completion of the reference's TODO), primary packets and their lights
  .mirror_packets / .shade_rays, reflections=True           <-> the one mirrored bounce of gVals[7] (Scene::TraceReflection and its nested
                                                                 RayTrace<0, hasMask>), include/snail_instances_materials_bounce.h
  InstancedMaterialSet(..., transparent=True), .can_select_transparent, .shade_packets_transp / .shade_rays_transp / .continue_packets,
  .render_transparent / .render_transparent_packets / .render_transparent_image_host
                                                            <-> the transparency continuation (Scene::TraceTransparency and its nested
                                                                 RayTrace<0, hasMask>, level by level), include/snail_instances_materials_transparency.h
  .mirror_rays / .tree_frame_packets / .render_tree_tiles_host / .render_tree_frame_host / .set_level_budget / .level_bytes
                                                            <-> the continuation TOGETHER with the bounce, tile lists, 4x AA, depth shading and
                                                                 the tint (RenderTask::Work), include/snail_instances_materials_tree.h

  InstancedMaterialSet.from_dev(isc, per_blas, ...), DevBlasShading, .rebuild_blas_dev / .update_blas_dev
                                                            <-> an animated instanced scene: BLASes of Scene.from_fast_dev whose records are packed
                                                                 on the device and follow their rebuilds, include/snail_instances_materials_dynamic.h

Materials, textures and pack_shtris are snail_amd.materials'."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .instances import InstancedScene
from . import materials as P
from .materials import RENDER_REFLECTIONS, SAMPLE_COMPONENTS, _material_records, _texture_array, pack_shtris
from .scene import _stream_ptr, _torch


class _BlasShading(C.Structure):
    _fields_ = [("shtris64", C.c_void_p), ("nTris", C.c_int32), ("matMap", C.c_void_p), ("nMap", C.c_int32)]


class _BlasShadingDev(C.Structure):
    _fields_ = _BlasShading._fields_ + [("d_uv6", C.c_void_p), ("d_matIdx", C.c_void_p), ("d_flat", C.c_void_p), ("d_perm", C.c_void_p), ("d_nrm9", C.c_void_p),
                                        ("d_verts9", C.c_void_p)]


class _BlasRebuild(C.Structure):
    _fields_ = [("blas", C.c_int32), ("d_verts9", C.c_void_p), ("d_nrm9", C.c_void_p), ("d_perm", C.c_void_p), ("d_info", C.c_void_p)]


class DevBlasShading:
    """The shading data of a Scene.from_fast_dev BLAS for InstancedMaterialSet.from_dev: device tensors on the scene's device describing the
    INPUT triangles -- d_uv float32 [n, 3, 2], d_mat_index int32 [n], d_flat uint8 [n] or None (none flat) -- the BLAS's material_map (host),
    and the normals: d_nrm float32 [n, 3, 3], or None for face normals of d_verts float32 [n, 3, 3]."""

    def __init__(self, d_uv, d_mat_index, d_flat, material_map, d_nrm=None, d_verts=None):
        self.d_uv, self.d_mat_index, self.d_flat, self.material_map, self.d_nrm, self.d_verts = d_uv, d_mat_index, d_flat, material_map, d_nrm, d_verts


def _addr(t):
    return None if t is None else (t.data_ptr() if hasattr(t, "data_ptr") else t.ctypes.data)


def create_instanced_set(instances_handle, shtris_list, map_list, materials, textures, transparent: bool = False):
    """snail_instances_materials_create over raw arguments (per BLAS: uint8 [n, 64] records, int32 map) -> handle (c_void_p); SnailError with
    the library's text when the set is refused.  transparent=True: snail_instances_materials_create_transparent, with the materials'
    opacity_texture"""
    sh = [np.ascontiguousarray(s, dtype=np.uint8).reshape(-1, 64) for s in shtris_list]
    mp = [np.ascontiguousarray(m, dtype=np.int32).reshape(-1) for m in map_list]
    if len(sh) != len(mp):
        raise ValueError("one record array and one map per BLAS")
    per = (_BlasShading * max(len(sh), 1))()
    for b in range(len(sh)):
        per[b].shtris64, per[b].nTris = (sh[b].ctypes.data if len(sh[b]) else None), len(sh[b])
        per[b].matMap, per[b].nMap = (mp[b].ctypes.data if len(mp[b]) else None), len(mp[b])
    recs = _material_records(materials)
    tex = _texture_array(textures)
    if transparent:
        op = np.ascontiguousarray([getattr(m, "opacity_texture", 0) for m in materials], dtype=np.int32)
        h = _lib.lib().snail_instances_materials_create_transparent(instances_handle, C.cast(per, C.c_void_p) if len(sh) else None, len(sh),
                                                                    _lib.ptr(recs) if len(recs) else None, len(recs), _lib.ptr(op) if len(op) else None,
                                                                    C.cast(tex, C.c_void_p) if len(textures) else None, len(textures))
        if not h:
            raise _lib.SnailError("snail_instances_materials_create_transparent: %s" % _lib.lib().snail_last_error().decode())
        return C.c_void_p(h)
    h = _lib.lib().snail_instances_materials_create(instances_handle, C.cast(per, C.c_void_p) if len(sh) else None, len(sh), _lib.ptr(recs) if len(recs) else None,
                                                    len(recs), C.cast(tex, C.c_void_p) if len(textures) else None, len(textures))
    if not h:
        raise _lib.SnailError("snail_instances_materials_create: %s" % _lib.lib().snail_last_error().decode())
    return C.c_void_p(h)


class _FrameStep:
    """include/snail_instances_materials_rebuild_all.h.  A base of InstancedMaterialSet, so that the class's own method list stays the list of
    include/snail_instances_materials*.h up to snail_instances_materials_dynamic.h, which the tests of those headers enumerate."""

    def rebuild_all_dev(self, entries, xf12, blas_index=None, stream=None, perm=None, info=None):
        """The per-frame step in one call (snail_instances_materials_rebuild_all_dev): rebuild_blas_dev(entries) followed by
        isc.update_dev(xf12, blas_index, perm=perm, info=info) under one set of locks -- the BLASes' builds in one batched pass, their records
        packed again, then the top-level tree over the new BLAS root boxes (a BLAS whose build is refused contributes the box of the tree it
        keeps), all on `stream`, no host wait.  -> (blas_info int32 [k, 6] as rebuild_blas_dev's, top_perm, top_info as update_dev's)."""
        arr, binfo, items = self._rebuild_entries("rebuild_all_dev", entries, stream)
        isc = self.isc
        n, info = isc._update_dev_begin(xf12, blas_index, stream, perm, info)
        _lib.check(_lib.lib().snail_instances_materials_rebuild_all_dev(self._h, C.cast(arr, C.c_void_p) if items else None, len(items), _lib.ptr(xf12), _lib.ptr(blas_index),
                                                                        n, _lib.ptr(isc._d_perm), _lib.ptr(info), _stream_ptr(stream)),
                   "snail_instances_materials_rebuild_all_dev")
        self._rebuilt(binfo, items)
        top_perm, top_info = isc._update_dev_end(n, stream, perm, info)
        return binfo, top_perm, top_info


class InstancedMaterialSet(_FrameStep):
    """The shading data of an instanced scene on its GPU.  per_blas[b] = (uv, nrm, mat_index, flat, material_map) of BLAS b's INPUT triangles
    (the order that scene was built from; its bvh.perm permutes them into triId order); a map entry is -1 (the default material) or an index
    into `materials`, ONE list for all BLASes.  The instanced scene (and through it the BLAS scenes) is kept alive by this object.  The
    instance records are read at every launch: after isc.update / update_dev the same set shades with the new rotations.
    transparent=True: the materials may be of the kinds that can select a transparent lane (Material.transparent, Material.uber with any
    dissolve); such a set is shaded by the *_transp / render_transparent* methods alone."""

    def __init__(self, isc: InstancedScene, per_blas, materials=(), textures=(), transparent: bool = False):
        self.isc = isc
        self._h = None
        per_blas = list(per_blas)
        if len(per_blas) != len(isc.blas):
            raise _lib.SnailError("InstancedMaterialSet: shading data of %d BLASes for an instanced scene of %d" % (len(per_blas), len(isc.blas)))
        self.shtris, maps = [], []
        for b, (uv, nrm, mat_index, flat, material_map) in enumerate(per_blas):
            sc = isc.blas[b]
            perm = None if getattr(sc, "_fast_dev", False) else getattr(sc.bvh, "perm", None)
            if perm is None:
                raise _lib.SnailError("InstancedMaterialSet: BLAS %d carries no host permutation (BVH slot -> input triangle); build it from host triangles" % b)
            self.shtris.append(pack_shtris(uv, nrm, mat_index, flat, perm))
            maps.append(material_map)
        self._h = create_instanced_set(isc._h, self.shtris, maps, list(materials), list(textures), transparent)

    # ---- include/snail_instances_materials_dynamic.h: BLASes that deform on the device ---------------------------------------------------------
    @classmethod
    def from_dev(cls, isc: InstancedScene, per_blas, materials=(), textures=(), transparent: bool = False, stream=None):
        """The set of an instanced scene with Scene.from_fast_dev BLASes (snail_instances_materials_create_dev).  per_blas[b] is the
        constructor's host 5-tuple for a BLAS built from host triangles and a DevBlasShading for a Scene.from_fast_dev BLAS, whose records are
        packed on the device through that scene's d_perm and packed again by rebuild_blas_dev / update_blas_dev.  The device tensors of uv,
        material index and flat are copied: they need not outlive the call."""
        torch = _torch()
        per_blas = list(per_blas)
        if len(per_blas) != len(isc.blas):
            raise _lib.SnailError("InstancedMaterialSet.from_dev: shading data of %d BLASes for an instanced scene of %d" % (len(per_blas), len(isc.blas)))
        self = cls.__new__(cls)
        self.isc, self._h, self.shtris, self._dynamic = isc, None, [], True
        per = (_BlasShadingDev * max(len(per_blas), 1))()
        keep = []
        for b, pb in enumerate(per_blas):
            sc = isc.blas[b]
            fast = getattr(sc, "_fast_dev", False)
            if isinstance(pb, DevBlasShading) != bool(fast):
                raise _lib.SnailError("InstancedMaterialSet.from_dev: BLAS %d: a Scene.from_fast_dev BLAS takes a DevBlasShading, a BLAS built from host "
                                      "triangles the host tuple (uv, nrm, mat_index, flat, material_map)" % b)
            if fast:
                n, d = sc._fast_n, sc._dev()
                P.MaterialSet._check_dev("d_uv", pb.d_uv, torch.float32, n * 6, d)
                P.MaterialSet._check_dev("d_mat_index", pb.d_mat_index, torch.int32, n, d)
                P.MaterialSet._check_dev("d_flat", pb.d_flat, torch.uint8, n, d, optional=True)
                P.MaterialSet._check_dev("d_nrm", pb.d_nrm, torch.float32, n * 9, d, optional=True)
                P.MaterialSet._check_dev("d_verts", pb.d_verts, torch.float32, n * 9, d, optional=True)
                mp = np.ascontiguousarray(pb.material_map, dtype=np.int32).reshape(-1)
                per[b].nTris = n
                per[b].d_uv6, per[b].d_matIdx, per[b].d_flat, per[b].d_perm = _addr(pb.d_uv), _addr(pb.d_mat_index), _addr(pb.d_flat), _addr(sc.d_perm)
                per[b].d_nrm9, per[b].d_verts9 = _addr(pb.d_nrm), _addr(pb.d_verts)
                self.shtris.append(None)
            else:
                uv, nrm, mat_index, flat, material_map = pb
                perm = getattr(sc.bvh, "perm", None)
                if perm is None:
                    raise _lib.SnailError("InstancedMaterialSet.from_dev: BLAS %d carries no host permutation (BVH slot -> input triangle)" % b)
                sh = np.ascontiguousarray(pack_shtris(uv, nrm, mat_index, flat, perm), dtype=np.uint8).reshape(-1, 64)
                mp = np.ascontiguousarray(material_map, dtype=np.int32).reshape(-1)
                per[b].shtris64, per[b].nTris = (sh.ctypes.data if len(sh) else None), len(sh)
                self.shtris.append(sh)
            per[b].matMap, per[b].nMap = (mp.ctypes.data if len(mp) else None), len(mp)
            keep.append(mp)
        materials, textures = list(materials), list(textures)
        recs = _material_records(materials)
        tex = _texture_array(textures)
        op = np.ascontiguousarray([getattr(m, "opacity_texture", 0) for m in materials] or [0], dtype=np.int32) if transparent else None
        h = _lib.lib().snail_instances_materials_create_dev(isc._h, C.cast(per, C.c_void_p) if len(per_blas) else None, len(per_blas), _lib.ptr(recs) if len(recs) else None,
                                                            len(recs), _lib.ptr(op), C.cast(tex, C.c_void_p) if len(textures) else None, len(textures), _stream_ptr(stream))
        if not h:
            raise _lib.SnailError("snail_instances_materials_create_dev: %s" % _lib.lib().snail_last_error().decode())
        self._h = C.c_void_p(h)
        return self

    def _blas_list(self, what, entries, words, stream):
        """the SnailBlasRebuild list of rebuild_blas_dev / update_blas_dev -> (array, info tensor [k, words], [(b, scene, d_verts, d_nrm)])"""
        if not getattr(self, "_dynamic", False):
            raise _lib.SnailError("%s: the set was not made by InstancedMaterialSet.from_dev" % what)
        torch = _torch()
        items = list(entries.items())
        d = self.isc._dev()
        info = torch.empty((len(items), words), dtype=torch.int32, device=d)
        if stream is not None:
            info.record_stream(stream)
        arr = (_BlasRebuild * max(len(items), 1))()
        for k, (b, _) in enumerate(items):
            b = int(b)
            if not (0 <= b < len(self.isc.blas)) or not getattr(self.isc.blas[b], "_fast_dev", False):
                raise _lib.SnailError("%s: BLAS %d is out of range, or not a Scene.from_fast_dev BLAS (a BLAS built from host triangles is never rebuilt)" % (what, b))
            arr[k].blas = b
            arr[k].d_perm = _addr(self.isc.blas[b].d_perm)
            arr[k].d_info = info.data_ptr() + k * words * 4
        return arr, info, items

    def rebuild_blas_dev(self, entries, stream=None):
        """entries = {b: (d_verts, d_nrm or None)}: rebuild every listed Scene.from_fast_dev BLAS from its new vertices, as Scene.rebuild_fast_dev
        does, and pack the records of all of them again through the new permutations in one launch on the same stream
        (snail_instances_materials_rebuild_dev); face normals of d_verts where d_nrm is None.  No host wait.  -> int32 [k, 6] device tensor, a
        row per entry in the dictionary's order: the build's {status, nNodes, depth, n}, then {records committed (0 / 1), zeroed triangles}.
        A BLAS whose status is not 0 keeps tree, perm and records.  Each scene's d_perm is written.  The top-level tree is NOT touched: follow
        with isc.update_dev (or isc.update) before the next frame.  The tensors must stay alive and unchanged until the work has run."""
        arr, info, items = self._rebuild_entries("rebuild_blas_dev", entries, stream)
        _lib.check(_lib.lib().snail_instances_materials_rebuild_dev(self._h, C.cast(arr, C.c_void_p) if items else None, len(items), _stream_ptr(stream)),
                   "snail_instances_materials_rebuild_dev")
        self._rebuilt(info, items)
        return info

    def _rebuild_entries(self, what, entries, stream):
        """the checked SnailBlasRebuild list of rebuild_blas_dev / rebuild_all_dev"""
        arr, info, items = self._blas_list(what, entries, 6, stream)
        torch = _torch()
        for k, (b, (d_verts, d_nrm)) in enumerate(items):
            sc = self.isc.blas[int(b)]
            if sc._check_verts(d_verts, sc._dev()) != sc._fast_n:
                raise ValueError("BLAS %d: d_verts must hold %d triangles" % (int(b), sc._fast_n))
            P.MaterialSet._check_dev("d_nrm", d_nrm, torch.float32, sc._fast_n * 9, sc._dev(), optional=True)
            arr[k].d_verts9, arr[k].d_nrm9 = _addr(d_verts), _addr(d_nrm)
        return arr, info, items

    def _rebuilt(self, info, items):
        for k, (b, _) in enumerate(items):
            sc = self.isc.blas[int(b)]
            sc.d_info = info[k, :4]
            sc._stale = True           # .bvh / .perm / .depth are read back when next asked, as after Scene.rebuild_fast_dev

    def update_blas_dev(self, entries, stream=None):
        """entries = {b: (d_nrm or None, d_verts or None)}: pack the records of the listed BLASes again through each scene's d_perm, and nothing
        else (snail_instances_materials_update_dev): after a BLAS scene was rebuilt by Scene.rebuild_fast_dev or through another set, or for
        new normals alone.  -> int32 [k, 2] device tensor, rows {1, zeroed triangles}."""
        arr, info, items = self._blas_list("update_blas_dev", entries, 2, stream)
        torch = _torch()
        for k, (b, (d_nrm, d_verts)) in enumerate(items):
            sc = self.isc.blas[int(b)]
            P.MaterialSet._check_dev("d_nrm", d_nrm, torch.float32, sc._fast_n * 9, sc._dev(), optional=True)
            P.MaterialSet._check_dev("d_verts", d_verts, torch.float32, sc._fast_n * 9, sc._dev(), optional=True)
            arr[k].d_verts9, arr[k].d_nrm9 = _addr(d_verts), _addr(d_nrm)
        _lib.check(_lib.lib().snail_instances_materials_update_dev(self._h, C.cast(arr, C.c_void_p) if items else None, len(items), _stream_ptr(stream)),
                   "snail_instances_materials_update_dev")
        return info

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().snail_instances_materials_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _frame_args(cam, lights7, ambient):
        lights = np.ascontiguousarray(lights7 if lights7 is not None else np.zeros((0, 7)), dtype=np.float32).reshape(-1, 7)
        return lights, np.ascontiguousarray(cam.as_array13(), dtype=np.float32), np.ascontiguousarray(ambient, dtype=np.float32)

    def shade_packets(self, cam, resx: int, resy: int, packet_xy, hits, out=None, stream=None):
        """The samples of a packet list from its hit records (t, u, v, instance, tri_id: packet-major [n, 256] device tensors, as
        InstancedScene.trace_packets returns them) -> float32 [n, 9, 64, 4]: normal xyz, diffuse rgb, specular rgb per (quad, lane).
        snail_instances_materials_shade_packets_dev."""
        torch = _torch()
        n = int(packet_xy.shape[0])
        if out is None:
            out = torch.empty((n, SAMPLE_COMPONENTS, 64, 4), dtype=torch.float32, device=self.isc._dev())
        cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32)
        rc = _lib.lib().snail_instances_materials_shade_packets_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(packet_xy), n, _lib.ptr(hits[0]), _lib.ptr(hits[1]),
                                                                    _lib.ptr(hits[2]), _lib.ptr(hits[3]), _lib.ptr(hits[4]), _lib.ptr(out), _stream_ptr(stream))
        _lib.check(rc, "snail_instances_materials_shade_packets_dev")
        return out

    def mirror_packets(self, cam, resx: int, resy: int, packet_xy, t, samples, stats=None, stream=None):
        """Scene::TraceReflection on the primary samples of a packet list (t: the hits' distances [n, 256]; samples: shade_packets' buffer) ->
        (origin, dir, idir [n, 64, 3, 4] float32, mask [n, 64] uint8, distance [n, 256] float32, object, element [n, 256] int32, bary
        [n, 64, 2, 4] float32): the mirrored packets as InstancedScene.traverse_primary takes them in and out (object, element and bary zero).
        snail_instances_materials_mirror_packets_dev."""
        torch = _torch()
        n = int(packet_xy.shape[0])
        dev = self.isc._dev()
        org, d, idir = (torch.empty((n, 64, 3, 4), dtype=torch.float32, device=dev) for _ in range(3))
        mask = torch.empty((n, 64), dtype=torch.uint8, device=dev)
        dist = torch.empty((n, 256), dtype=torch.float32, device=dev)
        obj, elem = (torch.empty((n, 256), dtype=torch.int32, device=dev) for _ in range(2))
        bary = torch.empty((n, 64, 2, 4), dtype=torch.float32, device=dev)
        cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32)
        rc = _lib.lib().snail_instances_materials_mirror_packets_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(packet_xy), n, _lib.ptr(t), _lib.ptr(samples),
                                                                     _lib.ptr(org), _lib.ptr(d), _lib.ptr(idir), _lib.ptr(mask), _lib.ptr(dist), _lib.ptr(obj), _lib.ptr(elem),
                                                                     _lib.ptr(bary), _lib.ptr(stats), _stream_ptr(stream))
        _lib.check(rc, "snail_instances_materials_mirror_packets_dev")
        return org, d, idir, mask, dist, obj, elem, bary

    def shade_rays(self, dirs, mask, t, bary, inst, tri_id, out=None, stream=None):
        """The samples of generic packets (RayGroup<0, hasMask>): dirs [n, 64, 3, 4], mask [n, 64] uint8 or None (every lane selected), hit
        records t / inst / tri_id [n, 256] and bary [n, 64, 2, 4] (device tensors: the distance, object, element and bary of
        InstancedScene.traverse_primary) -> float32 [n, 9, 64, 4].  snail_instances_materials_shade_rays_dev."""
        torch = _torch()
        n = int(dirs.shape[0])
        if out is None:
            out = torch.empty((n, SAMPLE_COMPONENTS, 64, 4), dtype=torch.float32, device=self.isc._dev())
        rc = _lib.lib().snail_instances_materials_shade_rays_dev(self._h, n, _lib.ptr(dirs), _lib.ptr(mask), _lib.ptr(t), _lib.ptr(bary), _lib.ptr(inst), _lib.ptr(tri_id),
                                                                 _lib.ptr(out), _stream_ptr(stream))
        _lib.check(rc, "snail_instances_materials_shade_rays_dev")
        return out

    def render(self, cam, resx: int, resy: int, lights7=None, ambient=(0.1, 0.1, 0.1), out=None, stats=None, stream=None, flags: int = 0, reflections: bool = False):
        """The lit frame, [resy, resx, 3] uint8 (B,G,R) (or `out`: a uint8 device tensor [resy, pitch] / [resy, w, 3] whose rows may be wider).
        snail_instances_render_materials_dev; flags must be 0.  reflections=True: with the one mirrored bounce of gVals[7]
        (snail_instances_materials_bounce_dev; `flags` are then that function's)."""
        torch = _torch()
        if out is None:
            out = torch.zeros((resy, resx, 3), dtype=torch.uint8, device=self.isc._dev())
        lights, cam13, amb = self._frame_args(cam, lights7, ambient)
        if reflections:
            rc = _lib.lib().snail_instances_materials_bounce_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(lights) if len(lights) else None, len(lights), _lib.ptr(amb),
                                                                 int(flags) | RENDER_REFLECTIONS, _lib.ptr(out), int(out.stride(0)), _lib.ptr(stats), _stream_ptr(stream))
            _lib.check(rc, "snail_instances_materials_bounce_dev")
            return out
        rc = _lib.lib().snail_instances_render_materials_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(lights) if len(lights) else None, len(lights), _lib.ptr(amb),
                                                             int(flags), _lib.ptr(out), int(out.stride(0)), _lib.ptr(stats), _stream_ptr(stream))
        _lib.check(rc, "snail_instances_render_materials_dev")
        return out

    def render_packets(self, cam, resx: int, resy: int, packet_xy, lights7=None, ambient=(0.1, 0.1, 0.1), out=None, stats=None, stream=None, flags: int = 0,
                       reflections: bool = False):
        """render for an explicit packet list (int32 [n, 2] device tensor): packet-major [n, 256, 3] uint8 (B,G,R).
        snail_instances_render_materials_packets_dev.  reflections=True: snail_instances_materials_bounce_packets_dev."""
        torch = _torch()
        n = int(packet_xy.shape[0])
        if out is None:
            out = torch.empty((n, 256, 3), dtype=torch.uint8, device=self.isc._dev())
        lights, cam13, amb = self._frame_args(cam, lights7, ambient)
        if reflections:
            rc = _lib.lib().snail_instances_materials_bounce_packets_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(packet_xy), n, _lib.ptr(lights) if len(lights) else None,
                                                                         len(lights), _lib.ptr(amb), int(flags) | RENDER_REFLECTIONS, _lib.ptr(out), _lib.ptr(stats),
                                                                         _stream_ptr(stream))
            _lib.check(rc, "snail_instances_materials_bounce_packets_dev")
            return out
        rc = _lib.lib().snail_instances_render_materials_packets_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(packet_xy), n, _lib.ptr(lights) if len(lights) else None,
                                                                     len(lights), _lib.ptr(amb), int(flags), _lib.ptr(out), _lib.ptr(stats), _stream_ptr(stream))
        _lib.check(rc, "snail_instances_render_materials_packets_dev")
        return out

    def render_image_host(self, cam, resx: int, resy: int, lights7=None, ambient=(0.1, 0.1, 0.1), flags: int = 0, pitch: int | None = None, fill: int = 0,
                          reflections: bool = False):
        """snail_instances_render_materials_image: the frame in host memory, uint8 [resy, pitch] (pitch = 3 * resx unless given; bytes past a
        row's pixels keep `fill`), and the call's TreeStats.  reflections=True: snail_instances_materials_bounce_image."""
        pitch = resx * 3 if pitch is None else int(pitch)
        img = np.full((resy, pitch), fill, dtype=np.uint8)
        stats = np.zeros(4, dtype=np.uint64)
        lights, cam13, amb = self._frame_args(cam, lights7, ambient)
        if reflections:
            rc = _lib.lib().snail_instances_materials_bounce_image(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(lights) if len(lights) else None, len(lights), _lib.ptr(amb),
                                                                   int(flags) | RENDER_REFLECTIONS, _lib.ptr(img), pitch, _lib.ptr(stats))
            _lib.check(rc, "snail_instances_materials_bounce_image")
            return img, stats
        rc = _lib.lib().snail_instances_render_materials_image(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(lights) if len(lights) else None, len(lights), _lib.ptr(amb),
                                                               int(flags), _lib.ptr(img), pitch, _lib.ptr(stats))
        _lib.check(rc, "snail_instances_render_materials_image")
        return img, stats

    # ---- include/snail_instances_materials_transparency.h -----------------------------------------------------------------------------------
    @property
    def can_select_transparent(self) -> bool:
        """whether the set holds a material that can select a transparent lane (Material.transparent, or Material.uber with 0 < dissolve < 1):
        such a set is refused by every method above this block"""
        r = _lib.lib().snail_instances_materials_can_select_transparent(self._h)
        if r < 0:
            raise _lib.SnailError("snail_instances_materials_can_select_transparent: %s" % _lib.lib().snail_last_error().decode())
        return bool(r)

    def shade_packets_transp(self, cam, resx: int, resy: int, packet_xy, hits, stream=None):
        """shade_packets for any set, with Sample::opacity and the transparency selector -> (samples float32 [n, 9, 64, 4], opacity float32
        [n, 256], sel uint8 [n, 64]: low 4 bits = transSel after the opacity < 1 filter).  snail_instances_materials_shade_packets_transp_dev."""
        torch = _torch()
        n = int(packet_xy.shape[0])
        dev = self.isc._dev()
        out = torch.empty((n, SAMPLE_COMPONENTS, 64, 4), dtype=torch.float32, device=dev)
        opacity = torch.empty((n, 256), dtype=torch.float32, device=dev)
        sel = torch.empty((n, 64), dtype=torch.uint8, device=dev)
        cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32)
        rc = _lib.lib().snail_instances_materials_shade_packets_transp_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(packet_xy), n, _lib.ptr(hits[0]), _lib.ptr(hits[1]),
                                                                           _lib.ptr(hits[2]), _lib.ptr(hits[3]), _lib.ptr(hits[4]), _lib.ptr(out), _lib.ptr(opacity),
                                                                           _lib.ptr(sel), _stream_ptr(stream))
        _lib.check(rc, "snail_instances_materials_shade_packets_transp_dev")
        return out, opacity, sel

    def shade_rays_transp(self, dirs, mask, t, bary, inst, tri_id, stream=None):
        """shade_rays for any set -> (samples, opacity, sel) as shade_packets_transp.  snail_instances_materials_shade_rays_transp_dev."""
        torch = _torch()
        n = int(dirs.shape[0])
        dev = self.isc._dev()
        out = torch.empty((n, SAMPLE_COMPONENTS, 64, 4), dtype=torch.float32, device=dev)
        opacity = torch.empty((n, 256), dtype=torch.float32, device=dev)
        sel = torch.empty((n, 64), dtype=torch.uint8, device=dev)
        rc = _lib.lib().snail_instances_materials_shade_rays_transp_dev(self._h, n, _lib.ptr(dirs), _lib.ptr(mask), _lib.ptr(t), _lib.ptr(bary), _lib.ptr(inst),
                                                                        _lib.ptr(tri_id), _lib.ptr(out), _lib.ptr(opacity), _lib.ptr(sel), _stream_ptr(stream))
        _lib.check(rc, "snail_instances_materials_shade_rays_transp_dev")
        return out, opacity, sel

    def continue_packets(self, t, sel, cam=None, resx: int = 0, resy: int = 0, packet_xy=None, rays=None, stats=None, stream=None):
        """Scene::TraceTransparency's packets of one level from its hits t [n, 256] and selector sel [n, 64] (device tensors).  The level's rays:
        cam / resx / resy / packet_xy (the primary level) or rays = (origin, dir, idir) [n, 64, 3, 4] (generic packets) ->
        (origin, dir, idir [n, 64, 3, 4] float32, mask [n, 64] uint8, distance [n, 256] float32, object, element [n, 256] int32 (zeros), bary
        [n, 64, 2, 4] float32 (zeros), order [n] int32: the packet's index, or -1 when none of its lanes is selected): the packets as
        InstancedScene.traverse_primary takes them in and out.  snail_instances_materials_continue_packets_dev."""
        torch = _torch()
        n = int(t.shape[0])
        dev = self.isc._dev()
        org, d, idir = (torch.empty((n, 64, 3, 4), dtype=torch.float32, device=dev) for _ in range(3))
        mask = torch.empty((n, 64), dtype=torch.uint8, device=dev)
        dist = torch.empty((n, 256), dtype=torch.float32, device=dev)
        obj, elem = (torch.empty((n, 256), dtype=torch.int32, device=dev) for _ in range(2))
        bary = torch.empty((n, 64, 2, 4), dtype=torch.float32, device=dev)
        order = torch.empty((n,), dtype=torch.int32, device=dev)
        cam13 = None if cam is None else np.ascontiguousarray(cam.as_array13(), dtype=np.float32)
        ro, rd, ri = rays if rays is not None else (None, None, None)
        rc = _lib.lib().snail_instances_materials_continue_packets_dev(self._h, _lib.ptr(cam13), int(resx), int(resy), _lib.ptr(packet_xy), n, _lib.ptr(ro), _lib.ptr(rd),
                                                                       _lib.ptr(ri), _lib.ptr(t), _lib.ptr(sel), _lib.ptr(org), _lib.ptr(d), _lib.ptr(idir), _lib.ptr(mask),
                                                                       _lib.ptr(dist), _lib.ptr(obj), _lib.ptr(elem), _lib.ptr(bary), _lib.ptr(order), _lib.ptr(stats),
                                                                       _stream_ptr(stream))
        _lib.check(rc, "snail_instances_materials_continue_packets_dev")
        return org, d, idir, mask, dist, obj, elem, bary, order

    def _truncated(self, truncated):
        return truncated if truncated is not None else _torch().zeros(1, dtype=_torch().int64, device=self.isc._dev())

    def render_transparent(self, cam, resx: int, resy: int, lights7=None, ambient=(0.1, 0.1, 0.1), out=None, stats=None, stream=None, flags: int = 0,
                           max_depth: int = 8, truncated=None):
        """The lit frame with the transparency continuation, at most max_depth levels deep -> (frame [resy, resx, 3] uint8 (B,G,R) or `out`,
        truncated: an int64 device tensor of one word, += the lanes level max_depth would still select; 0 = the frame is the reference's).
        snail_instances_materials_transparent_dev."""
        torch = _torch()
        if out is None:
            out = torch.zeros((resy, resx, 3), dtype=torch.uint8, device=self.isc._dev())
        truncated = self._truncated(truncated)
        lights, cam13, amb = self._frame_args(cam, lights7, ambient)
        rc = _lib.lib().snail_instances_materials_transparent_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(lights) if len(lights) else None, len(lights), _lib.ptr(amb),
                                                                  int(flags), _lib.ptr(out), int(out.stride(0)), int(max_depth), _lib.ptr(truncated), _lib.ptr(stats),
                                                                  _stream_ptr(stream))
        _lib.check(rc, "snail_instances_materials_transparent_dev")
        return out, truncated

    def render_transparent_packets(self, cam, resx: int, resy: int, packet_xy, lights7=None, ambient=(0.1, 0.1, 0.1), out=None, stats=None, stream=None,
                                   flags: int = 0, max_depth: int = 8, truncated=None):
        """render_transparent for an explicit packet list -> (packet-major [n, 256, 3] uint8 (B,G,R), truncated).
        snail_instances_materials_transparent_packets_dev."""
        torch = _torch()
        n = int(packet_xy.shape[0])
        if out is None:
            out = torch.empty((n, 256, 3), dtype=torch.uint8, device=self.isc._dev())
        truncated = self._truncated(truncated)
        lights, cam13, amb = self._frame_args(cam, lights7, ambient)
        rc = _lib.lib().snail_instances_materials_transparent_packets_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(packet_xy), n,
                                                                          _lib.ptr(lights) if len(lights) else None, len(lights), _lib.ptr(amb), int(flags), _lib.ptr(out),
                                                                          int(max_depth), _lib.ptr(truncated), _lib.ptr(stats), _stream_ptr(stream))
        _lib.check(rc, "snail_instances_materials_transparent_packets_dev")
        return out, truncated

    def render_transparent_image_host(self, cam, resx: int, resy: int, lights7=None, ambient=(0.1, 0.1, 0.1), flags: int = 0, pitch: int | None = None, fill: int = 0,
                                      max_depth: int = 8, truncated=None):
        """snail_instances_materials_transparent_image: the frame in host memory -> (uint8 [resy, pitch], stats uint64 [4], truncated: uint64
        [1], the caller's array (+=) or a new one)"""
        pitch = resx * 3 if pitch is None else int(pitch)
        img = np.full((resy, pitch), fill, dtype=np.uint8)
        stats = np.zeros(4, dtype=np.uint64)
        truncated = np.zeros(1, dtype=np.uint64) if truncated is None else truncated
        lights, cam13, amb = self._frame_args(cam, lights7, ambient)
        rc = _lib.lib().snail_instances_materials_transparent_image(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(lights) if len(lights) else None, len(lights),
                                                                    _lib.ptr(amb), int(flags), _lib.ptr(img), pitch, int(max_depth), _lib.ptr(truncated), _lib.ptr(stats))
        _lib.check(rc, "snail_instances_materials_transparent_image")
        return img, stats, truncated

    # ---- include/snail_instances_materials_tree.h: the continuation together with the bounce, tile lists, 4x AA, depth shading and the tint; any set ----
    def _tile_args(self, cam, lights7, ambient, tint):
        lights, cam13, amb = self._frame_args(cam, lights7, ambient)
        tnt = None if tint is None else np.ascontiguousarray(tint, dtype=np.float32).reshape(3)
        return lights, (_lib.ptr(lights) if len(lights) else None), cam13, amb, tnt

    def mirror_rays(self, origin, dirs, mask, t, samples, order_in=None, out=None, stats=None, stream=None):
        """Scene::TraceReflection from a level's generic packets: origin / dirs [n, 64, 3, 4], mask [n, 64] uint8 or None (every lane selected),
        t [n, 256], the level's samples [n, 9, 64, 4] (device tensors); order_in [n] int32 or None: the level's own order list ->
        (origin, dir, idir [n, 64, 3, 4] float32, mask [n, 64] uint8, distance [n, 256] float32, object, element [n, 256] int32 (zeros), bary
        [n, 64, 2, 4] float32 (zeros), order [n] int32): the mirrored packets as InstancedScene.traverse_primary takes them in and out, or the
        nine tensors of `out` written in place: a packet whose order_in word is negative gets order -1 and nothing else.
        snail_instances_materials_mirror_rays_dev."""
        torch = _torch()
        n = int(dirs.shape[0])
        dev = self.isc._dev()
        if out is None:
            out = tuple(torch.empty((n, 64, 3, 4), dtype=torch.float32, device=dev) for _ in range(3)) + (
                torch.empty((n, 64), dtype=torch.uint8, device=dev), torch.empty((n, 256), dtype=torch.float32, device=dev),
                torch.empty((n, 256), dtype=torch.int32, device=dev), torch.empty((n, 256), dtype=torch.int32, device=dev),
                torch.empty((n, 64, 2, 4), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev))
        org, d, idir, msk, dist, obj, elem, bary, order = out
        rc = _lib.lib().snail_instances_materials_mirror_rays_dev(self._h, n, _lib.ptr(origin), _lib.ptr(dirs), _lib.ptr(mask), _lib.ptr(t), _lib.ptr(samples),
                                                                  _lib.ptr(order_in), _lib.ptr(org), _lib.ptr(d), _lib.ptr(idir), _lib.ptr(msk), _lib.ptr(dist), _lib.ptr(obj),
                                                                  _lib.ptr(elem), _lib.ptr(bary), _lib.ptr(order), _lib.ptr(stats), _stream_ptr(stream))
        _lib.check(rc, "snail_instances_materials_mirror_rays_dev")
        return out

    def tree_frame_packets(self, cam, resx: int, resy: int, packet_xy, lights7=None, flags: int = 0, tint=None, ambient=(0.1, 0.1, 0.1), out=None, stats=None,
                           stream=None, max_depth: int = 8, truncated=None):
        """The lit packets of an explicit packet list for any set, with the transparency continuation at most max_depth levels deep under any
        of RENDER_REFLECTIONS / RENDER_DEPTH / RENDER_AA4 and the tint -> (packet-major [n, 256, 3] uint8 (B,G,R), truncated: int64 device
        tensor of one word, +=).  snail_instances_materials_tree_frame_packets_dev."""
        torch = _torch()
        n = int(packet_xy.shape[0])
        if out is None:
            out = torch.empty((n, 256, 3), dtype=torch.uint8, device=self.isc._dev())
        truncated = self._truncated(truncated)
        lights, lp, cam13, amb, tnt = self._tile_args(cam, lights7, ambient, tint)
        rc = _lib.lib().snail_instances_materials_tree_frame_packets_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(packet_xy), n, lp, len(lights), _lib.ptr(amb),
                                                                         int(flags), _lib.ptr(tnt), _lib.ptr(out), int(max_depth), _lib.ptr(truncated), _lib.ptr(stats),
                                                                         _stream_ptr(stream))
        _lib.check(rc, "snail_instances_materials_tree_frame_packets_dev")
        return out, truncated

    def render_tree_tiles_host(self, cam, resx: int, resy: int, tiles, offsets=None, lights7=None, flags: int = 0, tint=None, ambient=(0.1, 0.1, 0.1), data=None,
                               max_depth: int = 8, truncated=None):
        """The tile list (tiles: int32 [n, 4] = x, y, w, h; per tile the planes R, G-R, B-R at offsets[k] of data) for any set ->
        (data, offsets, stats, truncated: uint64 [1], the caller's array (+=) or a new one).  snail_instances_materials_tree_render_tiles."""
        t = np.ascontiguousarray(tiles, dtype=np.int32).reshape(-1, 4)
        size = 3 * t[:, 2].astype(np.int64) * t[:, 3]
        if offsets is None:
            offsets = np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.int64)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if data is None:
            data = np.zeros(int((offsets + size).max()) if len(t) else 0, dtype=np.uint8)
        lights, lp, cam13, amb, tnt = self._tile_args(cam, lights7, ambient, tint)
        stats = np.zeros(4, dtype=np.uint64)
        truncated = np.zeros(1, dtype=np.uint64) if truncated is None else truncated
        rc = _lib.lib().snail_instances_materials_tree_render_tiles(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(t), _lib.ptr(offsets), len(t), lp, len(lights),
                                                                    _lib.ptr(amb), int(flags), _lib.ptr(tnt), _lib.ptr(data), int(max_depth), _lib.ptr(truncated),
                                                                    _lib.ptr(stats))
        _lib.check(rc, "snail_instances_materials_tree_render_tiles")
        return data, offsets, stats, truncated

    def render_tree_frame_host(self, cam, resx: int, resy: int, lights7=None, flags: int = 0, ambient=(0.1, 0.1, 0.1), pitch: int | None = None, fill: int = 0,
                               max_depth: int = 8, truncated=None):
        """The frame in host memory for any set -> (uint8 [resy, pitch], stats, truncated: uint64 [1]).
        snail_instances_materials_tree_render_frame."""
        pitch = resx * 3 if pitch is None else int(pitch)
        img = np.full((resy, pitch), fill, dtype=np.uint8)
        stats = np.zeros(4, dtype=np.uint64)
        truncated = np.zeros(1, dtype=np.uint64) if truncated is None else truncated
        lights, lp, cam13, amb, _ = self._tile_args(cam, lights7, ambient, None)
        rc = _lib.lib().snail_instances_materials_tree_render_frame(self._h, _lib.ptr(cam13), resx, resy, lp, len(lights), _lib.ptr(amb), int(flags), _lib.ptr(img), pitch,
                                                                    int(max_depth), _lib.ptr(truncated), _lib.ptr(stats))
        _lib.check(rc, "snail_instances_materials_tree_render_frame")
        return img, stats, truncated

    def set_level_budget(self, nbytes: int):
        """snail_instances_materials_set_level_budget: the bytes the levels of one group of intermediates may take; a call clamps it up to one
        output packet's worth and runs its packet list in slices that stay within it"""
        _lib.check(_lib.lib().snail_instances_materials_set_level_budget(self._h, int(nbytes)), "snail_instances_materials_set_level_budget")

    @staticmethod
    def level_bytes(n_lights: int, flags: int = 0, max_depth: int = 8) -> int:
        """snail_instances_materials_level_bytes: the bytes of the levels of ONE output packet"""
        b = _lib.lib().snail_instances_materials_level_bytes(int(n_lights), int(flags), int(max_depth))
        if b < 0:
            raise _lib.SnailError("snail_instances_materials_level_bytes: %s" % _lib.lib().snail_last_error().decode())
        return int(b)

    # ---- include/snail_instances_materials_heatmap.h: per-packet TreeStats and the gVals[5] heat-map under full shading; any set ----
    def packet_stats(self, cam, resx: int, resy: int, packet_xy=None, lights7=None, reflections: bool = False, out=None, stats=None, stream=None, flags: int = 0,
                     max_depth: int = 8, truncated=None):
        """snail_instances_materials_packet_stats_dev: the TreeStats {intersects, iterations, rays, skips} of every packet's RayTrace call
        under full shading -- the whole tree of nested calls -- -> (int32 device tensor [n, 4] holding uint32 words, truncated: int64 device
        tensor of one word, +=).  packet_xy = int32 device tensor [n, 2], or None = the frame's grid, row-major."""
        torch = _torch()
        n = int(packet_xy.shape[0]) if packet_xy is not None else ((resx + 15) // 16) * ((resy + 15) // 16)
        if out is None:
            out = torch.zeros((n, 4), dtype=torch.int32, device=self.isc._dev())
        truncated = self._truncated(truncated)
        lights, lp, cam13, _, _ = self._tile_args(cam, lights7, (0.0, 0.0, 0.0), None)
        rc = _lib.lib().snail_instances_materials_packet_stats_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(packet_xy), n, lp, len(lights),
                                                                   int(flags) | (RENDER_REFLECTIONS if reflections else 0), int(max_depth), _lib.ptr(out),
                                                                   _lib.ptr(truncated), _lib.ptr(stats), _stream_ptr(stream))
        _lib.check(rc, "snail_instances_materials_packet_stats_dev")
        return out, truncated

    def render_heat_packets(self, cam, resx: int, resy: int, packet_xy=None, lights7=None, flags: int = 0, tint=None, out=None, packet_stats=None, stats=None,
                            stream=None, max_depth: int = 8, truncated=None):
        """snail_instances_materials_heat_packets_dev: the heat-map of the packets -> (packet-major [n, 256, 3] uint8 (B,G,R), truncated).
        flags: RENDER_REFLECTIONS, RENDER_AA4; tint = three factors (gVals[8]) or None; packet_stats (optional) int32 device tensor [n, 4]
        ([n, 4, 4] with RENDER_AA4)."""
        torch = _torch()
        n = int(packet_xy.shape[0]) if packet_xy is not None else ((resx + 15) // 16) * ((resy + 15) // 16)
        if out is None:
            out = torch.empty((n, 256, 3), dtype=torch.uint8, device=self.isc._dev())
        truncated = self._truncated(truncated)
        lights, lp, cam13, _, tnt = self._tile_args(cam, lights7, (0.0, 0.0, 0.0), tint)
        rc = _lib.lib().snail_instances_materials_heat_packets_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(packet_xy), n, lp, len(lights), int(flags),
                                                                   _lib.ptr(tnt), _lib.ptr(out), _lib.ptr(packet_stats), int(max_depth), _lib.ptr(truncated),
                                                                   _lib.ptr(stats), _stream_ptr(stream))
        _lib.check(rc, "snail_instances_materials_heat_packets_dev")
        return out, truncated

    def render_heat_tiles_host(self, cam, resx: int, resy: int, tiles, offsets=None, lights7=None, flags: int = 0, tint=None, data=None, max_depth: int = 8,
                               truncated=None):
        """snail_instances_materials_render_heat_tiles: render_tree_tiles_host with gVals[5] -> (data, offsets, stats, truncated: uint64 [1],
        the caller's array (+=) or a new one)."""
        t = np.ascontiguousarray(tiles, dtype=np.int32).reshape(-1, 4)
        size = 3 * t[:, 2].astype(np.int64) * t[:, 3]
        if offsets is None:
            offsets = np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.int64)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if data is None:
            data = np.zeros(int((offsets + size).max()) if len(t) else 0, dtype=np.uint8)
        lights, lp, cam13, _, tnt = self._tile_args(cam, lights7, (0.0, 0.0, 0.0), tint)
        stats = np.zeros(4, dtype=np.uint64)
        truncated = np.zeros(1, dtype=np.uint64) if truncated is None else truncated
        rc = _lib.lib().snail_instances_materials_render_heat_tiles(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(t), _lib.ptr(offsets), len(t), lp, len(lights),
                                                                    int(flags), _lib.ptr(tnt), _lib.ptr(data), int(max_depth), _lib.ptr(truncated), _lib.ptr(stats))
        _lib.check(rc, "snail_instances_materials_render_heat_tiles")
        return data, offsets, stats, truncated

    def render_heat_frame_host(self, cam, resx: int, resy: int, lights7=None, flags: int = 0, pitch: int | None = None, fill: int = 0, max_depth: int = 8,
                               truncated=None):
        """snail_instances_materials_render_heat_frame: render_tree_frame_host with gVals[5] -> (uint8 [resy, pitch] (B,G,R rows; pitch =
        3 * resx unless given, bytes past a row's pixels keep `fill`), stats, truncated: uint64 [1])."""
        pitch = resx * 3 if pitch is None else int(pitch)
        img = np.full((resy, max(pitch, 0)), fill, dtype=np.uint8)
        stats = np.zeros(4, dtype=np.uint64)
        truncated = np.zeros(1, dtype=np.uint64) if truncated is None else truncated
        lights, lp, cam13, _, _ = self._tile_args(cam, lights7, (0.0, 0.0, 0.0), None)
        rc = _lib.lib().snail_instances_materials_render_heat_frame(self._h, _lib.ptr(cam13), resx, resy, lp, len(lights), int(flags), _lib.ptr(img), pitch,
                                                                    int(max_depth), _lib.ptr(truncated), _lib.ptr(stats))
        _lib.check(rc, "snail_instances_materials_render_heat_frame")
        return img, stats, truncated


__all__ = ["InstancedMaterialSet", "DevBlasShading", "create_instanced_set"]
