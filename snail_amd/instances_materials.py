"""Full shading of instanced scenes: per-BLAS ShTriangle records and material maps, ONE scene-wide material and texture list, over the C-ABI
of include/snail_instances_materials.h.

  InstancedMaterialSet(isc, per_blas, materials, textures)   <-> DBVH::GetSElement (the BLAS's ShTriangle through ShTriangle::Transform) and
                                                                 DBVH::GetMaterialId over Scene::materials
  .shade_packets / .render / .render_packets / .render_image_host   <-> Scene<DBVH>::RayTrace with gVals[6] and HasShadingData() = 1 (this
                                                                 project's completion of the reference's TODO), primary packets and their lights
  .mirror_packets / .shade_rays, reflections=True           <-> the one mirrored bounce of gVals[7] (Scene::TraceReflection and its nested
                                                                 RayTrace<0, hasMask>), include/snail_instances_materials_bounce.h

Materials, textures and pack_shtris are snail_amd.materials'."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .instances import InstancedScene
from .materials import RENDER_REFLECTIONS, SAMPLE_COMPONENTS, _material_records, _texture_array, pack_shtris
from .scene import _stream_ptr, _torch


class _BlasShading(C.Structure):
    _fields_ = [("shtris64", C.c_void_p), ("nTris", C.c_int32), ("matMap", C.c_void_p), ("nMap", C.c_int32)]


def create_instanced_set(instances_handle, shtris_list, map_list, materials, textures):
    """snail_instances_materials_create over raw arguments (per BLAS: uint8 [n, 64] records, int32 map) -> handle (c_void_p); SnailError with
    the library's text when the set is refused"""
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
    h = _lib.lib().snail_instances_materials_create(instances_handle, C.cast(per, C.c_void_p) if len(sh) else None, len(sh), _lib.ptr(recs) if len(recs) else None,
                                                    len(recs), C.cast(tex, C.c_void_p) if len(textures) else None, len(textures))
    if not h:
        raise _lib.SnailError("snail_instances_materials_create: %s" % _lib.lib().snail_last_error().decode())
    return C.c_void_p(h)


class InstancedMaterialSet:
    """The shading data of an instanced scene on its GPU.  per_blas[b] = (uv, nrm, mat_index, flat, material_map) of BLAS b's INPUT triangles
    (the order that scene was built from; its bvh.perm permutes them into triId order); a map entry is -1 (the default material) or an index
    into `materials`, ONE list for all BLASes.  The instanced scene (and through it the BLAS scenes) is kept alive by this object.  The
    instance records are read at every launch: after isc.update / update_dev the same set shades with the new rotations."""

    def __init__(self, isc: InstancedScene, per_blas, materials=(), textures=()):
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
        self._h = create_instanced_set(isc._h, self.shtris, maps, list(materials), list(textures))

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


__all__ = ["InstancedMaterialSet", "create_instanced_set"]
