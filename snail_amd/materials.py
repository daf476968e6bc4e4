"""Full shading of plain scenes: the host-side mirror of the reference's shading data -- ShTriangle records, shading::Material objects
and MipmapTexture / PointSampler -- over the C-ABI of include/snail_materials.h.

  Texture(level0)                                   <-> MipmapTexture(image, rgb8) + GenMips, sampled by sampling::PointSampler
  Material.simple / .textured / .uber               <-> SimpleMaterial<NDotR>, TexMaterial<NDotR>, UberMaterial(MaterialDesc)
  pack_shtris(uv, nrm, mat_index, flat, perm)       <-> the ShTriangle constructor + the builder's permutation of shTris
  MaterialSet(scene, uv, nrm, mat_index, flat, material_map, materials, textures)   <-> BVH::shTris / BVH::materials + Scene::materials
  .shade_packets / .render / .render_packets / .render_image_host   <-> Scene::RayTrace with gVals[6] && HasShadingData(), primary packets

  .mirror_packets / .shade_rays, reflections=True   <-> the one mirrored bounce of gVals[7] (Scene::TraceReflection and its nested
                                                        RayTrace<0, hasMask>), include/snail_materials_bounce.h

  .frame_packets / .render_tiles_host / .render_frame_host   <-> RenderTask::Work around those frames: tile lists with the planar store,
                                                        4x AA (gVals[9]), depth shading (gVals[1]) and the tint (gVals[8]),
                                                        include/snail_materials_tiles.h

  Material.transparent, MaterialSet(..., transparent=True), .can_select_transparent, .shade_packets_transp / .shade_rays_transp /
  .continue_packets, .render_transparent / .render_transparent_packets / .render_transparent_image_host
                                                    <-> TransparentMaterial<NDotR> / UberMaterial's dissFactor, Sample::opacity, the transSel
                                                        selector, Scene::TraceTransparency and its nested RayTrace calls, level by level,
                                                        include/snail_materials_transparency.h

  MaterialSet.from_dev(scene, d_uv, d_mat_index, ...), .rebuild_dev / .update_dev
                                                    <-> the builder permuting shTris together with tris (src/bvh/tree.cpp:122-125, :249-252) for a
                                                        mesh that deforms: records packed on the device behind every device rebuild,
                                                        include/snail_materials_dynamic.h

  .mirror_rays / .tree_frame_packets / .render_tree_tiles_host / .render_tree_frame_host / .set_level_budget / .level_bytes
                                                    <-> the continuation TOGETHER with the bounce (every RayTrace of the continuation chain
                                                        mirrors its hit lanes; the mirrored call continues but never mirrors), tile lists,
                                                        4x AA, depth shading and the tint, include/snail_materials_tree.h

Out of this module (the host renderer keeps them): OBJ / MTL ingest."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .scene import Scene, _stream_ptr, _torch

KIND_SIMPLE, KIND_TEX, KIND_UBER, KIND_TRANSPARENT = 0, 1, 2, 3
MATERIAL_DTYPE = np.dtype([("kind", "<i4"), ("ndotr", "<i4"), ("diffuse", "<f4", 3), ("specular", "<f4", 3), ("dissolve", "<f4"), ("texture", "<i4")])
assert MATERIAL_DTYPE.itemsize == 40
SAMPLE_COMPONENTS = 9        # normal, diffuse, specular
RENDER_REFLECTIONS = 1       # SNAIL_RENDER_REFLECTIONS (include/snail_hip.h)
RENDER_DEPTH = 2             # SNAIL_RENDER_DEPTH
RENDER_AA4 = 4               # SNAIL_RENDER_AA4


def texture_size(w: int, h: int):
    """(bytes of the mip chain, levels); SnailError for a shape that is refused"""
    n = C.c_int(0)
    b = _lib.lib().snail_texture_size(int(w), int(h), C.addressof(n))
    if b <= 0:
        raise _lib.SnailError("texture %d x %d: width and height must be powers of two of at most 8192" % (w, h))
    return int(b), n.value


class Texture:
    """An rgb8 texture with its mip chain (snail_texture_build): level0 = uint8 [h, w, 3] in the byte order the sampler reads (byte 0 -> red)."""

    def __init__(self, level0):
        a = np.ascontiguousarray(level0, dtype=np.uint8)
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("level0 must be uint8 [h, w, 3]")
        self.height, self.width = int(a.shape[0]), int(a.shape[1])
        size, _ = texture_size(self.width, self.height)
        self.levels = np.zeros(size, dtype=np.uint8)
        n = C.c_int(0)
        _lib.check(_lib.lib().snail_texture_build(_lib.ptr(a), self.width, self.height, _lib.ptr(self.levels), size, C.addressof(n)), "snail_texture_build")
        self.n_levels = n.value


class Material:
    """One record of MATERIAL_DTYPE."""

    def __init__(self, kind, ndotr=True, diffuse=(1.0, 1.0, 1.0), specular=(0.0, 0.0, 0.0), dissolve=0.0, texture=0, opacity_texture=0):
        self.opacity_texture = int(opacity_texture)      # read for KIND_TRANSPARENT only (snail_materials_create_transparent's opacityTexture)
        self.rec = np.zeros((), dtype=MATERIAL_DTYPE)
        self.rec["kind"], self.rec["ndotr"], self.rec["diffuse"], self.rec["specular"] = int(kind), 1 if ndotr else 0, diffuse, specular
        self.rec["dissolve"], self.rec["texture"] = dissolve, int(texture)

    @classmethod
    def simple(cls, color, ndotr: bool = True):
        return cls(KIND_SIMPLE, ndotr, diffuse=color)

    @classmethod
    def textured(cls, texture_index: int, ndotr: bool = True):
        return cls(KIND_TEX, ndotr, texture=texture_index)

    @classmethod
    def uber(cls, diffuse, specular, dissolve: float = 0.0):
        """MaterialDesc's diffuse / specular / dissolveFactor (the constructor's swap of diffuse.x and .z happens in the library)"""
        return cls(KIND_UBER, True, diffuse=diffuse, specular=specular, dissolve=dissolve)

    @classmethod
    def transparent(cls, texture: int = 0, opacity_texture: int = 0, ndotr: bool = True):
        """TransparentMaterial<NDotR>: `texture` is the colour map, `opacity_texture` the opacity map (its first channel is the opacity).
        Accepted by MaterialSet(..., transparent=True) alone; the plain creator refuses the kind."""
        return cls(KIND_TRANSPARENT, ndotr, texture=texture, opacity_texture=opacity_texture)


def pack_shtris(uv, nrm, mat_index, flat=None, perm=None) -> np.ndarray:
    """snail_shtris_pack: uv [n, 3, 2], nrm [n, 3, 3], mat_index [n], flat [n] of the INPUT triangles -> uint8 [n, 64] records in triId order
    (perm = BVH slot -> input triangle, e.g. HostBVH.perm)."""
    uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 6)
    nr = np.ascontiguousarray(nrm, dtype=np.float32).reshape(-1, 9)
    mi = np.ascontiguousarray(mat_index, dtype=np.int32).reshape(-1)
    n = len(uv)
    fl = np.zeros(n, dtype=np.uint8) if flat is None else np.ascontiguousarray(np.asarray(flat).astype(bool), dtype=np.uint8).reshape(-1)
    pm = None if perm is None else np.ascontiguousarray(perm, dtype=np.int32).reshape(-1)
    if len(nr) != n or len(mi) != n or len(fl) != n or (pm is not None and len(pm) != n):
        raise ValueError("uv, nrm, mat_index, flat and perm must hold one entry per triangle")
    out = np.zeros((n, 64), dtype=np.uint8)
    _lib.check(_lib.lib().snail_shtris_pack(_lib.ptr(uv), _lib.ptr(nr), _lib.ptr(mi), _lib.ptr(fl), n, _lib.ptr(pm), _lib.ptr(out)), "snail_shtris_pack")
    return out


def _material_records(materials) -> np.ndarray:
    recs = np.zeros(len(materials), dtype=MATERIAL_DTYPE)
    for k, m in enumerate(materials):
        recs[k] = m.rec
    return recs


class _Tex(C.Structure):
    _fields_ = [("levels", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32)]


def _texture_array(textures):
    tex = (_Tex * max(len(textures), 1))()
    for k, t in enumerate(textures):
        tex[k].levels, tex[k].width, tex[k].height = t.levels.ctypes.data, t.width, t.height
    return tex


def create_set(scene_handle, shtris, material_map, materials, textures, transparent: bool = False):
    """snail_materials_create (transparent=True: snail_materials_create_transparent) over raw arguments -> handle (c_void_p); SnailError with
    the library's text when the set is refused"""
    sh = np.ascontiguousarray(shtris, dtype=np.uint8).reshape(-1, 64)
    mp = np.ascontiguousarray(material_map, dtype=np.int32).reshape(-1)
    recs = _material_records(materials)
    tex = _texture_array(textures)
    if transparent:
        op = np.ascontiguousarray([getattr(m, "opacity_texture", 0) for m in materials], dtype=np.int32)
        h = _lib.lib().snail_materials_create_transparent(scene_handle, _lib.ptr(sh), len(sh), _lib.ptr(mp), len(mp), _lib.ptr(recs) if len(recs) else None, len(recs),
                                                          _lib.ptr(op) if len(op) else None, C.cast(tex, C.c_void_p) if len(textures) else None, len(textures))
    else:
        h = _lib.lib().snail_materials_create(scene_handle, _lib.ptr(sh), len(sh), _lib.ptr(mp), len(mp), _lib.ptr(recs) if len(recs) else None, len(recs),
                                              C.cast(tex, C.c_void_p) if len(textures) else None, len(textures))
    if not h:
        raise _lib.SnailError("%s: %s" % ("snail_materials_create_transparent" if transparent else "snail_materials_create", _lib.lib().snail_last_error().decode()))
    return C.c_void_p(h)


def create_set_dev(scene_handle, d_uv, d_mat_index, d_flat, n, d_perm, d_nrm, d_verts, material_map, materials, textures, transparent: bool = False, stream=None):
    """snail_materials_create_dev over raw arguments (device tensors or None) -> handle (c_void_p); SnailError with the library's text when
    the set is refused"""
    mp = np.ascontiguousarray(material_map, dtype=np.int32).reshape(-1)
    recs = _material_records(materials)
    tex = _texture_array(textures)
    op = np.ascontiguousarray([getattr(m, "opacity_texture", 0) for m in materials] or [0], dtype=np.int32) if transparent else None
    h = _lib.lib().snail_materials_create_dev(scene_handle, _lib.ptr(d_uv), _lib.ptr(d_mat_index), _lib.ptr(d_flat), int(n), _lib.ptr(d_perm), _lib.ptr(d_nrm),
                                              _lib.ptr(d_verts), _lib.ptr(mp), len(mp), _lib.ptr(recs) if len(recs) else None, len(recs), _lib.ptr(op),
                                              C.cast(tex, C.c_void_p) if len(textures) else None, len(textures), _stream_ptr(stream))
    if not h:
        raise _lib.SnailError("snail_materials_create_dev: %s" % _lib.lib().snail_last_error().decode())
    return C.c_void_p(h)


class MaterialSet:
    """The shading data of a plain scene on its GPU.  uv / nrm / mat_index / flat describe the INPUT triangles (the order the scene was built
    from; scene.bvh.perm permutes them into triId order); material_map[i] = -1 (the default material) or an index into `materials`.
    The scene is kept alive by this object.

    The records are permuted ONCE, by the tree the scene holds now, so the scene must have been built from host triangles (Scene(HostBVH),
    Scene.from_fast, Scene.from_lbvh).  A scene whose tree is built or rebuilt on the device (Scene.from_fast_dev / rebuild_fast_dev) is
    refused: a rebuild renumbers the triangles, and a set made before it would shade every hit with another triangle's data."""

    def __init__(self, scene: Scene, uv, nrm, mat_index, flat=None, material_map=(-1,), materials=(), textures=(), transparent: bool = False):
        self.scene = scene
        self._h = None
        if getattr(scene, "_fast_dev", False):
            raise _lib.SnailError("MaterialSet: the scene's tree is built on the device (from_fast_dev) and may be rebuilt there, which renumbers "
                                  "the triangles; build the scene from host triangles (Scene(HostBVH.build(..)), Scene.from_fast, Scene.from_lbvh)")
        perm = getattr(scene.bvh, "perm", None)
        if perm is None:
            raise _lib.SnailError("MaterialSet: the scene carries no permutation (BVH slot -> input triangle), so its shading data cannot be put into triId order")
        self.shtris = pack_shtris(uv, nrm, mat_index, flat, perm)
        self._h = create_set(scene._h, self.shtris, material_map, list(materials), list(textures), transparent)

    # ---- include/snail_materials_dynamic.h: the set of a deforming mesh ------------------------------------------------------------------
    @classmethod
    def from_dev(cls, scene: Scene, d_uv, d_mat_index, d_flat=None, material_map=(-1,), materials=(), textures=(), transparent: bool = False, d_nrm=None,
                 d_verts=None, stream=None):
        """The set of a Scene.from_fast_dev scene, its records packed on the device through scene.d_perm (snail_materials_create_dev) and
        packed again by rebuild_dev / update_dev.  Device tensors on the scene's device, describing the INPUT triangles: d_uv float32
        [n, 3, 2], d_mat_index int32 [n], d_flat uint8 [n] or None (none flat); normals d_nrm float32 [n, 3, 3], or None for face normals of
        d_verts float32 [n, 3, 3].  The tensors are copied: they need not outlive the call."""
        if not getattr(scene, "_fast_dev", False):
            raise _lib.SnailError("MaterialSet.from_dev: the scene was not made by Scene.from_fast_dev (MaterialSet(...) serves a tree that is never rebuilt)")
        torch = _torch()
        n = scene._fast_n
        d = scene._dev()
        cls._check_dev("d_uv", d_uv, torch.float32, n * 6, d)
        cls._check_dev("d_mat_index", d_mat_index, torch.int32, n, d)
        cls._check_dev("d_flat", d_flat, torch.uint8, n, d, optional=True)
        cls._check_dev("d_nrm", d_nrm, torch.float32, n * 9, d, optional=True)
        cls._check_dev("d_verts", d_verts, torch.float32, n * 9, d, optional=True)
        self = cls.__new__(cls)
        self.scene, self._h, self.shtris = scene, None, None
        self._h = create_set_dev(scene._h, d_uv, d_mat_index, d_flat, n, scene.d_perm, d_nrm, d_verts, material_map, list(materials), list(textures), transparent, stream)
        self._dynamic = True
        return self

    @staticmethod
    def _check_dev(name, t, dtype, numel, d, optional=False):
        if t is None and optional:
            return
        if not (hasattr(t, "data_ptr") and t.is_cuda and t.device == d and t.dtype == dtype and t.is_contiguous() and t.numel() == numel):
            raise ValueError("%s must be a contiguous %s tensor of %d values on %s" % (name, dtype, numel, d))

    def _dyn_args(self, what, d_nrm, d_verts):
        if not getattr(self, "_dynamic", False):
            raise _lib.SnailError("%s: the set was not made by MaterialSet.from_dev" % what)
        torch = _torch()
        n, d = self.scene._fast_n, self.scene._dev()
        self._check_dev("d_nrm", d_nrm, torch.float32, n * 9, d, optional=True)
        self._check_dev("d_verts", d_verts, torch.float32, n * 9, d, optional=True)
        return torch, d

    def rebuild_dev(self, d_verts, d_nrm=None, stream=None, info=None):
        """Rebuild the scene from new vertices, as Scene.rebuild_fast_dev does, and pack the records again through the new permutation on the
        same stream (snail_materials_rebuild_dev): with d_nrm, or with face normals of d_verts when it is None.  No host wait.  -> info, int32
        [6] device tensor: the rebuild's {status, nNodes, depth, n}, then {records committed (0 / 1), zeroed triangles}.  A status other
        than 0 leaves tree AND records as they were.  The tensors must stay alive and unchanged until the work enqueued here has run."""
        torch, d = self._dyn_args("rebuild_dev", d_nrm, d_verts)
        sc = self.scene
        sc._check_verts(d_verts, d)
        if info is None:
            info = torch.empty(6, dtype=torch.int32, device=d)
            if stream is not None:
                info.record_stream(stream)
        _lib.check(_lib.lib().snail_materials_rebuild_dev(self._h, _lib.ptr(d_verts), _lib.ptr(d_nrm), _lib.ptr(sc.d_perm), _lib.ptr(info), _stream_ptr(stream)),
                   "snail_materials_rebuild_dev")
        sc.d_info = info[:4]
        sc._stale = True           # .bvh / .perm / .depth are read back when next asked, as after Scene.rebuild_fast_dev
        return info

    def update_dev(self, d_nrm=None, d_verts=None, stream=None, info=None):
        """Pack the records again through scene.d_perm, and nothing else (snail_materials_update_dev): after the scene was rebuilt by
        Scene.rebuild_fast_dev or through another set, or for new normals alone.  -> info, int32 [2] device tensor {1, zeroed triangles}."""
        torch, d = self._dyn_args("update_dev", d_nrm, d_verts)
        if info is None:
            info = torch.empty(2, dtype=torch.int32, device=d)
            if stream is not None:
                info.record_stream(stream)
        _lib.check(_lib.lib().snail_materials_update_dev(self._h, _lib.ptr(self.scene.d_perm), _lib.ptr(d_nrm), _lib.ptr(d_verts), _lib.ptr(info), _stream_ptr(stream)),
                   "snail_materials_update_dev")
        return info

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().snail_materials_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _lights(lights7):
        return np.ascontiguousarray(lights7 if lights7 is not None else np.zeros((0, 7)), dtype=np.float32).reshape(-1, 7)

    def shade_packets(self, cam, resx: int, resy: int, packet_xy, hits, out=None, stream=None):
        """The samples of a packet list from its hit records (t, u, v, tri_id: packet-major [n, 256] device tensors, as Scene.trace_packets
        returns them) -> float32 [n, 9, 64, 4]: normal xyz, diffuse rgb, specular rgb per (quad, lane).  snail_materials_shade_packets_dev."""
        torch = _torch()
        n = int(packet_xy.shape[0])
        if out is None:
            out = torch.empty((n, SAMPLE_COMPONENTS, 64, 4), dtype=torch.float32, device=self.scene._dev())
        cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32)
        rc = _lib.lib().snail_materials_shade_packets_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(packet_xy), n, _lib.ptr(hits[0]), _lib.ptr(hits[1]),
                                                          _lib.ptr(hits[2]), _lib.ptr(hits[3]), _lib.ptr(out), _stream_ptr(stream))
        _lib.check(rc, "snail_materials_shade_packets_dev")
        return out

    def mirror_packets(self, cam, resx: int, resy: int, packet_xy, t, samples, stats=None, stream=None):
        """Scene::TraceReflection on the primary samples of a packet list (t: the hits' distances [n, 256]; samples: shade_packets' buffer) ->
        (origin, dir, idir [n, 64, 3, 4] float32, mask [n, 64] uint8, distance [n, 256] float32, object [n, 256] int32): the mirrored packets
        in the layouts snail_trace_rays_dev takes.  snail_materials_mirror_packets_dev."""
        torch = _torch()
        n = int(packet_xy.shape[0])
        dev = self.scene._dev()
        org, d, idir = (torch.empty((n, 64, 3, 4), dtype=torch.float32, device=dev) for _ in range(3))
        mask = torch.empty((n, 64), dtype=torch.uint8, device=dev)
        dist = torch.empty((n, 256), dtype=torch.float32, device=dev)
        obj = torch.empty((n, 256), dtype=torch.int32, device=dev)
        cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32)
        rc = _lib.lib().snail_materials_mirror_packets_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(packet_xy), n, _lib.ptr(t), _lib.ptr(samples), _lib.ptr(org),
                                                           _lib.ptr(d), _lib.ptr(idir), _lib.ptr(mask), _lib.ptr(dist), _lib.ptr(obj), _lib.ptr(stats), _stream_ptr(stream))
        _lib.check(rc, "snail_materials_mirror_packets_dev")
        return org, d, idir, mask, dist, obj

    def shade_rays(self, dirs, mask, t, u, v, tri_id, out=None, stream=None):
        """The samples of generic packets (RayGroup<0, hasMask>): dirs [n, 64, 3, 4], mask [n, 64] uint8 or None (every lane selected), hit
        records t / u / v / tri_id [n, 256] (device tensors) -> float32 [n, 9, 64, 4].  snail_materials_shade_rays_dev."""
        torch = _torch()
        n = int(dirs.shape[0])
        if out is None:
            out = torch.empty((n, SAMPLE_COMPONENTS, 64, 4), dtype=torch.float32, device=self.scene._dev())
        rc = _lib.lib().snail_materials_shade_rays_dev(self._h, n, _lib.ptr(dirs), _lib.ptr(mask), _lib.ptr(t), _lib.ptr(u), _lib.ptr(v), _lib.ptr(tri_id), _lib.ptr(out),
                                                       _stream_ptr(stream))
        _lib.check(rc, "snail_materials_shade_rays_dev")
        return out

    # ---- include/snail_materials_transparency.h ----------------------------------------------------------------------------------------
    @property
    def can_select_transparent(self) -> bool:
        """whether the set holds a material that can select a transparent lane (Material.transparent, or Material.uber with 0 < dissolve < 1):
        such a set is refused by every method above and below this block"""
        r = _lib.lib().snail_materials_can_select_transparent(self._h)
        if r < 0:
            raise _lib.SnailError("snail_materials_can_select_transparent: %s" % _lib.lib().snail_last_error().decode())
        return bool(r)

    def shade_packets_transp(self, cam, resx: int, resy: int, packet_xy, hits, stream=None):
        """shade_packets for any set, with Sample::opacity and the transparency selector -> (samples float32 [n, 9, 64, 4], opacity float32
        [n, 256], sel uint8 [n, 64]: low 4 bits = transSel after the opacity < 1 filter).  snail_materials_shade_packets_transp_dev."""
        torch = _torch()
        n = int(packet_xy.shape[0])
        dev = self.scene._dev()
        out = torch.empty((n, SAMPLE_COMPONENTS, 64, 4), dtype=torch.float32, device=dev)
        opacity = torch.empty((n, 256), dtype=torch.float32, device=dev)
        sel = torch.empty((n, 64), dtype=torch.uint8, device=dev)
        cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32)
        rc = _lib.lib().snail_materials_shade_packets_transp_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(packet_xy), n, _lib.ptr(hits[0]), _lib.ptr(hits[1]),
                                                                 _lib.ptr(hits[2]), _lib.ptr(hits[3]), _lib.ptr(out), _lib.ptr(opacity), _lib.ptr(sel), _stream_ptr(stream))
        _lib.check(rc, "snail_materials_shade_packets_transp_dev")
        return out, opacity, sel

    def shade_rays_transp(self, dirs, mask, t, u, v, tri_id, stream=None):
        """shade_rays for any set -> (samples, opacity, sel) as shade_packets_transp.  snail_materials_shade_rays_transp_dev."""
        torch = _torch()
        n = int(dirs.shape[0])
        dev = self.scene._dev()
        out = torch.empty((n, SAMPLE_COMPONENTS, 64, 4), dtype=torch.float32, device=dev)
        opacity = torch.empty((n, 256), dtype=torch.float32, device=dev)
        sel = torch.empty((n, 64), dtype=torch.uint8, device=dev)
        rc = _lib.lib().snail_materials_shade_rays_transp_dev(self._h, n, _lib.ptr(dirs), _lib.ptr(mask), _lib.ptr(t), _lib.ptr(u), _lib.ptr(v), _lib.ptr(tri_id),
                                                              _lib.ptr(out), _lib.ptr(opacity), _lib.ptr(sel), _stream_ptr(stream))
        _lib.check(rc, "snail_materials_shade_rays_transp_dev")
        return out, opacity, sel

    def continue_packets(self, t, sel, cam=None, resx: int = 0, resy: int = 0, packet_xy=None, rays=None, stats=None, stream=None):
        """Scene::TraceTransparency's packets of one level from its hits t [n, 256] and selector sel [n, 64] (device tensors).  The level's rays:
        cam / resx / resy / packet_xy (the primary level) or rays = (origin, dir, idir) [n, 64, 3, 4] (generic packets) ->
        (origin, dir, idir [n, 64, 3, 4] float32, mask [n, 64] uint8, distance [n, 256] float32, object [n, 256] int32, order [n] int32: the
        packet's index, or -1 when none of its lanes is selected).  snail_materials_continue_packets_dev."""
        torch = _torch()
        n = int(t.shape[0])
        dev = self.scene._dev()
        org, d, idir = (torch.empty((n, 64, 3, 4), dtype=torch.float32, device=dev) for _ in range(3))
        mask = torch.empty((n, 64), dtype=torch.uint8, device=dev)
        dist = torch.empty((n, 256), dtype=torch.float32, device=dev)
        obj = torch.empty((n, 256), dtype=torch.int32, device=dev)
        order = torch.empty((n,), dtype=torch.int32, device=dev)
        cam13 = None if cam is None else np.ascontiguousarray(cam.as_array13(), dtype=np.float32)
        ro, rd, ri = rays if rays is not None else (None, None, None)
        rc = _lib.lib().snail_materials_continue_packets_dev(self._h, _lib.ptr(cam13), int(resx), int(resy), _lib.ptr(packet_xy), n, _lib.ptr(ro), _lib.ptr(rd), _lib.ptr(ri),
                                                             _lib.ptr(t), _lib.ptr(sel), _lib.ptr(org), _lib.ptr(d), _lib.ptr(idir), _lib.ptr(mask), _lib.ptr(dist),
                                                             _lib.ptr(obj), _lib.ptr(order), _lib.ptr(stats), _stream_ptr(stream))
        _lib.check(rc, "snail_materials_continue_packets_dev")
        return org, d, idir, mask, dist, obj, order

    def _truncated(self, truncated):
        return truncated if truncated is not None else _torch().zeros(1, dtype=_torch().int64, device=self.scene._dev())

    def render_transparent(self, cam, resx: int, resy: int, lights7=None, ambient=(0.1, 0.1, 0.1), out=None, stats=None, stream=None, flags: int = 0,
                           max_depth: int = 8, truncated=None):
        """The lit frame with the transparency continuation, at most max_depth levels deep -> (frame [resy, resx, 3] uint8 (B,G,R) or `out`,
        truncated: an int64 device tensor of one word, += the lanes level max_depth would still select; 0 = the frame is the reference's).
        snail_materials_transparent_dev."""
        torch = _torch()
        if out is None:
            out = torch.zeros((resy, resx, 3), dtype=torch.uint8, device=self.scene._dev())
        truncated = self._truncated(truncated)
        lights = self._lights(lights7)
        cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32)
        amb = np.ascontiguousarray(ambient, dtype=np.float32)
        rc = _lib.lib().snail_materials_transparent_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(lights) if len(lights) else None, len(lights), _lib.ptr(amb),
                                                        int(flags), _lib.ptr(out), int(out.stride(0)), int(max_depth), _lib.ptr(truncated), _lib.ptr(stats), _stream_ptr(stream))
        _lib.check(rc, "snail_materials_transparent_dev")
        return out, truncated

    def render_transparent_packets(self, cam, resx: int, resy: int, packet_xy, lights7=None, ambient=(0.1, 0.1, 0.1), out=None, stats=None, stream=None,
                                   flags: int = 0, max_depth: int = 8, truncated=None):
        """render_transparent for an explicit packet list -> (packet-major [n, 256, 3] uint8 (B,G,R), truncated).
        snail_materials_transparent_packets_dev."""
        torch = _torch()
        n = int(packet_xy.shape[0])
        if out is None:
            out = torch.empty((n, 256, 3), dtype=torch.uint8, device=self.scene._dev())
        truncated = self._truncated(truncated)
        lights = self._lights(lights7)
        cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32)
        amb = np.ascontiguousarray(ambient, dtype=np.float32)
        rc = _lib.lib().snail_materials_transparent_packets_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(packet_xy), n, _lib.ptr(lights) if len(lights) else None,
                                                                len(lights), _lib.ptr(amb), int(flags), _lib.ptr(out), int(max_depth), _lib.ptr(truncated), _lib.ptr(stats),
                                                                _stream_ptr(stream))
        _lib.check(rc, "snail_materials_transparent_packets_dev")
        return out, truncated

    def render_transparent_image_host(self, cam, resx: int, resy: int, lights7=None, ambient=(0.1, 0.1, 0.1), flags: int = 0, pitch: int | None = None, fill: int = 0,
                                      max_depth: int = 8, truncated=None):
        """snail_materials_transparent_image: the frame in host memory -> (uint8 [resy, pitch], stats uint64 [4], truncated: uint64 [1], the
        caller's array (+=) or a new one)"""
        pitch = resx * 3 if pitch is None else int(pitch)
        img = np.full((resy, pitch), fill, dtype=np.uint8)
        stats = np.zeros(4, dtype=np.uint64)
        truncated = np.zeros(1, dtype=np.uint64) if truncated is None else truncated
        lights = self._lights(lights7)
        cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32)
        amb = np.ascontiguousarray(ambient, dtype=np.float32)
        rc = _lib.lib().snail_materials_transparent_image(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(lights) if len(lights) else None, len(lights), _lib.ptr(amb),
                                                          int(flags), _lib.ptr(img), pitch, int(max_depth), _lib.ptr(truncated), _lib.ptr(stats))
        _lib.check(rc, "snail_materials_transparent_image")
        return img, stats, truncated

    def render(self, cam, resx: int, resy: int, lights7=None, ambient=(0.1, 0.1, 0.1), out=None, stats=None, stream=None, flags: int = 0, reflections: bool = False):
        """The lit frame, [resy, resx, 3] uint8 (B,G,R) (or `out`: a uint8 device tensor [resy, pitch] / [resy, w, 3] whose rows may be wider).
        reflections=True: with the one mirrored bounce of gVals[7] (snail_materials_bounce_dev; `flags` are then that function's)."""
        torch = _torch()
        if out is None:
            out = torch.zeros((resy, resx, 3), dtype=torch.uint8, device=self.scene._dev())
        pitch = int(out.stride(0))
        lights = self._lights(lights7)
        cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32)
        amb = np.ascontiguousarray(ambient, dtype=np.float32)
        if reflections:
            rc = _lib.lib().snail_materials_bounce_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(lights) if len(lights) else None, len(lights), _lib.ptr(amb),
                                                       int(flags) | RENDER_REFLECTIONS, _lib.ptr(out), pitch, _lib.ptr(stats), _stream_ptr(stream))
            _lib.check(rc, "snail_materials_bounce_dev")
            return out
        rc = _lib.lib().snail_render_materials_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(lights) if len(lights) else None, len(lights), _lib.ptr(amb),
                                                   int(flags), _lib.ptr(out), pitch, _lib.ptr(stats), _stream_ptr(stream))
        _lib.check(rc, "snail_render_materials_dev")
        return out

    def render_packets(self, cam, resx: int, resy: int, packet_xy, lights7=None, ambient=(0.1, 0.1, 0.1), out=None, stats=None, stream=None, flags: int = 0,
                       reflections: bool = False):
        """render for an explicit packet list: packet-major [n, 256, 3] uint8 (B,G,R).  reflections=True: snail_materials_bounce_packets_dev."""
        torch = _torch()
        n = int(packet_xy.shape[0])
        if out is None:
            out = torch.empty((n, 256, 3), dtype=torch.uint8, device=self.scene._dev())
        lights = self._lights(lights7)
        cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32)
        amb = np.ascontiguousarray(ambient, dtype=np.float32)
        if reflections:
            rc = _lib.lib().snail_materials_bounce_packets_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(packet_xy), n, _lib.ptr(lights) if len(lights) else None,
                                                               len(lights), _lib.ptr(amb), int(flags) | RENDER_REFLECTIONS, _lib.ptr(out), _lib.ptr(stats), _stream_ptr(stream))
            _lib.check(rc, "snail_materials_bounce_packets_dev")
            return out
        rc = _lib.lib().snail_render_materials_packets_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(packet_xy), n, _lib.ptr(lights) if len(lights) else None,
                                                           len(lights), _lib.ptr(amb), int(flags), _lib.ptr(out), _lib.ptr(stats), _stream_ptr(stream))
        _lib.check(rc, "snail_render_materials_packets_dev")
        return out

    def render_image_host(self, cam, resx: int, resy: int, lights7=None, ambient=(0.1, 0.1, 0.1), flags: int = 0, pitch: int | None = None, fill: int = 0,
                          reflections: bool = False):
        """snail_render_materials_image: the frame in host memory, uint8 [resy, pitch] (pitch = 3 * resx unless given; bytes past a row's
        pixels keep `fill`), and the call's TreeStats.  reflections=True: snail_materials_bounce_image."""
        pitch = resx * 3 if pitch is None else int(pitch)
        img = np.full((resy, pitch), fill, dtype=np.uint8)
        stats = np.zeros(4, dtype=np.uint64)
        lights = self._lights(lights7)
        cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32)
        amb = np.ascontiguousarray(ambient, dtype=np.float32)
        if reflections:
            rc = _lib.lib().snail_materials_bounce_image(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(lights) if len(lights) else None, len(lights), _lib.ptr(amb),
                                                         int(flags) | RENDER_REFLECTIONS, _lib.ptr(img), pitch, _lib.ptr(stats))
            _lib.check(rc, "snail_materials_bounce_image")
            return img, stats
        rc = _lib.lib().snail_render_materials_image(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(lights) if len(lights) else None, len(lights), _lib.ptr(amb),
                                                     int(flags), _lib.ptr(img), pitch, _lib.ptr(stats))
        _lib.check(rc, "snail_render_materials_image")
        return img, stats

    # ---- include/snail_materials_tiles.h: any of RENDER_REFLECTIONS / RENDER_DEPTH / RENDER_AA4, the tint, tile lists -------------------
    def _tile_args(self, cam, lights7, ambient, tint):
        lights = self._lights(lights7)
        cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32)
        amb = np.ascontiguousarray(ambient, dtype=np.float32)
        tnt = None if tint is None else np.ascontiguousarray(tint, dtype=np.float32).reshape(3)
        return lights, (_lib.ptr(lights) if len(lights) else None), cam13, amb, tnt

    def frame_packets(self, cam, resx: int, resy: int, packet_xy, lights7=None, flags: int = 0, tint=None, ambient=(0.1, 0.1, 0.1), out=None, stats=None,
                      stream=None):
        """snail_materials_frame_packets_dev: the packets of an explicit list (int32 [n, 2] device tensor) with any of RENDER_REFLECTIONS /
        RENDER_DEPTH / RENDER_AA4 and an optional tint (three factors, gVals[8]): packet-major [n, 256, 3] uint8 (B,G,R)."""
        torch = _torch()
        n = int(packet_xy.shape[0])
        if out is None:
            out = torch.empty((n, 256, 3), dtype=torch.uint8, device=self.scene._dev())
        lights, lp, cam13, amb, tnt = self._tile_args(cam, lights7, ambient, tint)
        rc = _lib.lib().snail_materials_frame_packets_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(packet_xy), n, lp, len(lights), _lib.ptr(amb), int(flags),
                                                          _lib.ptr(tnt), _lib.ptr(out), _lib.ptr(stats), _stream_ptr(stream))
        _lib.check(rc, "snail_materials_frame_packets_dev")
        return out

    def render_tiles_host(self, cam, resx: int, resy: int, tiles, offsets=None, lights7=None, flags: int = 0, tint=None, ambient=(0.1, 0.1, 0.1), data=None):
        """snail_materials_render_tiles: the tile-list renderer of src/render.h:16-19 with full shading.  tiles = [n, 4] (x, y, w, h); returns
        (data, offsets, stats) with tile k's planes R, G-R, B-R at data[offsets[k]:offsets[k] + 3 w h], back to back unless the caller
        brings `offsets` (and, if it likes, a `data` buffer of its own).  tint = three factors (gVals[8]) or None."""
        t = np.ascontiguousarray(tiles, dtype=np.int32).reshape(-1, 4)
        size = 3 * t[:, 2].astype(np.int64) * t[:, 3]
        if offsets is None:
            offsets = np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.int64)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if data is None:
            data = np.zeros(int((offsets + size).max()) if len(t) else 0, dtype=np.uint8)
        lights, lp, cam13, amb, tnt = self._tile_args(cam, lights7, ambient, tint)
        stats = np.zeros(4, dtype=np.uint64)
        rc = _lib.lib().snail_materials_render_tiles(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(t), _lib.ptr(offsets), len(t), lp, len(lights), _lib.ptr(amb),
                                                     int(flags), _lib.ptr(tnt), _lib.ptr(data), _lib.ptr(stats))
        _lib.check(rc, "snail_materials_render_tiles")
        return data, offsets, stats

    def render_frame_host(self, cam, resx: int, resy: int, lights7=None, flags: int = 0, ambient=(0.1, 0.1, 0.1), pitch: int | None = None, fill: int = 0):
        """snail_materials_render_frame: render_image_host with RENDER_DEPTH and RENDER_AA4 accepted -> (uint8 [resy, pitch] (B,G,R rows; pitch =
        3 * resx unless given, bytes past a row's pixels keep `fill`), stats)."""
        pitch = resx * 3 if pitch is None else int(pitch)
        img = np.full((resy, pitch), fill, dtype=np.uint8)
        stats = np.zeros(4, dtype=np.uint64)
        lights, lp, cam13, amb, _ = self._tile_args(cam, lights7, ambient, None)
        rc = _lib.lib().snail_materials_render_frame(self._h, _lib.ptr(cam13), resx, resy, lp, len(lights), _lib.ptr(amb), int(flags), _lib.ptr(img), pitch,
                                                     _lib.ptr(stats))
        _lib.check(rc, "snail_materials_render_frame")
        return img, stats

    # ---- include/snail_materials_tree.h: the continuation together with the bounce, tile lists, 4x AA, depth shading and the tint; any set ----
    def mirror_rays(self, origin, dirs, mask, t, samples, order_in=None, out=None, stats=None, stream=None):
        """Scene::TraceReflection from a level's generic packets: origin / dirs [n, 64, 3, 4], mask [n, 64] uint8 or None (every lane selected),
        t [n, 256], the level's samples [n, 9, 64, 4] (device tensors); order_in [n] int32 or None: the level's own order list ->
        (origin, dir, idir [n, 64, 3, 4] float32, mask [n, 64] uint8, distance [n, 256] float32, object [n, 256] int32, order [n] int32), or
        the seven tensors of `out` written in place: a packet whose order_in word is negative gets order -1 and nothing else.
        snail_materials_mirror_rays_dev."""
        torch = _torch()
        n = int(dirs.shape[0])
        dev = self.scene._dev()
        if out is None:
            out = tuple(torch.empty((n, 64, 3, 4), dtype=torch.float32, device=dev) for _ in range(3)) + (
                torch.empty((n, 64), dtype=torch.uint8, device=dev), torch.empty((n, 256), dtype=torch.float32, device=dev),
                torch.empty((n, 256), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev))
        org, d, idir, msk, dist, obj, order = out
        rc = _lib.lib().snail_materials_mirror_rays_dev(self._h, n, _lib.ptr(origin), _lib.ptr(dirs), _lib.ptr(mask), _lib.ptr(t), _lib.ptr(samples), _lib.ptr(order_in),
                                                        _lib.ptr(org), _lib.ptr(d), _lib.ptr(idir), _lib.ptr(msk), _lib.ptr(dist), _lib.ptr(obj), _lib.ptr(order),
                                                        _lib.ptr(stats), _stream_ptr(stream))
        _lib.check(rc, "snail_materials_mirror_rays_dev")
        return out

    def tree_frame_packets(self, cam, resx: int, resy: int, packet_xy, lights7=None, flags: int = 0, tint=None, ambient=(0.1, 0.1, 0.1), out=None, stats=None,
                           stream=None, max_depth: int = 8, truncated=None):
        """frame_packets for any set, with the transparency continuation at most max_depth levels deep under any of RENDER_REFLECTIONS /
        RENDER_DEPTH / RENDER_AA4 and the tint -> (packet-major [n, 256, 3] uint8 (B,G,R), truncated: int64 device tensor of one word, +=).
        snail_materials_tree_frame_packets_dev."""
        torch = _torch()
        n = int(packet_xy.shape[0])
        if out is None:
            out = torch.empty((n, 256, 3), dtype=torch.uint8, device=self.scene._dev())
        truncated = self._truncated(truncated)
        lights, lp, cam13, amb, tnt = self._tile_args(cam, lights7, ambient, tint)
        rc = _lib.lib().snail_materials_tree_frame_packets_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(packet_xy), n, lp, len(lights), _lib.ptr(amb), int(flags),
                                                               _lib.ptr(tnt), _lib.ptr(out), int(max_depth), _lib.ptr(truncated), _lib.ptr(stats), _stream_ptr(stream))
        _lib.check(rc, "snail_materials_tree_frame_packets_dev")
        return out, truncated

    def render_tree_tiles_host(self, cam, resx: int, resy: int, tiles, offsets=None, lights7=None, flags: int = 0, tint=None, ambient=(0.1, 0.1, 0.1), data=None,
                               max_depth: int = 8, truncated=None):
        """render_tiles_host for any set -> (data, offsets, stats, truncated: uint64 [1], the caller's array (+=) or a new one).
        snail_materials_tree_render_tiles."""
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
        rc = _lib.lib().snail_materials_tree_render_tiles(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(t), _lib.ptr(offsets), len(t), lp, len(lights), _lib.ptr(amb),
                                                          int(flags), _lib.ptr(tnt), _lib.ptr(data), int(max_depth), _lib.ptr(truncated), _lib.ptr(stats))
        _lib.check(rc, "snail_materials_tree_render_tiles")
        return data, offsets, stats, truncated

    def render_tree_frame_host(self, cam, resx: int, resy: int, lights7=None, flags: int = 0, ambient=(0.1, 0.1, 0.1), pitch: int | None = None, fill: int = 0,
                               max_depth: int = 8, truncated=None):
        """render_frame_host for any set -> (uint8 [resy, pitch], stats, truncated: uint64 [1]).  snail_materials_tree_render_frame."""
        pitch = resx * 3 if pitch is None else int(pitch)
        img = np.full((resy, pitch), fill, dtype=np.uint8)
        stats = np.zeros(4, dtype=np.uint64)
        truncated = np.zeros(1, dtype=np.uint64) if truncated is None else truncated
        lights, lp, cam13, amb, _ = self._tile_args(cam, lights7, ambient, None)
        rc = _lib.lib().snail_materials_tree_render_frame(self._h, _lib.ptr(cam13), resx, resy, lp, len(lights), _lib.ptr(amb), int(flags), _lib.ptr(img), pitch,
                                                          int(max_depth), _lib.ptr(truncated), _lib.ptr(stats))
        _lib.check(rc, "snail_materials_tree_render_frame")
        return img, stats, truncated

    def set_level_budget(self, nbytes: int):
        """snail_materials_set_level_budget: the bytes the levels of one group of intermediates may take; a call clamps it up to one output
        packet's worth and runs its packet list in slices that stay within it"""
        _lib.check(_lib.lib().snail_materials_set_level_budget(self._h, int(nbytes)), "snail_materials_set_level_budget")

    @staticmethod
    def level_bytes(n_lights: int, flags: int = 0, max_depth: int = 8) -> int:
        """snail_materials_level_bytes: the bytes of the levels of ONE output packet"""
        b = _lib.lib().snail_materials_level_bytes(int(n_lights), int(flags), int(max_depth))
        if b < 0:
            raise _lib.SnailError("snail_materials_level_bytes: %s" % _lib.lib().snail_last_error().decode())
        return int(b)

    # ---- include/snail_materials_heatmap.h: per-packet TreeStats and the gVals[5] heat-map under full shading; any set ----
    def packet_stats(self, cam, resx: int, resy: int, packet_xy=None, lights7=None, reflections: bool = False, out=None, stats=None, stream=None, flags: int = 0,
                     max_depth: int = 8, truncated=None):
        """snail_materials_packet_stats_dev: the TreeStats {intersects, iterations, rays, skips} of every packet's RayTrace call under full
        shading -- the whole tree of nested calls -- -> (int32 device tensor [n, 4] holding uint32 words, truncated: int64 device tensor of one
        word, +=).  packet_xy = int32 device tensor [n, 2], or None = the frame's grid, row-major."""
        torch = _torch()
        n = int(packet_xy.shape[0]) if packet_xy is not None else ((resx + 15) // 16) * ((resy + 15) // 16)
        if out is None:
            out = torch.zeros((n, 4), dtype=torch.int32, device=self.scene._dev())
        truncated = self._truncated(truncated)
        lights, lp, cam13, _, _ = self._tile_args(cam, lights7, (0.0, 0.0, 0.0), None)
        rc = _lib.lib().snail_materials_packet_stats_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(packet_xy), n, lp, len(lights),
                                                         int(flags) | (RENDER_REFLECTIONS if reflections else 0), int(max_depth), _lib.ptr(out), _lib.ptr(truncated),
                                                         _lib.ptr(stats), _stream_ptr(stream))
        _lib.check(rc, "snail_materials_packet_stats_dev")
        return out, truncated

    def render_heat_packets(self, cam, resx: int, resy: int, packet_xy=None, lights7=None, flags: int = 0, tint=None, out=None, packet_stats=None, stats=None,
                            stream=None, max_depth: int = 8, truncated=None):
        """snail_materials_heat_packets_dev: the heat-map of the packets -> (packet-major [n, 256, 3] uint8 (B,G,R), truncated).  flags:
        RENDER_REFLECTIONS, RENDER_AA4; tint = three factors (gVals[8]) or None; packet_stats (optional) int32 device tensor [n, 4] ([n, 4, 4]
        with RENDER_AA4)."""
        torch = _torch()
        n = int(packet_xy.shape[0]) if packet_xy is not None else ((resx + 15) // 16) * ((resy + 15) // 16)
        if out is None:
            out = torch.empty((n, 256, 3), dtype=torch.uint8, device=self.scene._dev())
        truncated = self._truncated(truncated)
        lights, lp, cam13, _, tnt = self._tile_args(cam, lights7, (0.0, 0.0, 0.0), tint)
        rc = _lib.lib().snail_materials_heat_packets_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(packet_xy), n, lp, len(lights), int(flags), _lib.ptr(tnt),
                                                         _lib.ptr(out), _lib.ptr(packet_stats), int(max_depth), _lib.ptr(truncated), _lib.ptr(stats), _stream_ptr(stream))
        _lib.check(rc, "snail_materials_heat_packets_dev")
        return out, truncated

    def render_heat_tiles_host(self, cam, resx: int, resy: int, tiles, offsets=None, lights7=None, flags: int = 0, tint=None, data=None, max_depth: int = 8,
                               truncated=None):
        """snail_materials_render_heat_tiles: render_tree_tiles_host with gVals[5] -> (data, offsets, stats, truncated: uint64 [1], the caller's
        array (+=) or a new one)."""
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
        rc = _lib.lib().snail_materials_render_heat_tiles(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(t), _lib.ptr(offsets), len(t), lp, len(lights), int(flags),
                                                          _lib.ptr(tnt), _lib.ptr(data), int(max_depth), _lib.ptr(truncated), _lib.ptr(stats))
        _lib.check(rc, "snail_materials_render_heat_tiles")
        return data, offsets, stats, truncated

    def render_heat_frame_host(self, cam, resx: int, resy: int, lights7=None, flags: int = 0, pitch: int | None = None, fill: int = 0, max_depth: int = 8,
                               truncated=None):
        """snail_materials_render_heat_frame: render_tree_frame_host with gVals[5] -> (uint8 [resy, pitch] (B,G,R rows; pitch = 3 * resx unless
        given, bytes past a row's pixels keep `fill`), stats, truncated: uint64 [1])."""
        pitch = resx * 3 if pitch is None else int(pitch)
        img = np.full((resy, max(pitch, 0)), fill, dtype=np.uint8)
        stats = np.zeros(4, dtype=np.uint64)
        truncated = np.zeros(1, dtype=np.uint64) if truncated is None else truncated
        lights, lp, cam13, _, _ = self._tile_args(cam, lights7, (0.0, 0.0, 0.0), None)
        rc = _lib.lib().snail_materials_render_heat_frame(self._h, _lib.ptr(cam13), resx, resy, lp, len(lights), int(flags), _lib.ptr(img), pitch, int(max_depth),
                                                          _lib.ptr(truncated), _lib.ptr(stats))
        _lib.check(rc, "snail_materials_render_heat_frame")
        return img, stats, truncated
