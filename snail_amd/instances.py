"""Two-level instanced scenes: the host-side mirror of the reference's second `AccStruct` model, DBVH (src/dbvh/tree.h,
src/dbvh/tree.cpp, src/dbvh/traverse.cpp), over the C-ABI of include/snail_instances.h.

  InstancedScene(blas, rotations, translations, blas_index)   <-> DBVH(vector<ObjectInstance>)   (host build: snail_instances_build)
  .update(rotations, translations, blas_index)                <-> rebuilding the DBVH for the next frame (rtracer.cpp's -instances mode)
  .update_dev(xf12, blas_index)                                <-> the same rebuild ON THE DEVICE from device tensors (snail_instances_rebuild_dev)
  .trace_primary(cam, resx, resy)                              <-> RayGenerator + SafeInv + DBVH::TraversePrimary over 16x16 packets
  .traverse_primary(ctx, element) / .traverse_shadow(ctx)     <-> DBVH::TraversePrimary<so,mask> / DBVH::TraverseShadow
  .render_tiles_host(cam, resx, resy, tiles, ...)              <-> Render(scene, camera, resx, resy, data, coords, offsets, options, rank, threads)

The instance id a hit reports is the instance's BUILDER SLOT (the DBVH::elements order); .perm()[slot] is the caller's instance."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .bvh import NODE_DTYPE
from .scene import Scene, Context, ShadowContext, HitFrame, _filled_on, _stream_ptr, _torch


def _xf12(rotations, translations) -> np.ndarray:
    r = np.ascontiguousarray(rotations, dtype=np.float32).reshape(-1, 3, 3)
    t = np.ascontiguousarray(translations, dtype=np.float32).reshape(-1, 3)
    if len(r) != len(t):
        raise ValueError("rotations and translations differ in length")
    return np.ascontiguousarray(np.concatenate([r.reshape(-1, 9), t], axis=1), dtype=np.float32)


def build_instances(xf12: np.ndarray, blas_index: np.ndarray, blas_bbox6: np.ndarray):
    """snail_instances_build -> (nodes NODE_DTYPE [nNodes], depth, perm int32 [n]: builder slot -> caller's instance)."""
    xf = np.ascontiguousarray(xf12, dtype=np.float32).reshape(-1, 12)
    bi = np.ascontiguousarray(blas_index, dtype=np.int32).reshape(-1)
    bb = np.ascontiguousarray(blas_bbox6, dtype=np.float32).reshape(-1, 6)
    n = len(xf)
    if len(bi) != n:
        raise ValueError("blas_index must hold one entry per instance")
    nodes = np.zeros(max(2 * n, 1), dtype=NODE_DTYPE)
    perm = np.zeros(n, dtype=np.int32)
    nn, depth = C.c_int(0), C.c_int(0)
    _lib.check(_lib.lib().snail_instances_build(_lib.ptr(xf), _lib.ptr(bi), n, _lib.ptr(bb), len(bb), _lib.ptr(nodes), C.addressof(nn),
                                                C.addressof(depth), _lib.ptr(perm)), "snail_instances_build")
    return np.ascontiguousarray(nodes[:nn.value]), depth.value, perm


class InstancedScene:
    """Rigid instances of BLAS scenes (snail_amd.scene.Scene, kept alive by this object) under a top-level tree resident on their GPU."""

    def __init__(self, blas_scenes, rotations, translations, blas_index=None):
        self.blas = list(blas_scenes) if isinstance(blas_scenes, (list, tuple)) else [blas_scenes]
        if not self.blas:
            raise ValueError("at least one BLAS scene")
        self.device = self.blas[0].device
        self._h = None
        nodes, depth, xf, bi, perm = self._build(rotations, translations, blas_index)
        arr = (C.c_void_p * len(self.blas))(*[s._h.value for s in self.blas])
        h = _lib.lib().snail_instances_create(arr, len(self.blas), _lib.ptr(nodes), len(nodes), _lib.ptr(xf), _lib.ptr(bi), len(xf), depth)
        if not h:
            raise _lib.SnailError("snail_instances_create: %s" % _lib.lib().snail_last_error().decode())
        self._h = C.c_void_p(h)
        self._set(nodes, depth, xf, bi, perm)

    @classmethod
    def from_tree(cls, blas_scenes, nodes, xf12_slots, blas_index_slots, depth: int = 0):
        """A caller's tree (e.g. the reference's own DBVH::nodes with its elements' transforms in slot order), validated by
        snail_instances_create; perm() is then the identity."""
        self = cls.__new__(cls)
        self.blas = list(blas_scenes)
        self.device = self.blas[0].device
        self._h = None
        nodes = np.ascontiguousarray(np.asarray(nodes).view(NODE_DTYPE))
        xf = np.ascontiguousarray(xf12_slots, dtype=np.float32).reshape(-1, 12)
        bi = np.ascontiguousarray(blas_index_slots, dtype=np.int32).reshape(-1)
        arr = (C.c_void_p * len(self.blas))(*[s._h.value for s in self.blas])
        h = _lib.lib().snail_instances_create(arr, len(self.blas), _lib.ptr(nodes), len(nodes), _lib.ptr(xf), _lib.ptr(bi), len(xf), int(depth))
        if not h:
            raise _lib.SnailError("snail_instances_create: %s" % _lib.lib().snail_last_error().decode())
        self._h = C.c_void_p(h)
        self._set(nodes, int(depth), xf, bi, np.arange(len(xf), dtype=np.int32))
        return self

    def _build(self, rotations, translations, blas_index):
        xf = _xf12(rotations, translations)
        n = len(xf)
        bi = np.zeros(n, dtype=np.int32) if blas_index is None else np.ascontiguousarray(blas_index, dtype=np.int32).reshape(-1)
        bb = np.stack([np.concatenate(s.get_bbox()) for s in self.blas]).astype(np.float32)
        nodes, depth, perm = build_instances(xf, bi, bb)
        # the handle takes the records in builder-slot order (DBVH::elements)
        return nodes, depth, np.ascontiguousarray(xf[perm]), np.ascontiguousarray(bi[perm]), perm

    def _set(self, nodes, depth, xf, bi, perm):
        self._nodes, self._depth, self._xf, self._bi, self._perm = nodes, depth, xf, bi, perm
        # update_dev: _dirty = the handle may hold another tree than the fields above; _d_perm = the scene's own device copy of perm, which
        # every rebuild that stands overwrites and a refused one leaves alone (_perm_seeded: it starts from the fields above)
        self._dirty = False
        self._perm_seeded = False
        if not hasattr(self, "_d_perm"):
            self._d_perm = None

    def update(self, rotations, translations, blas_index=None, stream=None) -> None:
        """New transforms and a new tree for the next frame, ordered on `stream` after every launch enqueued before it."""
        nodes, depth, xf, bi, perm = self._build(rotations, translations, blas_index)
        _lib.check(_lib.lib().snail_instances_update(self._h, _lib.ptr(nodes), len(nodes), _lib.ptr(xf), _lib.ptr(bi), len(xf), depth, _stream_ptr(stream)),
                   "snail_instances_update")
        self._set(nodes, depth, xf, bi, perm)

    def update_dev(self, xf12, blas_index=None, stream=None, perm=None, info=None):
        """update() on the device (snail_instances_rebuild_dev): xf12 = float32 [n, 12] and blas_index = int32 [n] (None: all 0) are torch
        tensors on the scene's device in the CALLER's order; nothing waits on the host, except when the scene's buffers grow and on the
        first call after an update().  The tree, the slot order and the records it leaves are byte-equal to update()'s.
        -> (perm int32 [n]: slot -> caller's instance, info int32 [4]: {status, nNodes, depth, n}), device tensors filled on `stream`;
        status 1 (non-finite transform, BLAS index out of range) or 2 (deeper than 64 levels) leaves the scene as it was.  Without `perm`
        the returned tensor is a view of the scene's own copy, valid until the next update_dev; with `perm` it is copied there on `stream`.
        xf12 and blas_index are read on `stream` and must stay alive and unchanged until that work has run (keep the tensors, or
        record_stream them, when `stream` is not the current one).  nodes() / perm() / slot_transforms() / depth read the handle back (and
        wait for it) when they are next asked."""
        n, info = self._update_dev_begin(xf12, blas_index, stream, perm, info)
        _lib.check(_lib.lib().snail_instances_rebuild_dev(self._h, _lib.ptr(xf12), _lib.ptr(blas_index), n, _lib.ptr(self._d_perm), _lib.ptr(info),
                                                          _stream_ptr(stream)), "snail_instances_rebuild_dev")
        return self._update_dev_end(n, stream, perm, info)

    def _update_dev_begin(self, xf12, blas_index, stream, perm, info):
        """update_dev before its library call: the arguments checked, the scene's device copy of perm in place -> (n, info tensor).  (Shared with
        InstancedMaterialSet.rebuild_all_dev, whose one call rebuilds BLASes and this tree.)"""
        torch = _torch()
        d = self._dev()
        if not (hasattr(xf12, "data_ptr") and xf12.is_cuda and xf12.device == d and xf12.dtype == torch.float32 and xf12.dim() == 2
                and xf12.shape[1] == 12 and xf12.is_contiguous()):
            raise ValueError("xf12 must be a contiguous float32 [n, 12] tensor on %s" % d)
        n = int(xf12.shape[0])
        if blas_index is not None and not (blas_index.is_cuda and blas_index.device == d and blas_index.dtype == torch.int32
                                           and blas_index.numel() == n and blas_index.is_contiguous()):
            raise ValueError("blas_index must be a contiguous int32 [n] tensor on %s" % d)
        if perm is not None and not (perm.is_cuda and perm.device == d and perm.dtype == torch.int32 and perm.numel() >= n and perm.is_contiguous()):
            raise ValueError("perm must be a contiguous int32 tensor of at least n entries on %s" % d)
        cap = 0 if self._d_perm is None else int(self._d_perm.numel())
        if cap < n or not self._perm_seeded:
            # (one-off, like the growth of the handle's buffers: the scene's device copy of perm starts from what the host knows)
            self._refresh()
            torch.cuda.synchronize(d)
            if cap < max(n, len(self._perm)):
                self._d_perm = torch.empty(max(n, len(self._perm), 2 * cap), dtype=torch.int32, device=d)
            self._d_perm[:len(self._perm)].copy_(torch.from_numpy(np.ascontiguousarray(self._perm, dtype=np.int32)))
            torch.cuda.synchronize(d)
            self._perm_seeded = True
        if info is None:
            info = torch.empty(4, dtype=torch.int32, device=d)
            if stream is not None:
                info.record_stream(stream)
        return n, info

    def _update_dev_end(self, n, stream, perm, info):
        """update_dev after its library call -> (perm, info)"""
        torch = _torch()
        d = self._dev()
        self._dirty = True
        if perm is None:
            return self._d_perm[:n], info
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(d)):
            perm[:n].copy_(self._d_perm[:n])
        return perm, info

    def _refresh(self):
        """what the handle holds after the update_dev calls since the last look: its own tree and records (snail_instances_read_tree,
        which waits for everything enqueued), the depth of that tree, and the perm of the latest rebuild that stood"""
        if not self._dirty:
            return
        nn, n = C.c_int(0), C.c_int(0)
        L = _lib.lib()
        _lib.check(L.snail_instances_read_tree(self._h, None, 0, C.addressof(nn), None, None, 0, C.addressof(n)), "snail_instances_read_tree")
        nodes = np.zeros(nn.value, dtype=NODE_DTYPE)
        xf = np.zeros((n.value, 12), dtype=np.float32)
        bi = np.zeros(n.value, dtype=np.int32)
        _lib.check(L.snail_instances_read_tree(self._h, _lib.ptr(nodes), len(nodes), None, _lib.ptr(xf), _lib.ptr(bi), len(xf), None),
                   "snail_instances_read_tree")
        # depth = the deepest leaf (children follow their parent)
        sub = nodes["sub"].astype(np.int64)
        level = np.zeros(len(nodes), dtype=np.int64)
        for i in np.nonzero((sub & 0x80000000) == 0)[0]:
            level[sub[i]] = level[sub[i] + 1] = level[i] + 1
        self._nodes, self._depth, self._xf, self._bi = nodes, int(level.max()), xf, bi
        self._perm = self._d_perm[:n.value].cpu().numpy().astype(np.int32)
        self._dirty = False

    @property
    def depth(self) -> int:
        self._refresh()
        return self._depth

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().snail_instances_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # ---- for tests --------------------------------------------------------------------------------
    def nodes(self) -> np.ndarray:
        self._refresh()
        return self._nodes.copy()

    def perm(self) -> np.ndarray:
        self._refresh()
        return self._perm.copy()

    def slot_transforms(self):
        """(xf12 [n,12], blas_index [n]) in builder-slot order, as the handle holds them."""
        self._refresh()
        return self._xf.copy(), self._bi.copy()

    # ---- traversal ----------------------------------------------------------------------------------
    def _dev(self):
        return _torch().device("cuda", self.device)

    def new_stats(self):
        return _torch().zeros(4, dtype=_torch().int64, device=self._dev())

    def trace_primary(self, cam, resx: int, resy: int, rect=None, stats=None, stream=None):
        """-> (t, u, v, instance, tri_id) row-major [resy, resx] tensors; miss = (+inf, 0, 0, 0, 0)."""
        torch = _torch()
        x0, y0, w, h = rect if rect is not None else (0, 0, resx, resy)
        d = self._dev()
        with _filled_on(stream):
            t = torch.full((resy, resx), float("inf"), dtype=torch.float32, device=d)
            u = torch.zeros((resy, resx), dtype=torch.float32, device=d)
            v = torch.zeros((resy, resx), dtype=torch.float32, device=d)
            inst = torch.zeros((resy, resx), dtype=torch.int32, device=d)
            tri = torch.zeros((resy, resx), dtype=torch.int32, device=d)
        cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32)
        rc = _lib.lib().snail_instances_trace_primary_dev(self._h, _lib.ptr(cam13), resx, resy, x0, y0, w, h, _lib.ptr(t), _lib.ptr(u), _lib.ptr(v),
                                                         _lib.ptr(inst), _lib.ptr(tri), _lib.ptr(stats), _stream_ptr(stream))
        _lib.check(rc, "snail_instances_trace_primary_dev")
        return t, u, v, inst, tri

    def trace_packets(self, cam, resx: int, resy: int, packet_xy, stats=None, stream=None):
        """Packet-major [n,256] (t, u, v, instance, tri_id) of the packets at int32 [n,2] pixel origins (device tensor)."""
        torch = _torch()
        n = int(packet_xy.shape[0])
        d = self._dev()
        with _filled_on(stream):
            t = torch.full((n, 256), float("inf"), dtype=torch.float32, device=d)
            u = torch.zeros((n, 256), dtype=torch.float32, device=d)
            v = torch.zeros((n, 256), dtype=torch.float32, device=d)
            inst = torch.zeros((n, 256), dtype=torch.int32, device=d)
            tri = torch.zeros((n, 256), dtype=torch.int32, device=d)
        cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32)
        rc = _lib.lib().snail_instances_trace_packets_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(packet_xy), n, _lib.ptr(t), _lib.ptr(u), _lib.ptr(v),
                                                         _lib.ptr(inst), _lib.ptr(tri), _lib.ptr(stats), _stream_ptr(stream))
        _lib.check(rc, "snail_instances_trace_packets_dev")
        return t, u, v, inst, tri

    def render_depth(self, cam, resx: int, resy: int, arith=None, stream=None):
        """The gVals[1] depth-shaded RGB8 frame [resy, resx, 3] (B,G,R) of the instanced scene: packet-major distances, then the existing
        shade_depth and frame-store kernels."""
        torch = _torch()
        from .render import divide_image, tile_packets
        xy = np.ascontiguousarray(tile_packets(divide_image(resx, resy)), dtype=np.int32).reshape(-1, 2)
        pxy = torch.from_numpy(xy).to(self._dev())
        t = self.trace_packets(cam, resx, resy, pxy, stream=stream)[0]
        a = arith if arith is not None else self.blas[0].arith()
        bgr = Scene.shade_depth(t, stream=stream, arith=a)
        frame = torch.zeros((resy, resx, 3), dtype=torch.uint8, device=self._dev())
        Scene.packets_bgr_to_frame(pxy, bgr, frame, stream=stream)
        return frame

    def render_whitted(self, cam, resx: int, resy: int, lights7, ambient=(0.1, 0.1, 0.1), color=(1.0, 1.0, 1.0), out=None, stats=None, stream=None,
                       reflections: bool = False):
        """Scene<DBVH>::RayTrace in the simple-shading configuration (Scene.render_whitted for an instanced scene: primary packets, one
        shadow packet per point light, reflections=True = gVals[7]), staged on the device; returns the interleaved [resy,resx,3] uint8
        (B,G,R) frame.  snail_instances_render_whitted_dev."""
        torch = _torch()
        if out is None:
            out = torch.zeros((resy, resx, 3), dtype=torch.uint8, device=self._dev())
        lights = np.ascontiguousarray(lights7 if lights7 is not None else np.zeros((0, 7)), dtype=np.float32).reshape(-1, 7)
        cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32)
        amb = np.ascontiguousarray(ambient, dtype=np.float32); col = np.ascontiguousarray(color, dtype=np.float32)
        rc = _lib.lib().snail_instances_render_whitted_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(lights) if len(lights) else None, len(lights),
                                                          _lib.ptr(amb), _lib.ptr(col), 1 if reflections else 0, _lib.ptr(out), resx * 3, _lib.ptr(stats),
                                                          _stream_ptr(stream))
        _lib.check(rc, "snail_instances_render_whitted_dev")
        return out

    def render_whitted_packets(self, cam, resx: int, resy: int, packet_xy, lights7, ambient=(0.1, 0.1, 0.1), color=(1.0, 1.0, 1.0), out=None, stats=None,
                               stream=None, reflections: bool = False):
        """render_whitted for an explicit packet list (int32 [n,2] device tensor): packet-major [n,256,3] uint8 (B,G,R)."""
        torch = _torch()
        n = int(packet_xy.shape[0])
        if out is None:
            out = torch.empty((n, 256, 3), dtype=torch.uint8, device=self._dev())
        lights = np.ascontiguousarray(lights7 if lights7 is not None else np.zeros((0, 7)), dtype=np.float32).reshape(-1, 7)
        cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32)
        amb = np.ascontiguousarray(ambient, dtype=np.float32); col = np.ascontiguousarray(color, dtype=np.float32)
        rc = _lib.lib().snail_instances_render_whitted_packets_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(packet_xy), n,
                                                                  _lib.ptr(lights) if len(lights) else None, len(lights), _lib.ptr(amb), _lib.ptr(col),
                                                                  1 if reflections else 0, _lib.ptr(out), _lib.ptr(stats), _stream_ptr(stream))
        _lib.check(rc, "snail_instances_render_whitted_packets_dev")
        return out

    RENDER_REFLECTIONS, RENDER_DEPTH, RENDER_AA4 = 1, 2, 4     # include/snail_hip.h: flags of the host-pointer image call

    def render_image_host(self, cam, resx: int, resy: int, lights7=None, flags: int = 0, ambient=(0.1, 0.1, 0.1), color=(1.0, 1.0, 1.0)):
        """snail_instances_render_image = Render(scene, camera, image, options, threads) for an instanced scene: the rgb8 frame
        [resy, resx, 3] (B,G,R) in host memory and the call's TreeStats.  flags: RENDER_REFLECTIONS (gVals[7]), RENDER_DEPTH (gVals[1]);
        RENDER_AA4 is refused."""
        lights = np.ascontiguousarray(lights7 if lights7 is not None else np.zeros((0, 7)), dtype=np.float32).reshape(-1, 7)
        cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32)
        amb = np.ascontiguousarray(ambient, dtype=np.float32); col = np.ascontiguousarray(color, dtype=np.float32)
        img = np.zeros((resy, resx, 3), dtype=np.uint8)
        stats = np.zeros(4, dtype=np.uint64)
        rc = _lib.lib().snail_instances_render_image(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(lights) if len(lights) else None, len(lights),
                                                    _lib.ptr(amb), _lib.ptr(col), int(flags), _lib.ptr(img), resx * 3, _lib.ptr(stats))
        _lib.check(rc, "snail_instances_render_image")
        return img, stats

    @staticmethod
    def _shade_args(cam, lights7, ambient, color, tint):
        lights = np.ascontiguousarray(lights7 if lights7 is not None else np.zeros((0, 7)), dtype=np.float32).reshape(-1, 7)
        cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32)
        amb = np.ascontiguousarray(ambient, dtype=np.float32); col = np.ascontiguousarray(color, dtype=np.float32)
        tnt = None if tint is None else np.ascontiguousarray(tint, dtype=np.float32).reshape(3)
        return lights, cam13, amb, col, tnt

    def shade_packets(self, cam, resx: int, resy: int, packet_xy, lights7=None, flags: int = 0, tint=None, ambient=(0.1, 0.1, 0.1), color=(1.0, 1.0, 1.0),
                      out=None, stats=None, stream=None):
        """snail_instances_shade_packets_dev: the packets of an explicit list (int32 [n,2] device tensor) with any of RENDER_REFLECTIONS /
        RENDER_DEPTH / RENDER_AA4 and an optional tint (three factors, gVals[8]): packet-major [n,256,3] uint8 (B,G,R)."""
        torch = _torch()
        n = int(packet_xy.shape[0])
        if out is None:
            out = torch.empty((n, 256, 3), dtype=torch.uint8, device=self._dev())
        lights, cam13, amb, col, tnt = self._shade_args(cam, lights7, ambient, color, tint)
        rc = _lib.lib().snail_instances_shade_packets_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(packet_xy), n, _lib.ptr(lights) if len(lights) else None,
                                                         len(lights), _lib.ptr(amb), _lib.ptr(col), int(flags), _lib.ptr(tnt), _lib.ptr(out), _lib.ptr(stats),
                                                         _stream_ptr(stream))
        _lib.check(rc, "snail_instances_shade_packets_dev")
        return out

    def render_tiles_host(self, cam, resx: int, resy: int, tiles, lights7=None, flags: int = 0, tint=None, ambient=(0.1, 0.1, 0.1), color=(1.0, 1.0, 1.0),
                          offsets=None, data=None):
        """snail_instances_render_tiles: the tile-list renderer of src/render.h:16-19 for an instanced scene.  tiles = [n, 4] (x, y, w, h);
        returns (data, offsets, stats) with tile k's planes R, G-R, B-R at data[offsets[k]:offsets[k] + 3 w h], laid out like
        Scene.render_tiles_host (back to back) unless the caller brings `offsets` and a `data` buffer of its own.  tint = three factors
        (gVals[8]) or None."""
        t = np.ascontiguousarray(tiles, dtype=np.int32).reshape(-1, 4)
        size = 3 * t[:, 2].astype(np.int64) * t[:, 3]
        if offsets is None:
            offsets = np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.int64)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if data is None:
            data = np.zeros(int((offsets + size).max()) if len(t) else 0, dtype=np.uint8)
        lights, cam13, amb, col, tnt = self._shade_args(cam, lights7, ambient, color, tint)
        stats = np.zeros(4, dtype=np.uint64)
        rc = _lib.lib().snail_instances_render_tiles(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(t), _lib.ptr(offsets), len(t), _lib.ptr(lights) if len(lights) else None,
                                                    len(lights), _lib.ptr(amb), _lib.ptr(col), int(flags), _lib.ptr(tnt), _lib.ptr(data), _lib.ptr(stats))
        _lib.check(rc, "snail_instances_render_tiles")
        return data, offsets, stats

    def render_frame_host(self, cam, resx: int, resy: int, lights7=None, flags: int = 0, ambient=(0.1, 0.1, 0.1), color=(1.0, 1.0, 1.0)):
        """snail_instances_render_frame: render_image_host with RENDER_AA4 accepted (gVals[9]) -> (rgb8 frame [resy, resx, 3] (B,G,R), stats)."""
        lights, cam13, amb, col, _ = self._shade_args(cam, lights7, ambient, color, None)
        img = np.zeros((resy, resx, 3), dtype=np.uint8)
        stats = np.zeros(4, dtype=np.uint64)
        rc = _lib.lib().snail_instances_render_frame(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(lights) if len(lights) else None, len(lights), _lib.ptr(amb),
                                                    _lib.ptr(col), int(flags), _lib.ptr(img), resx * 3, _lib.ptr(stats))
        _lib.check(rc, "snail_instances_render_frame")
        return img, stats

    # ---- include/snail_heatmap.h: per-packet TreeStats and the reference's gVals[5] heat-map ------------------------------------------
    def _heat_args(self, cam, lights7, tint):
        lights, cam13, _, _, tnt = self._shade_args(cam, lights7, (0, 0, 0), (0, 0, 0), tint)
        return lights, (_lib.ptr(lights) if len(lights) else None), cam13, tnt

    def packet_stats(self, cam, resx: int, resy: int, packet_xy=None, lights7=None, reflections: bool = False, out=None, stats=None, stream=None, flags: int = 0):
        """snail_instances_packet_stats_dev: the TreeStats {intersects, iterations, rays, skips} of every packet's RayTrace call as an int32
        device tensor [n, 4] holding uint32 words.  packet_xy = int32 device tensor [n, 2], or None = the frame's grid, row-major."""
        torch = _torch()
        n = int(packet_xy.shape[0]) if packet_xy is not None else ((resx + 15) // 16) * ((resy + 15) // 16)
        if out is None:
            out = torch.zeros((n, 4), dtype=torch.int32, device=self._dev())
        lights, lp, cam13, _ = self._heat_args(cam, lights7, None)
        rc = _lib.lib().snail_instances_packet_stats_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(packet_xy), n, lp, len(lights),
                                                        int(flags) | (self.RENDER_REFLECTIONS if reflections else 0), _lib.ptr(out), _lib.ptr(stats), _stream_ptr(stream))
        _lib.check(rc, "snail_instances_packet_stats_dev")
        return out

    def render_heat_packets(self, cam, resx: int, resy: int, packet_xy=None, lights7=None, flags: int = 0, tint=None, out=None, packet_stats=None, stats=None,
                            stream=None):
        """snail_instances_heat_packets_dev: the heat-map of the packets, packet-major [n, 256, 3] uint8 (B,G,R).  flags: RENDER_REFLECTIONS,
        RENDER_AA4; tint = three factors (gVals[8]) or None; packet_stats (optional) int32 device tensor [n, 4] ([n, 4, 4] with RENDER_AA4)."""
        torch = _torch()
        n = int(packet_xy.shape[0]) if packet_xy is not None else ((resx + 15) // 16) * ((resy + 15) // 16)
        if out is None:
            out = torch.empty((n, 256, 3), dtype=torch.uint8, device=self._dev())
        lights, lp, cam13, tnt = self._heat_args(cam, lights7, tint)
        rc = _lib.lib().snail_instances_heat_packets_dev(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(packet_xy), n, lp, len(lights), int(flags), _lib.ptr(tnt),
                                                        _lib.ptr(out), _lib.ptr(packet_stats), _lib.ptr(stats), _stream_ptr(stream))
        _lib.check(rc, "snail_instances_heat_packets_dev")
        return out

    def render_heat_tiles_host(self, cam, resx: int, resy: int, tiles, lights7=None, flags: int = 0, tint=None):
        """snail_instances_render_heat_tiles: render_tiles_host with gVals[5] -> (data, offsets, stats)."""
        t = np.ascontiguousarray(tiles, dtype=np.int32).reshape(-1, 4)
        size = 3 * t[:, 2].astype(np.int64) * t[:, 3]
        offsets = np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.int64)
        data = np.zeros(int(size.sum()), dtype=np.uint8)
        lights, lp, cam13, tnt = self._heat_args(cam, lights7, tint)
        stats = np.zeros(4, dtype=np.uint64)
        rc = _lib.lib().snail_instances_render_heat_tiles(self._h, _lib.ptr(cam13), resx, resy, _lib.ptr(t), _lib.ptr(offsets), len(t), lp, len(lights), int(flags),
                                                         _lib.ptr(tnt), _lib.ptr(data), _lib.ptr(stats))
        _lib.check(rc, "snail_instances_render_heat_tiles")
        return data, offsets, stats

    def render_heat_frame_host(self, cam, resx: int, resy: int, lights7=None, flags: int = 0, pitch: int | None = None, fill: int = 0):
        """snail_instances_render_heat_frame: render_frame_host with gVals[5] -> (rgb8 frame [resy, resx, 3], or the rows [resy, pitch] when a
        pitch is given -- the bytes between rows keep `fill` --, stats)."""
        lights, lp, cam13, _ = self._heat_args(cam, lights7, None)
        p = resx * 3 if pitch is None else int(pitch)
        img = np.full((resy, max(p, 0)), fill, dtype=np.uint8)
        stats = np.zeros(4, dtype=np.uint64)
        rc = _lib.lib().snail_instances_render_heat_frame(self._h, _lib.ptr(cam13), resx, resy, lp, len(lights), int(flags), _lib.ptr(img), p, _lib.ptr(stats))
        _lib.check(rc, "snail_instances_render_heat_frame")
        return (img if pitch is not None else img.reshape(resy, resx, 3)), stats

    def traverse_primary(self, ctx: Context, element, stats=None, stream=None) -> Context:
        """DBVH::TraversePrimary<shared_origin, mask>: ctx.distance / ctx.object (= instance slot) / element (= triId) / ctx.barycentric
        (may be None) IN/OUT."""
        rc = _lib.lib().snail_instances_trace_rays_dev(self._h, ctx.n_packets, ctx.size, int(ctx.shared_origin), _lib.ptr(ctx.origin), _lib.ptr(ctx.dir),
                                                      _lib.ptr(ctx.idir), _lib.ptr(ctx.mask), _lib.ptr(ctx.distance), _lib.ptr(ctx.object), _lib.ptr(element),
                                                      _lib.ptr(ctx.barycentric), _lib.ptr(stats), _stream_ptr(stream))
        _lib.check(rc, "snail_instances_trace_rays_dev")
        return ctx

    def traverse_shadow(self, ctx: ShadowContext, stats=None, stream=None) -> ShadowContext:
        rc = _lib.lib().snail_instances_trace_shadow_dev(self._h, ctx.n_packets, ctx.size, _lib.ptr(ctx.origin), _lib.ptr(ctx.dir), _lib.ptr(ctx.idir),
                                                        _lib.ptr(ctx.distance), _lib.ptr(stats), _stream_ptr(stream))
        _lib.check(rc, "snail_instances_trace_shadow_dev")
        return ctx


__all__ = ["InstancedScene", "build_instances", "HitFrame"]
