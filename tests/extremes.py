"""Scenes, cameras and packets moved into the numeric regimes the near-origin workloads never reach: scaled by 2^k (exact in
float32 while nothing under- or overflows) or translated far from the origin.  Shared by tests/test_oracle_scale.py (what the
oracle does there) and tests/test_gpu_extremes.py (the kernels against the oracle there)."""
from __future__ import annotations

import functools

import numpy as np

from snail_amd import HostBVH, scenes
from snail_amd.camera import Camera
from tests import oracle_lib as O
from tests import util

F32 = np.float32


def pow2(k: int) -> np.float32:
    return F32(np.ldexp(1.0, k))


@functools.lru_cache(maxsize=64)
def scaled_pair(name: str, k: int):
    """(tri_verts * 2^k, HostBVH, OracleScene) -- the multiplication is exact for every vertex that stays normal and finite."""
    tv = (scenes.scene_by_name(name).astype(F32) * pow2(k)).astype(F32)
    return tv, HostBVH.build(tv), O.OracleScene(tv)


@functools.lru_cache(maxsize=16)
def moved_pair(name: str, k: int, off: tuple):
    """(tri_verts * 2^k + off, HostBVH, OracleScene): the addition rounds once the offset dwarfs the scene"""
    tv = ((scenes.scene_by_name(name).astype(F32) * pow2(k)).astype(F32) + np.asarray(off, dtype=F32)).astype(F32)
    return tv, HostBVH.build(tv), O.OracleScene(tv)


def base_camera(name: str) -> Camera:
    return util.camera_for(name, scenes.scene_by_name(name))


def scaled_camera(name: str, k: int) -> Camera:
    c = base_camera(name)
    return Camera((c.pos * pow2(k)).astype(F32), c.right, c.up, c.front, c.plane_dist)


def moved_camera(cam: Camera, k: int, off, dolly: float = 0.0) -> Camera:
    """cam's position times 2^k plus off, then moved by dolly * 2^k along its front vector"""
    pos = ((cam.pos * pow2(k)).astype(F32) + np.asarray(off, dtype=F32)).astype(F32)
    pos = (pos + F32(dolly) * pow2(k) * cam.front).astype(F32)
    return Camera(pos, cam.right, cam.up, cam.front, cam.plane_dist)


def fast_ok(tris, nodes) -> bool:
    """numpy restatement of snail_scene_create's fastOK rule: every triangle record and node bound finite and of bounded magnitude,
    node boxes not inverted (NaN fails every comparison, as there)."""
    with np.errstate(invalid="ignore"):
        t = np.asarray(tris).view(O.TRI_DTYPE)
        n = np.asarray(nodes).view(O.NODE_DTYPE)
        ok = (np.abs(t["a"]) <= F32(1e9)).all() and (np.abs(t["ba"]) <= F32(1e9)).all() and (np.abs(t["ca"]) <= F32(1e9)).all()
        ok = ok and (t["t0"] > 0).all() and (t["it0"] <= F32(1e12)).all() and (t["it0"] > 0).all()
        ok = ok and (np.abs(t["plane"]) <= F32(1e18)).all()
        ok = ok and (np.abs(n["bmin"]) <= F32(1e9)).all() and (np.abs(n["bmax"]) <= F32(1e9)).all() and (n["bmin"] <= n["bmax"]).all()
    return bool(ok)


def origin_sane(o) -> bool:
    """originSane / originSaneDev: the primary and light stages take M_FAST / M_COH only from origins of magnitude <= 1e9."""
    return bool((np.abs(np.asarray(o, dtype=F32)) <= F32(1e9)).all())


def lights_for(osc, cam: Camera) -> np.ndarray:
    """One light above the scene's centre, its radius relative to the scene (scales with it)."""
    bmin, bmax = osc.nodes[0]["bmin"], osc.nodes[0]["bmax"]
    c, e = (bmin + bmax) * F32(0.5), (bmax - bmin)
    return np.array([[c[0], c[1] + F32(0.35) * e[1], c[2], 1.0, 0.9, 0.8, F32(2.0) * e.max()]], dtype=F32)


def scaled_lights(name: str, k: int) -> np.ndarray:
    """The k = 0 light with position and radius times 2^k (so lights-only frames scale exactly where the oracle's absolute constants allow)."""
    tv, hb, osc = scaled_pair(name, 0)
    L = lights_for(osc, base_camera(name)).copy()
    L[:, 0:3] *= pow2(k)
    L[:, 6] *= pow2(k)
    return L


def generic_packets(name: str, k: int, shared: bool, masked: bool, size: int, npk: int = 4, seed: int = 7):
    """util.secondary_packets of the k = 0 scene with origins times 2^k (directions, idir, masks unchanged)."""
    tv, hb, osc = scaled_pair(name, 0)
    cam = base_camera(name)
    origin, dirs, idir, mask, dist, obj, bary = util.secondary_packets(osc, cam, 160, 96, npk, seed=seed, shared=shared, masked=masked, size=size)
    return (origin * pow2(k)).astype(F32), dirs, idir, mask, dist, obj, bary


def shadow_packets_scaled(name: str, k: int, npk: int = 4, seed: int = 3, size: int = 64):
    """util.shadow_packets of the k = 0 scene with light positions and distances times 2^k."""
    tv, hb, osc = scaled_pair(name, 0)
    origin, dirs, idir, dist = util.shadow_packets(osc, npk, seed=seed, size=size)
    return (origin * pow2(k)).astype(F32), dirs, idir, (dist * pow2(k)).astype(F32)


def run_rays(osc, pk, npk, size, shared, mode):
    origin, dirs, idir, mask, dist, obj, bary = pk
    d2, o2, b2 = dist.copy(), obj.copy(), bary.copy()
    st = osc.trace_rays(origin, dirs, idir, mask, d2, o2, b2, npk, size, shared, mode=mode)
    return d2, o2, b2, st


def run_shadow(osc, pk, npk, size, mode):
    origin, dirs, idir, dist = pk
    d2 = dist.copy()
    st = osc.trace_shadow(origin, dirs, idir, d2, npk, size, mode=mode)
    return d2, st


def scaled_tree_equals(nodes0, nodes_k, k: int) -> bool:
    """nodes_k is nodes0 with every bound times 2^k and the same child / leaf structure."""
    return (np.array_equal(nodes0["sub"], nodes_k["sub"]) and np.array_equal(nodes0["aux"], nodes_k["aux"])
            and util.bits((nodes0["bmin"] * pow2(k)).astype(F32)).tobytes() == util.bits(nodes_k["bmin"]).tobytes()
            and util.bits((nodes0["bmax"] * pow2(k)).astype(F32)).tobytes() == util.bits(nodes_k["bmax"]).tobytes())
