"""Edge cases of the instanced walk (include/snail_instances.h), as plain builders shared by tests/test_instances_edges_host.py (the
restatement on these cases, and the proof that each case reaches the edge it is named for) and tests/test_gpu_instances_edges.py (the
device against the restatement, bit for bit).  Nothing here touches a device: a Case holds arrays only, expected values come from
tests/dbvh_ref.py over the oracle's BLAS scenes."""
from __future__ import annotations

import itertools
import os
import types

import numpy as np

from snail_amd import scenes
from snail_amd.camera import Camera
from snail_amd.instances import build_instances
from tests import dbvh_ref as R
from tests import oracle_lib as O
from tests import util as U

F = np.float32
GOLD = os.path.join(os.path.dirname(__file__), "golden")
ARITH = [("ieee", O.MODE_IEEE), ("host_sse", O.MODE_SSE)]
EPS = F(0.00000001)                                 # SafeInv's addend (src/rtbase.h:117-120)

_tris, _oracles = {}, {}


def blas_tris(name):
    """Triangles [n, 9] of a BLAS: box, lancia (the reference's own mesh), chain (depth 63: the DEEP walk), and unit = the box scene
    mapped onto [0, 1]^3 (an extent below one ulp of a translation of 2^24)."""
    if name not in _tris:
        if name == "lancia":
            tv = np.load(os.path.join(GOLD, "lancia_tris.npz"))["tris"].reshape(-1, 9).astype(np.float32)
        elif name == "chain":
            tv = scenes.chain()
        elif name == "unit":
            tv = ((scenes.box_scene().astype(np.float32) + F(1.0)) * F(0.5)).astype(np.float32)
        else:
            tv = scenes.scene_by_name(name)
        _tris[name] = np.ascontiguousarray(tv, dtype=np.float32)
    return _tris[name]


def oracle(name):
    if name not in _oracles:
        _oracles[name] = O.OracleScene(blas_tris(name))
    return _oracles[name]


def bbox6(names):
    return np.stack([np.concatenate([oracle(nm).nodes[0]["bmin"], oracle(nm).nodes[0]["bmax"]]) for nm in names]).astype(np.float32)


class Case:
    """An instanced scene as arrays: `names` = its BLASes; rot / tr / bi = the instances in the caller's order; nodes / xs / bs = the
    top-level tree and the records in builder-slot order (the host builder's over (rot, tr, bi), or -- tree=True -- a caller's tree)."""

    def __init__(self, key, names, rot, tr, bi=None, nodes=None):
        self.key, self.names = key, list(names)
        self.rot = np.ascontiguousarray(rot, dtype=np.float32).reshape(-1, 3, 3)
        self.tr = np.ascontiguousarray(tr, dtype=np.float32).reshape(-1, 3)
        n = len(self.rot)
        self.bi = np.zeros(n, dtype=np.int32) if bi is None else np.ascontiguousarray(bi, dtype=np.int32).reshape(-1)
        self.xf = np.ascontiguousarray(np.concatenate([self.rot.reshape(-1, 9), self.tr], axis=1), dtype=np.float32)
        self.tree = nodes is not None
        if self.tree:
            self.nodes, self.perm = np.ascontiguousarray(nodes), np.arange(n, dtype=np.int32)
        else:
            self.nodes, self.depth, self.perm = build_instances(self.xf, self.bi, bbox6(self.names))
        self.xs, self.bs = np.ascontiguousarray(self.xf[self.perm]), np.ascontiguousarray(self.bi[self.perm])
        self._ref = None

    def ref(self):
        if self._ref is None:
            self._ref = R.Ref([oracle(nm) for nm in self.names], self.nodes, self.xs, self.bs)
        return self._ref

    def world(self):
        """what util.secondary_packets / util.shadow_packets want of a scene: its root box"""
        return types.SimpleNamespace(nodes=self.nodes)


# ---- cameras ---------------------------------------------------------------------------------------------------------------------------
def axis_camera(pos, axis, sign):
    """Looking exactly along +-e_axis: right and up are the two other unit vectors, so rays through the image centre have exact zeros."""
    e = np.eye(3, dtype=np.float32)
    return Camera(np.asarray(pos, dtype=np.float32), e[(axis + 1) % 3], e[(axis + 2) % 3], e[axis] * F(sign), 1.0)


def look_at(pos, target):
    pos, target = np.asarray(pos, dtype=np.float64), np.asarray(target, dtype=np.float64)
    f = target - pos
    f /= np.linalg.norm(f)
    up0 = np.array([0.0, 1.0, 0.0]) if abs(f[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    r = np.cross(up0, f)
    r /= np.linalg.norm(r)
    return Camera(pos.astype(np.float32), r.astype(np.float32), np.cross(f, r).astype(np.float32), f.astype(np.float32), 1.0)


def pixel_dir(cam, resx, resy, x, y):
    """the direction (not normalised) the ray generator gives pixel (x, y): right (x - w/2)/h + up (y - h/2)/h + front plane_dist"""
    c = np.asarray(cam.as_array13(), dtype=np.float64)
    return c[3:6] * ((x - resx * 0.5) / resy) + c[6:9] * ((y - resy * 0.5) / resy) + c[9:12] * c[12]


def grid_packets(resx, resy):
    return np.array([(x, y) for y in range(0, resy, 16) for x in range(0, resx, 16)], dtype=np.int32).reshape(-1, 2)


def scatter_packets(planes, packet_xy, resx, resy, miss=(np.inf, 0, 0, 0, 0)):
    """packet-major [n, 256] planes -> frames [resy, resx], pixels beyond the edge dropped"""
    out = []
    for pl, m in zip(planes, miss):
        fr = np.full((resy, resx), m, dtype=pl.dtype)
        for i, (px, py) in enumerate(np.asarray(packet_xy).tolist()):
            blk = pl[i].reshape(16, 16)
            h, w = max(0, min(16, resy - py)), max(0, min(16, resx - px))
            fr[py:py + h, px:px + w] = blk[:h, :w]
        out.append(fr)
    return out


# ---- expected values: computed once per (case, view, arithmetic), shared by the tests of both files ---------------------------------------
_expected = {}


def expected_frame(case, cam, resx, resy, mode, rect=None):
    k = ("frame", case.key, np.asarray(cam.as_array13()).tobytes(), resx, resy, mode, rect)
    if k not in _expected:
        _expected[k] = case.ref().render_primary(cam.as_array13(), resx, resy, mode=mode, rect=rect)
    return _expected[k]


def expected_packets(case, cam, resx, resy, packet_xy, mode):
    xy = np.ascontiguousarray(packet_xy, dtype=np.int32)
    k = ("packets", case.key, np.asarray(cam.as_array13()).tobytes(), resx, resy, mode, xy.tobytes())
    if k not in _expected:
        _expected[k] = case.ref().render_packets(cam.as_array13(), resx, resy, xy, mode)
    return _expected[k]


# ---- partial frames, rects, packet lists -------------------------------------------------------------------------------------------------
PARTIAL_SIZES = [(1, 1), (5, 3), (16, 16), (17, 33), (100, 7), (129, 65)]
RECT_FRAME = (100, 70)
RECTS = [(16, 16, 40, 30), (0, 0, 16, 64), (48, 32, 21, 24), (96, 64, 16, 16), (64, 0, 100, 16)]
_cases = {}


def blob():
    """Two BLASes, 12 instances squeezed around the origin (tests/test_gpu_instances.py::make's field with a small spread): a camera inside
    it sees a hit in nearly every direction, which the wide rays of a 1 x 1 or 100 x 7 frame need."""
    if "blob" not in _cases:
        names = ["box", "lancia"]
        bb = bbox6(names)
        rot, tr, bi = scenes.instance_field(bb[:, :3].min(axis=0), bb[:, 3:].max(axis=0), 12, seed=17, n_blas=2)
        _cases["blob"] = Case("blob", names, rot, (tr * F(0.02)).astype(np.float32), bi)
    return _cases["blob"]


def blob_camera():
    from snail_amd import FPSCamera
    return FPSCamera(np.array([0.3, 0.2, -0.1], dtype=np.float32), 0.4, 0.2).camera()


def packet_list(resx, resy):
    """the grid's packets in reverse order, one packet twice, then the packets of the right and bottom edges (partly outside) once more"""
    g = grid_packets(resx, resy)
    edge = g[(g[:, 0] + 16 > resx) | (g[:, 1] + 16 > resy)]
    return np.ascontiguousarray(np.concatenate([g[::-1], g[3:4], edge]), dtype=np.int32)


# ---- depth: combs --------------------------------------------------------------------------------------------------------------------------
def comb(depth, axis, far_first, name="box", step=2.5):
    """A caller's tree of `depth` levels over depth + 1 instances of one BLAS: identity rotations, translations k * step along `axis`;
    inner node k (record 2k) has the leaf of instance k (record 2k + 1) and the rest of the comb (record 2k + 2) as children, every box
    the exact union of its children's, aux = axis | firstNode << 16 with firstNode = 1 (the rest first for a ray going up the axis) when
    far_first.  -> Case (slot k = instance k).
    A walk that takes the rest first at every level pushes one leaf per level: `depth` stack entries, slots 0..depth - 1 of the first
    lane-indexed pair (tStkNode / tStkFL).  The second pair (tStkNode2 / tStkFL2, slots 64..127) would need a 65th push, i.e. a tree of
    more than SNAIL_INSTANCES_MAX_DEPTH = 64 levels, which snail_instances_create refuses: it cannot be reached, and no case tries."""
    n = depth + 1
    rot = np.tile(np.eye(3, dtype=np.float32), (n, 1, 1))
    tr = np.zeros((n, 3), dtype=np.float32)
    tr[:, axis] = np.arange(n, dtype=np.float32) * F(step)
    xf = np.concatenate([rot.reshape(-1, 9), tr], axis=1).astype(np.float32)
    bb = bbox6([name])[0]
    leaf_box = [R.instance_box(xf[k], bb) for k in range(n)]
    nodes = np.zeros(2 * depth + 1, dtype=R.NODE_DTYPE)

    def put(i, box, sub, aux):
        nodes[i]["bmin"], nodes[i]["bmax"], nodes[i]["sub"], nodes[i]["aux"] = box[0], box[1], sub, aux

    rest = leaf_box[depth]
    put(2 * depth, rest, 0x80000000 | depth, 1)
    for k in range(depth - 1, -1, -1):
        put(2 * k + 1, leaf_box[k], 0x80000000 | k, 1)
        rest = R.box_add(leaf_box[k], rest)
        put(2 * k, rest, 2 * k + 1, axis | ((1 if far_first else 0) << 16))
    return Case("comb-%d-%d-%d-%s" % (depth, axis, int(far_first), name), [name], rot, tr, nodes=nodes)


def comb_cameras(case, axis, side=24.0):
    """-> {"low": from below instance 0 looking up the axis, "high": from above the last instance looking down it, "side": across the
    comb's middle}.  The end-on cameras sit 0.25 / 0.125 off the comb's centre line and look exactly along the axis, so the ray through
    the image centre (lane 0 of the packet at (resx/2, resy/2)) passes through every instance."""
    lo, hi = case.nodes[0]["bmin"].astype(np.float64), case.nodes[0]["bmax"].astype(np.float64)
    c = (lo + hi) * 0.5
    off = np.zeros(3); off[(axis + 1) % 3], off[(axis + 2) % 3] = 0.25, 0.125
    p_lo, p_hi = c + off, c + off
    p_lo[axis], p_hi[axis] = lo[axis] - 6.0, hi[axis] + 6.0
    p_side = c.copy(); p_side[(axis + 1) % 3] += side; p_side[axis] += 0.75
    return {"low": axis_camera(p_lo, axis, 1.0), "high": axis_camera(p_hi, axis, -1.0), "side": axis_camera(p_side, (axis + 1) % 3, -1.0)}


def chain_comb():
    """comb(64) over the chain BLAS (its own depth takes the DEEP kernels) -> (Case, cameras); the chain is thin, so the side camera is near"""
    if "chain-comb" not in _cases:
        case = comb(64, 0, True, name="chain", step=16.0)
        _cases["chain-comb"] = (case, comb_cameras(case, 0, side=6.0))
    return _cases["chain-comb"]


def deep_camera(far_first):
    """the end-on camera from which the far child is the pushed one at every level of comb(., ., far_first)"""
    return "low" if far_first else "high"


# ---- octants ------------------------------------------------------------------------------------------------------------------------------
def octant_field():
    if "octants" not in _cases:
        bb = bbox6(["box"])
        rot, tr, bi = scenes.instance_field(bb[:, :3].min(axis=0), bb[:, 3:].max(axis=0), 12, seed=23)
        _cases["octants"] = Case("octants", ["box"], rot, (tr * F(0.2)).astype(np.float32), bi)
    return _cases["octants"]


def octant_cameras(case):
    """one camera per sign octant of the view direction, each looking at the field's centre from its far corner"""
    lo, hi = case.nodes[0]["bmin"].astype(np.float64), case.nodes[0]["bmax"].astype(np.float64)
    c, e = (lo + hi) * 0.5, (hi - lo)
    out = []
    for s in itertools.product((1.0, -1.0), repeat=3):
        s = np.array(s)
        out.append(look_at(c - s * e * np.array([0.9, 0.8, 1.0]), c + s * e * np.array([0.05, 0.1, 0.0])))
    return out


# ---- exact rotations ----------------------------------------------------------------------------------------------------------------------
def exact_rotations():
    """The 24 proper rotations of the cube group (signed permutation matrices of determinant +1), then four improper ones: the first four
    proper ones with the sign of one row flipped.  float32 [28, 3, 3], every entry exactly 0 or +-1."""
    proper = []
    for p in itertools.permutations(range(3)):
        for s in itertools.product((1.0, -1.0), repeat=3):
            m = np.zeros((3, 3))
            for r in range(3):
                m[r, p[r]] = s[r]
            if np.linalg.det(m) > 0:
                proper.append(m)
    assert len(proper) == 24
    improper = []
    for k in range(4):
        m = proper[5 * k + 1].copy()
        m[k % 3] *= -1.0
        improper.append(m)
    return np.array(proper + improper, dtype=np.float32)


def rotation_field():
    """28 instances of box, one per matrix of exact_rotations(), translations on a grid of 4 (x, y) and 2 (z): with the camera below on a
    grid of 0.5, org - T is exact."""
    if "rotations" not in _cases:
        rot = exact_rotations()
        tr = np.array([[4.0 * (i % 7) - 12.0, 4.0 * (i // 7) - 6.0, 2.0 * ((i * 5) % 3) - 2.0] for i in range(28)], dtype=np.float32)
        _cases["rotations"] = Case("rotations", ["box"], rot, tr)
    return _cases["rotations"]


def rotation_camera():
    """Looking exactly down +z from a point of the 0.5 grid: column resx/2 and row resy/2 of an even-sized frame have a direction
    component that is exactly 0, which an axis permutation carries to another inner axis, where SafeInv gives 1 / 1e-8."""
    return axis_camera(np.array([0.5, 0.0, -24.0], dtype=np.float32), 2, 1.0)


# ---- far field ----------------------------------------------------------------------------------------------------------------------------
FAR_K = [12, 20, 24]
FAR_AXES = [(0,), (0, 2), (0, 1, 2)]


def far_field(k, axes):
    """14 instances of the unit box around a camera 12 away, everything (translations and camera) shifted by 2^k on `axes`.  The positions
    are rounded to float32 after the shift: at k = 24 the spacing of floats is 2, twice the BLAS's extent.
    -> (Case, Camera, T64 [n, 3], org64 [3]): the last two are the positions before rounding."""
    key = "far-%d-%s" % (k, "".join(map(str, axes)))
    if key not in _cases:
        rng = np.random.default_rng(100 + k)
        n = 14
        rot, _, _ = scenes.instance_field((0, 0, 0), (1, 1, 1), n, seed=3)
        base = np.stack([rng.uniform(-3.0, 3.0, n), rng.uniform(-2.0, 2.0, n), rng.uniform(-1.5, 1.5, n)], axis=1)
        base = np.round(base * 64.0) / 64.0
        shift = np.zeros(3)
        shift[list(axes)] = 2.0 ** k
        t64 = base + shift
        org64 = np.array([0.28125, 0.40625, -12.0]) + shift
        case = Case(key, ["unit"], rot, t64.astype(np.float32))
        cam = axis_camera(org64.astype(np.float32), 2, 1.0)
        _cases[key] = (case, cam, t64, org64)
    return _cases[key]


# ---- duplicates ---------------------------------------------------------------------------------------------------------------------------
def _dup_transform():
    rot, tr, _ = scenes.instance_field((-1, -1, -1), (1, 1, 1), 3, seed=29)
    return rot[0], (tr[0] * F(0.1)).astype(np.float32)


def duplicates():
    """-> list of (Case, number of duplicates): one transform and BLAS 2, 3 and 9 times (9 coincident centres: 16 bins over an extent of 0,
    every centre in bin 0 by the deviation rule, median splits), then the 3 and the 9 mixed into a field of 8 distinct instances."""
    if "dups" not in _cases:
        r0, t0 = _dup_transform()
        out = []
        for m in (2, 3, 9):
            out.append((Case("dup-%d" % m, ["box"], np.tile(r0, (m, 1, 1)), np.tile(t0, (m, 1))), m))
        rot, tr, _ = scenes.instance_field((-1, -1, -1), (1, 1, 1), 8, seed=31)
        tr = (tr * F(0.25)).astype(np.float32)
        for m in (3, 9):
            # the duplicates interleaved with the distinct ones, not in a block
            rr, tt = list(rot), list(tr)
            for j in range(m):
                rr.insert((2 * j) % len(rr), r0); tt.insert((2 * j) % len(tt), t0)
            out.append((Case("dup-%d-mixed" % m, ["box"], np.array(rr), np.array(tt)), m))
        _cases["dups"] = out
    return _cases["dups"]


def duplicates_camera(case):
    r0, t0 = _dup_transform()
    lo, hi = case.nodes[0]["bmin"].astype(np.float64), case.nodes[0]["bmax"].astype(np.float64)
    back = max(6.0, 1.2 * float((hi - lo).max()))
    return look_at(t0.astype(np.float64) + np.array([0.4, 0.3, -back]), t0)


# ---- singular packets ---------------------------------------------------------------------------------------------------------------------
def singular_field():
    """Identity and the five other axis permutations (three of them improper), box each, so that a component of the outer direction
    arrives on each inner axis."""
    if "singular" not in _cases:
        rot = []
        for p in itertools.permutations(range(3)):
            m = np.zeros((3, 3), dtype=np.float32)
            for r in range(3):
                m[r, p[r]] = 1.0
            rot.append(m)
        tr = np.array([[0, 0, 0], [1.25, 0.25, 0], [-1.25, 0, 0.25], [0, 1.25, 0.25], [0.25, -1.25, 0], [0, 0.25, 1.25]], dtype=np.float32)   # overlapping
        _cases["singular"] = Case("singular", ["box"], np.array(rot), tr)
    return _cases["singular"]


def _recompute_idir(d, mode):
    with np.errstate(all="ignore"):
        return R.inv((d + EPS).astype(np.float32), mode)


def _edit_dirs(d, size, n_packets):
    """packet p: quads 0, size // 3 and size - 1 get component p % 3 = -1e-8 (all four lanes), quad size // 2 gets component (p + 1) % 3 =
    0.0.  -> the quads edited, per packet"""
    edited = []
    for p in range(n_packets):
        qs = sorted({0, size // 3, size - 1})
        c = p % 3
        for q in qs:
            d[p * size + q, 4 * c:4 * c + 4] = F(-0.00000001)
        z = size // 2
        if z not in qs:
            c0 = (p + 1) % 3
            d[p * size + z, 4 * c0:4 * c0 + 4] = F(0.0)
        edited.append(qs)
    return edited


# seeds of the packet generators, searched on the host (0, 1, 2, ...) for the first at which the non-vacuity assertions of
# tests/test_instances_edges_host.py hold: an edited quad hits an instance, resp. is occluded by one
SINGULAR_SEEDS = {(64, True, False): 0, (64, True, True): 1, (64, False, False): 0, (64, False, True): 0,
                  (16, True, False): 0, (16, True, True): 3, (16, False, False): 0, (16, False, True): 0}
SINGULAR_SHADOW_SEEDS = {64: 0, 16: 13}


def singular_packets(case, size, shared, masked, mode, seed=None):
    """Generic packets (util.secondary_packets) with singular directions: where a component is exactly -1e-8, SafeInv is Inv(0) (inf in
    IEEE; rcpps' inf through the Newton step in the SSE arithmetic).  The origin of such a quad (of the packet, when the origin is shared)
    is put on the root box's lower plane on that axis, so that the top-level box test multiplies the singular idir by exactly 0.
    -> (org, d, idir, mask, dist, obj, bary, edited quads per packet)"""
    n_packets = 3
    seed = SINGULAR_SEEDS[(size, bool(shared), bool(masked))] if seed is None else seed
    org, d, idir, mask, dist, obj, bary = U.secondary_packets(case.world(), None, 0, 0, n_packets, seed=seed + size + 7 * shared + 3 * masked,
                                                              shared=shared, masked=masked, size=size)
    edited = _edit_dirs(d, size, n_packets)
    lo = case.nodes[0]["bmin"]
    for p in range(n_packets):
        c = p % 3
        if shared:
            org[p, 4 * c:4 * c + 4] = lo[c]
        else:
            for q in edited[p]:
                org[p * size + q, 4 * c:4 * c + 4] = lo[c]
        if mask is not None:
            for q in edited[p]:
                mask[p * size + q] = 15          # (packet 1, which util leaves dead, lives in its singular quads alone)
    if mask is not None:
        lanes = (mask[:, None] >> np.arange(4)[None, :]) & 1
        dist[:] = np.where(lanes == 0, -np.inf, np.inf).astype(np.float32)
    return org, d, _recompute_idir(d, mode), mask, dist, obj, bary, edited


def singular_shadow_packets(case, size, mode, seed=None):
    n_packets = 3
    seed = SINGULAR_SHADOW_SEEDS[size] if seed is None else seed
    org, d, idir, dist = U.shadow_packets(case.world(), n_packets, seed=seed + size, size=size)
    edited = _edit_dirs(d, size, n_packets)
    lo = case.nodes[0]["bmin"]
    for p in range(n_packets):
        org[p, p % 3] = lo[p % 3]
        if p == 2:
            dist[p * size:(p + 1) * size] = F(5.0)          # (util leaves packet 2 fully masked)
        for q in edited[p]:
            dist[p * size + q] = F(7.5)
    return org, d, _recompute_idir(d, mode), dist, edited


# ---- the restatement over packet batches ----------------------------------------------------------------------------------------------------
def ref_generic(ref, org, d, idir, mask, dist, obj, elem, bary, size, shared, mode):
    """Ref.traverse over every packet of a Context batch, in place -> TreeStats"""
    st = np.zeros(4, dtype=np.uint64)
    for p in range(len(d) // size):
        sl = slice(p * size, (p + 1) * size)
        po = org[p:p + 1].reshape(1, 3, 4) if shared else org[sl].reshape(size, 3, 4)
        st += ref.traverse(po, d[sl].reshape(size, 3, 4), idir[sl].reshape(size, 3, 4), None if mask is None else mask[sl], dist[sl], obj[sl], elem[sl],
                           None if bary is None else bary[sl], shared, False, mode)
    return st


def ref_shadow(ref, org, d, idir, dist, size, mode):
    st = np.zeros(4, dtype=np.uint64)
    for p in range(len(d) // size):
        sl = slice(p * size, (p + 1) * size)
        po = np.repeat(org[p].reshape(1, 3, 1), 4, axis=2).astype(np.float32)
        st += ref.traverse(po, d[sl].reshape(size, 3, 4), idir[sl].reshape(size, 3, 4), None, dist[sl], None, None, None, True, True, mode)
    return st
