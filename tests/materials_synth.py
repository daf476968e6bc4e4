"""Synthetic hit records for the sample and mirror stages of full shading (tests/test_materials_synth_host.py, tests/test_gpu_materials_synth.py).
The stages take their hit records from the caller, so a test can hand them any record of the documented domain (include/snail_materials.h)
without building a scene whose traversal would produce it.  Here: ten texture shapes in one set (sides of 1, taller than wide, the 14-level
chains of 8192-wide and 8192-tall textures), a second set of the same shapes in constant grey, one TEX material per texture, SIMPLE and UBER
materials and the default behind a shuffled material map, a few hundred triangles' shading data (every map entry crossed with a class of texture
coordinates and with flat / not flat; normals of the lengths 0, 1e-20, ~1 and 1e3), and lists of packets whose 16 blocks follow one recipe
each.  The kernels under test never look at the geometry: the triangle soup exists to own the set and to supply the builder's permutation.
Seeded numpy, float32; nothing here touches the product library.

Left out: a texDiff product at or above 2^32 (the low-word truncation of uint(float) in the mip choice).  Min(texDiff.x * (w - 1),
texDiff.y * (h - 1)) * 0.6 reaches 2^32 only when BOTH sides are large: with |uv| < 2^20 it needs a texture of 4096 x 4096 or more, 50 MB or more
with its chain."""
from __future__ import annotations

import functools

import numpy as np

from tests import materials_bounce_ref as B
from tests import materials_cases as K
from tests import materials_ref as M
from tests import oracle_lib as O

F = np.float32
INF = F(np.inf)
SHAPES = [(1, 1), (2, 2), (1, 8), (8, 1), (8, 32), (32, 8), (8192, 2), (2, 8192), (4, 2048), (256, 256)]      # w x h, the order in the set
GREYS = [20 + 23 * k for k in range(len(SHAPES))]                 # the grey set: texture k is (g, g, g) everywhere, a different g per texture
FRAME = (70, 50)                                                   # 5 x 4 packets, the last column and row partial
N_PACKETS = 64
UV_MAX = 1048575.9375                                              # the largest float32 below 2^20
UV_CLASSES = ["unit", "int", "huge", "near", "span", "dyadic"]
NORMAL_LENGTHS = [0.0, 1e-20, 1.0, 1e3]
# the map: a shuffled list of the 14 materials and the default, so that a map index is never its material's index
MAP = [5, 12, 0, -1, 9, 3, 13, 1, 7, 10, 4, 2, 11, 8, 6]
GARBAGE_IDS = [2**31 - 1, -2**31, 1000000007, -1, -123456789]
# the camera of the primary lists: any will do (the sample stage reads directions only), slightly turned so that no component is exact
CAM13 = np.array([0.3, -0.2, -4.0, 0.96, 0.0, -0.28, 0.0, 1.0, 0.0, 0.28, 0.0, 0.96, 1.0], dtype=np.float32)


class Cam:
    """what MaterialSet's calls ask of a camera"""

    def as_array13(self):
        return CAM13


def levels_of(w, h):
    return len(M.level_shapes(w, h))


def noise_texture(w, h, seed):
    """uint8 [h, w, 3] of seeded noise: neighbouring texels, levels and textures all differ"""
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def material_descs(all_without_ndotr=False):
    """descriptions in the form of tests/materials_cases.py: one TEX per texture (with N.R for even textures, without for odd ones -- or all
    without), SIMPLE with and without N.R, UBER with dissolve 0 and 1"""
    d = [("tex", k, (k % 2 == 0) and not all_without_ndotr) for k in range(len(SHAPES))]
    d += [("simple", (0.9, 0.5, 0.2), True), ("simple", (0.3, 0.8, 0.6), False)]
    d += [("uber", (0.9, 0.4, 0.1), (0.2, 0.6, 1.0), 0.0), ("uber", (0.2, 0.7, 0.5), (1.0, 0.3, 0.1), 1.0)]
    return d


def ladder_scale(w, h, level):
    """s of a ladder triangle uv = (0,0), (s,0), (0,s): a quad whose barycentrics span 1/2 in both directions has texDiff = s / 2, so
    pixels = uint(0.3 s min(w - 1, h - 1)); s puts that in the middle of the level's range [2^(level-1), 2^level) (0.4 for level 0)"""
    want = 0.4 if level == 0 else 1.5 * 2.0 ** (level - 1)
    return want / (0.3 * min(w - 1, h - 1))


def ulps(v, k):
    v = F(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, F(np.inf) if k > 0 else F(-np.inf))
    return v


def clamp_ids(tri, n):
    """the header's rule for a triId outside the scene: below 0 becomes 0, n and above becomes n - 1"""
    return np.clip(np.asarray(tri, dtype=np.int64), 0, n - 1).astype(np.int32)


class Synth:
    def __init__(self):
        rng = np.random.RandomState(20261)
        self.textures = [noise_texture(w, h, 100 + k) for k, (w, h) in enumerate(SHAPES)]
        self.textures_grey = [np.full((h, w, 3), g, dtype=np.uint8) for (w, h), g in zip(SHAPES, GREYS)]
        self.descs = material_descs()
        self.descs_grey = material_descs(all_without_ndotr=True)
        self.material_map = list(MAP)
        assert sorted(MAP) == list(range(-1, len(self.descs)))
        self.default_entry = MAP.index(-1)
        entry_of_tex = {k: MAP.index(k) for k in range(len(SHAPES))}      # TEX material k is material k

        uv, nrm, entry, flat, meta = [], [], [], [], []

        def add(e, fl, u, cls, **kw):
            i = len(uv)
            uv.append(np.asarray(u, dtype=np.float64).reshape(3, 2)); entry.append(e); flat.append(bool(fl)); meta.append(dict(cls=cls, **kw))
            # normals: all three vertices of one length (triangle index mod 5 picks it), or one length per vertex
            ln = [NORMAL_LENGTHS[i % 5]] * 3 if i % 5 < 4 else [NORMAL_LENGTHS[j] for j in rng.randint(0, 4, size=3)]
            v = rng.normal(size=(3, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
            nrm.append(v * (np.array(ln) * rng.uniform(0.8, 1.2, size=3))[:, None])
            return i

        for cls in UV_CLASSES:
            for e in range(len(MAP)):
                for fl in (0, 1):
                    k = 2 * e + fl
                    if cls == "unit":
                        u = rng.uniform(-3.0, 3.0, size=(3, 2))
                    elif cls == "int":
                        u = rng.randint(-4, 5, size=(3, 2))
                    elif cls == "huge":
                        if fl:      # all three vertices next to +-2^20: ClampTexCoord's (float)(int) at its largest arguments
                            u = (UV_MAX - rng.randint(0, 64, size=(3, 2)) / 16.0) * rng.choice([-1.0, 1.0], size=(1, 2))
                        else:       # mixed signs, one coordinate exactly at the bound
                            u = rng.uniform(1e3, 1e6, size=(3, 2)) * rng.choice([-1.0, 1.0], size=(3, 2))
                            u[k % 3, k % 2] = UV_MAX * (1.0 if e % 2 else -1.0)
                    elif cls == "near":
                        u = np.zeros((3, 2))
                        for a in range(3):
                            for b in range(2):
                                base = int(rng.randint(-4, 5))
                                sgn = -1 if rng.rand() < 0.6 else 1
                                if a == 0 and b == e % 2:
                                    # vertex 0, which every covering block samples: a tiny negative coordinate, which ClampTexCoord wraps to
                                    # exactly 1.0 -- the one way to x1 = w - 1, with x2 wrapping to 0
                                    u[a, b] = -[1e-9, 1e-30, 1e-45][k % 3]
                                elif base == 0:
                                    u[a, b] = sgn * [1e-9, 1e-30, 1e-45, 1e-6][int(rng.randint(0, 4))]
                                elif rng.rand() < 0.5:
                                    u[a, b] = float(ulps(base, sgn * int(rng.randint(1, 5))))
                                else:
                                    u[a, b] = float(F(base) + F(sgn * rng.uniform(0.5e-6, 2e-6)))
                    elif cls == "span":
                        u = rng.uniform(-3.0, 3.0, size=(1, 2)) + rng.uniform(-1.0, 1.0, size=(3, 2)) * 10.0 ** (k % 6)
                    else:
                        # dyadic: every coordinate a multiple of 1/64 below 8.  "fine": any such vertices, the partner shifted by up to +-16;
                        # "coarse": edges of +-4 per axis, the partner shifted by up to +-8000.  With the barycentrics of dyadic_bary() every
                        # product and sum of the interpolation is then exact for the triangle AND its partner (24 bits suffice), so the two
                        # sample identically
                        if k % 2 == 0:
                            u = rng.randint(-511, 512, size=(3, 2)) / 64.0
                            shift = rng.randint(-16, 17, size=2)
                        else:
                            u0 = rng.randint(-255, 256, size=(1, 2)) / 64.0
                            edges = np.array([[(4.0, 0.0), (0.0, 4.0)], [(4.0, 4.0), (-4.0, 4.0)], [(-4.0, 0.0), (4.0, -4.0)]][k % 3]) * rng.choice([-1.0, 1.0])
                            u = np.concatenate([u0, u0 + edges], axis=0)
                            shift = rng.randint(-8000, 8001, size=2)
                        shift[shift == 0] = 3
                    i = add(e, fl, u, cls)
                    if cls == "dyadic":
                        j = add(e, fl, u + shift[None, :], "partner", partner_of=i)
                        nrm[j] = nrm[i].copy()
                        meta[i]["partner"] = j
        # ladders: one triangle per (texture, level) -- and two steep ones per texture with a side of 1, which must stay at level 0
        for k, (w, h) in enumerate(SHAPES):
            if min(w, h) >= 2:
                for lv in range(levels_of(w, h)):
                    s = ladder_scale(w, h, lv)
                    add(entry_of_tex[k], lv % 2, [(0.0, 0.0), (s, 0.0), (0.0, s)], "ladder", texture=k, level=lv)
            else:
                for n_, s in enumerate((1000.0, 100000.0)):
                    add(entry_of_tex[k], n_, [(0.0, 0.0), (s, 0.0), (0.0, s)], "ladder", texture=k, level=0)
        n = len(uv)
        self.n = n
        self.uv = np.array(uv, dtype=np.float64).astype(np.float32)
        self.nrm = np.array(nrm, dtype=np.float64).astype(np.float32)
        self.mat_index = np.array(entry, dtype=np.int32)
        self.flat = np.array(flat, dtype=bool)
        self.meta = meta
        assert np.isfinite(self.uv).all() and (np.abs(self.uv) < 2.0 ** 20).all() and np.isfinite(self.nrm).all()
        # geometry: small triangles on the 1/1024 grid
        c = rng.uniform(-2.0, 2.0, size=(n, 1, 3))
        self.tv = np.ascontiguousarray((np.round((c + rng.uniform(-0.2, 0.2, size=(n, 3, 3))) * 1024.0) / 1024.0).astype(np.float32))
        self.osc = O.OracleScene(self.tv)
        self.slot_of = np.zeros(n, dtype=np.int64)                         # input triangle -> triId
        self.slot_of[self.osc.perm] = np.arange(n)
        self.input_of = np.asarray(self.osc.perm, dtype=np.int64)          # triId -> input triangle
        self.slots_of_entry = [[int(self.slot_of[i]) for i in range(n) if entry[i] == e] for e in range(len(MAP))]
        kind_of_entry = ["default" if m < 0 else self.descs[m][0] for m in MAP]
        self.slots_of_kind = {kd: [s for e in range(len(MAP)) if kind_of_entry[e] == kd for s in self.slots_of_entry[e]] for kd in ("tex", "uber", "simple", "default")}
        self.pairs = [(int(self.slot_of[i]), int(self.slot_of[m["partner"]])) for i, m in enumerate(meta) if "partner" in m]

    # ---- barycentrics ---------------------------------------------------------------------------------------------------------------
    @staticmethod
    def inside(rng, shape):
        a, b = rng.rand(*shape), rng.rand(*shape)
        flip = a + b > 1.0
        return np.where(flip, 1.0 - a, a), np.where(flip, 1.0 - b, b)

    def bary(self, rng, flavour):
        """[4,4] bx, by of one block, inside the closed triangle: 0 anywhere, 1 a tight cluster (spread about 1e-4), 2 exactly on corners or edge
        midpoints, "span": every quad spans exactly 1/2 in both directions (the ladders), "dyadic": a cluster of exact dyadic offsets"""
        if flavour == "span":
            jx, jy = rng.uniform(0.0, 0.25, size=(4, 1)), rng.uniform(0.0, 0.25, size=(4, 1))
            bx = jx + np.array([[0.0, 0.5, 0.0, 0.25]]); by = jy + np.array([[0.0, 0.0, 0.5, 0.25]])
        elif flavour == "dyadic":
            cx, cy = [(0.25, 0.25), (0.125, 0.5), (0.5, 0.125), (0.125, 0.125)][int(rng.randint(0, 4))]
            bx = cx + rng.randint(0, 4, size=(4, 4)) / 8192.0; by = cy + rng.randint(0, 4, size=(4, 4)) / 8192.0
        elif flavour == 0:
            bx, by = self.inside(rng, (4, 4))
        elif flavour == 1:
            cx, cy = self.inside(rng, (1, 1))
            bx = cx * 0.99 + rng.uniform(0.0, 1e-4, size=(4, 4)); by = cy * 0.99 + rng.uniform(0.0, 1e-4, size=(4, 4))
        else:
            pts = np.array([(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (0.5, 0.0), (0.0, 0.5), (0.5, 0.5)])
            pick = pts[rng.randint(0, 6, size=(4, 4))]
            bx, by = pick[..., 0], pick[..., 1]
        return bx.astype(np.float32), by.astype(np.float32)

    def bary_for(self, rng, slot, flavour):
        """the barycentrics of a block on one triangle: the ladders' spanning quads; for the classes whose point lies AT the vertices (exact integers,
        integers +- a few ulps, +-2^20) corners and edge midpoints, vertex 0 first; otherwise the flavour asked for"""
        cls = self.meta[int(self.input_of[slot])]["cls"]
        bx, by = self.bary(rng, "span" if cls == "ladder" else 2 if cls in ("int", "near", "huge") else flavour)
        if cls in ("int", "near", "huge"):
            bx[0, 0:3], by[0, 0:3] = (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
        return bx, by

    # ---- the block recipes: each -> (t, id, bx, by), all [4 quads, 4 lanes] ---------------------------------------------------------------
    def block(self, rng, recipe, arg=None):
        n = self.n
        t = rng.uniform(0.5, 50.0, size=(4, 4)).astype(np.float32)
        flavour = int(rng.randint(0, 3))
        pick = lambda seq: seq[int(rng.randint(0, len(seq)))]      # noqa: E731
        if recipe == "one":                       # a full block on one triangle
            ids = np.full((4, 4), arg, dtype=np.int64)
            bx, by = self.bary_for(rng, arg, flavour)
            return t, ids, bx, by
        bx, by = self.bary(rng, flavour)
        hit = np.full((4, 4), True)
        if recipe == "one_material":              # a full block of one material on several triangles
            slots = self.slots_of_entry[arg]
            ids = rng.choice(slots, size=(4, 4))
            ids[0, 0], ids[0, 1] = slots[0], slots[1]
        elif recipe == "materials":               # a full block of several materials, the default among them
            es = [self.default_entry] + list(rng.choice([e for e in range(len(MAP)) if e != self.default_entry], size=int(rng.randint(1, 4)), replace=False))
            ids = np.array([[pick(self.slots_of_entry[pick(es)]) for _ in range(4)] for _ in range(4)], dtype=np.int64)
            ids[1, 2], ids[2, 1] = pick(self.slots_of_entry[es[0]]), pick(self.slots_of_entry[es[1]])
        elif recipe == "partial_one_material":    # a partial block of one material
            slots = self.slots_of_entry[arg]
            ids = rng.choice(slots, size=(4, 4)) if rng.rand() < 0.5 else np.full((4, 4), pick(slots), dtype=np.int64)
            hit = rng.rand(4, 4) < 0.7
            hit[int(rng.randint(0, 4)), int(rng.randint(0, 4))] = False
            if not hit.any():
                hit[2, 1] = True
        elif recipe == "lane0_missed":            # lane 0 missed while other lanes hit triangle 0 or another triangle
            ids = np.where(rng.rand(4, 4) < 0.5, 0, rng.randint(0, n, size=(4, 4)))
            hit = rng.rand(4, 4) < 0.8
            hit[:, 0] = rng.rand(4) < 0.25
            hit[0, 0] = False; hit[0, 1] = True; ids[0, 1] = 0
        elif recipe == "none":                    # no hit
            ids = np.zeros((4, 4), dtype=np.int64)
            hit[...] = False
        elif recipe == "odd_lane":                # one odd lane in an otherwise single-triangle block
            slot = int(rng.randint(0, n))
            ids = np.full((4, 4), slot, dtype=np.int64)
            e = int(self.mat_index[self.input_of[slot]])
            other = pick([s for s in self.slots_of_entry[e] if s != slot]) if arg % 2 == 0 else int(rng.randint(0, n))
            ids[int(rng.randint(0, 4)), int(rng.randint(0, 4))] = other
            bx, by = self.bary_for(rng, slot, flavour)
        elif recipe == "garbage_misses":          # missed lanes that carry ids far outside the scene (and any barycentrics)
            ids = rng.randint(0, n, size=(4, 4)) if arg % 2 else rng.choice(self.slots_of_entry[arg % len(MAP)], size=(4, 4))
            hit = rng.rand(4, 4) < 0.6
            hit[1, 0] = False; hit[3, 3] = True
            ids = np.where(hit, ids, rng.choice(GARBAGE_IDS, size=(4, 4)))
        elif recipe == "outside_hits":            # HIT lanes with ids of -5 and n + 7: clamped by the kernel to 0 and n - 1
            if arg % 4 == 3:
                ids = np.full((4, 4), -5 if arg % 8 == 3 else n + 7, dtype=np.int64)
            else:
                ids = np.full((4, 4), int(rng.randint(0, n)), dtype=np.int64)
                ids = np.where(rng.rand(4, 4) < 0.3, rng.choice([-5, n + 7], size=(4, 4)), ids)
                ids[0, 3], ids[2, 0] = -5, n + 7
        else:
            raise KeyError(recipe)
        t = np.where(hit, t, INF).astype(np.float32)
        return t, ids, bx, by

    MIXED = ["one_material", "materials", "partial_one_material", "lane0_missed", "none", "odd_lane", "garbage_misses", "outside_hits",
             "one_uber", "one_tex", "one_any", "one_material", "materials", "partial_one_material", "lane0_missed", "odd_lane"]

    @property
    def n_cover(self):
        """the packets whose blocks are single-triangle blocks over every triangle in turn"""
        return (self.n + 15) // 16

    def packet(self, p, generic=False):
        """packet p of the primary or of the generic list -> dict(t [64,4] float32, tri [64,4] int32, bary [64,8] float32, recipes [16]) and, for a
        generic packet, dirs [64,3,4] float32 and bits bool [64,4] (the selector: a lane that is not selected carries t = -inf).  Generic packets
        with an odd p behind the covering ones are partly masked (some of their missed lanes), the others have every lane selected."""
        rng = np.random.RandomState(5000 + 2 * p + (1 if generic else 0))
        t = np.zeros((64, 4), dtype=np.float32); tri = np.zeros((64, 4), dtype=np.int64); bary = np.zeros((64, 8), dtype=np.float32)
        recipes = []
        order = rng.permutation(16)
        for b in range(16):
            if p < self.n_cover:
                r, arg = "one", (16 * p + b) % self.n
            else:
                r = self.MIXED[order[b]]
                k = (p - self.n_cover) * 16 + b
                if r == "one_uber":
                    r, arg = "one", self.slots_of_kind["uber"][k % len(self.slots_of_kind["uber"])]
                elif r == "one_tex":
                    r, arg = "one", self.slots_of_kind["tex"][k % len(self.slots_of_kind["tex"])]
                elif r == "one_any":
                    r, arg = "one", int(rng.randint(0, self.n))
                elif r in ("one_material", "partial_one_material"):
                    arg = k % len(MAP)
                else:
                    arg = k
            bt, bi, bx, by = self.block(rng, r, arg)
            qs = slice(4 * b, 4 * b + 4)
            t[qs], tri[qs], bary[qs, 0:4], bary[qs, 4:8] = bt, bi, bx, by
            recipes.append(r)
        out = dict(t=t, tri=tri.astype(np.int32), bary=bary, recipes=recipes)
        if generic:
            d = rng.normal(size=(64, 3, 4))
            d /= np.sqrt((d * d).sum(axis=1, keepdims=True))
            bits = np.full((64, 4), True)
            if p % 2 == 1 and p >= self.n_cover:      # (every mixed packet has a block without a hit: lanes to leave unselected)
                bits = ~((t == INF) & (rng.rand(64, 4) < 0.5))
                bits[np.unravel_index(int(np.argmax(t == INF)), t.shape)] = False
                out["t"] = np.where(bits, t, -INF).astype(np.float32)
            out["dirs"], out["bits"] = np.ascontiguousarray(d.astype(np.float32)), bits
        assert not np.isnan(out["t"]).any() and ((out["t"] > 0) | (out["t"] == -INF)).all()
        return out

    def pair_packets(self, k):
        """two packets that differ only in their triIds: block b of the first lies on a dyadic triangle, block b of the second on its partner
        (shifted by exact integers), with the same barycentrics -> (dict, dict)"""
        rng = np.random.RandomState(7000 + k)
        t = rng.uniform(0.5, 50.0, size=(64, 4)).astype(np.float32)
        tri = [np.zeros((64, 4), dtype=np.int32), np.zeros((64, 4), dtype=np.int32)]
        bary = np.zeros((64, 8), dtype=np.float32)
        for b in range(16):
            qs = slice(4 * b, 4 * b + 4)
            pr = self.pairs[(16 * k + b) % len(self.pairs)]
            tri[0][qs], tri[1][qs] = pr
            bary[qs, 0:4], bary[qs, 4:8] = self.bary(rng, "dyadic")
        d = rng.normal(size=(64, 3, 4))
        d = np.ascontiguousarray((d / np.sqrt((d * d).sum(axis=1, keepdims=True))).astype(np.float32))
        return tuple(dict(t=t, tri=tri[j], bary=bary, dirs=d, bits=np.full((64, 4), True)) for j in range(2))

    def packet_xy(self, n=N_PACKETS):
        """the packets of the 70 x 50 frame (partial ones among them), repeated as often as the list needs"""
        xy = np.array([(x, y) for y in range(0, FRAME[1], 16) for x in range(0, FRAME[0], 16)], dtype=np.int32)
        return np.ascontiguousarray(xy[np.arange(n) % len(xy)])


@functools.lru_cache(maxsize=None)
def synth():
    return Synth()


@functools.lru_cache(maxsize=None)
def ref_textures(grey=False):
    s = synth()
    return [M.RefTexture(t) for t in (s.textures_grey if grey else s.textures)]


@functools.lru_cache(maxsize=None)
def reference(grey=False):
    """the restatement over the synthetic set"""
    s = synth()
    return M.MaterialsRef(s.osc, s.uv, s.nrm, s.mat_index, s.flat, s.material_map, K.ref_materials(s.descs_grey if grey else s.descs), ref_textures(grey))


def to_planes(nrm, diff, spec):
    return np.concatenate([nrm.transpose(1, 0, 2), diff.transpose(1, 0, 2), spec.transpose(1, 0, 2)], axis=0)


@functools.lru_cache(maxsize=None)
def expected_primary(mode):
    """the restatement's samples of the primary list (rays of oracle_lib.gen_packet in `mode`) -> (float32 [n,9,64,4], its diagnostics);
    computed once, shared, never changed.  Ids outside the scene are clamped by the header's rule first."""
    s, ref, diag = synth(), reference(), M.Diag()
    xy = s.packet_xy()
    out = np.zeros((N_PACKETS, 9, 64, 4), dtype=np.float32)
    for p in range(N_PACKETS):
        pk = s.packet(p)
        d = primary_dirs(int(xy[p, 0]), int(xy[p, 1]), mode)
        _, nrm, diff, spec = ref.samples(d, pk["t"], clamp_ids(pk["tri"], s.n), pk["bary"], diag)
        out[p] = to_planes(nrm, diff, spec)
    out.setflags(write=False)
    return out, diag


@functools.lru_cache(maxsize=None)
def primary_dirs(px, py, mode):
    d = O.gen_packet(CAM13, FRAME[0], FRAME[1], px, py, mode)[0].reshape(64, 3, 4).copy()
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def expected_generic():
    """the restatement's samples of the generic list (the packets' own directions and selectors; no arithmetic mode enters) ->
    (float32 [n,9,64,4], BounceDiag)"""
    s, br, diag = synth(), B.BounceRef(reference()), B.BounceDiag()
    out = np.zeros((N_PACKETS, 9, 64, 4), dtype=np.float32)
    for p in range(N_PACKETS):
        pk = s.packet(p, generic=True)
        _, nrm, diff, spec = br.samples_rays(pk["dirs"], pk["t"], clamp_ids(pk["tri"], s.n), pk["bary"], pk["bits"], diag)
        out[p] = to_planes(nrm, diff, spec)
    out.setflags(write=False)
    return out, diag


def check_conditions(d, bd=None):
    """the conditions that keep a comparison over the synthetic lists from passing vacuously, on the restatement's diagnostics (d: Diag of the
    list; bd: the BounceDiag of a generic list)"""
    assert d.blocks_a >= 64 and d.blocks_b >= 64 and d.blocks_c >= 64, (d.blocks_a, d.blocks_b, d.blocks_c)
    assert d.blocks_masked_one >= 16, d.blocks_masked_one
    assert d.quirk_lanes >= 16, d.quirk_lanes
    assert d.normals_flat >= 16 and d.normals_right >= 16 and d.normals_left_a >= 16, (d.normals_flat, d.normals_right, d.normals_left_a)
    assert d.uber_unmasked >= 16 and d.uber_masked >= 16 and d.default_meets_others >= 16, (d.uber_unmasked, d.uber_masked, d.default_meets_others)
    if bd is not None:
        assert bd.a_uber_masked >= 8 and bd.a_uber_unmasked >= 8 and bd.a_tex_masked >= 8, (bd.a_uber_masked, bd.a_uber_unmasked, bd.a_tex_masked)
    for k, (w, h) in enumerate(SHAPES):
        got = sorted(lv for (t, lv) in d.mips if t == k)
        want = list(range(levels_of(w, h))) if min(w, h) >= 2 else [0]      # a side of 1: Min(texDiff.x * 0, ..) = 0, level 0 whatever the step
        assert got == want, (k, (w, h), got, want)


def describe(d, bd=None):
    s = "blocks a/b/c/masked-one %d/%d/%d/%d quirk lanes %d normals flat/right/left %d/%d/%d uber unmasked/masked %d/%d default meets others %d" % (
        d.blocks_a, d.blocks_b, d.blocks_c, d.blocks_masked_one, d.quirk_lanes, d.normals_flat, d.normals_right, d.normals_left_a, d.uber_unmasked, d.uber_masked,
        d.default_meets_others)
    if bd is not None:
        s += " | (a) uber masked/unmasked %d/%d tex masked %d" % (bd.a_uber_masked, bd.a_uber_unmasked, bd.a_tex_masked)
    per_tex = {k: sorted(lv for (t, lv) in d.mips if t == k) for k in range(len(SHAPES))}
    return s + " | levels per texture " + str(per_tex)


# ---- one frame ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frame_case():
    """the `small` case of tests/materials_cases.py -- geometry, coordinates, normals, cameras, lights -- with the ten-texture noise set (its
    materials and map, by input index) in place of the case's own two textures -> (case, mat_index, restatement)"""
    c, s = K.case("small"), synth()
    mat_index = (np.arange(len(c["tv"])) % len(MAP)).astype(np.int32)
    return c, mat_index, M.MaterialsRef(c["osc"], c["uv"], c["nrm"], mat_index, c["flat"], s.material_map, K.ref_materials(s.descs), ref_textures())


# ---- the mirror stage's inputs ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mirror_inputs():
    """synthetic distances and sample buffers for the packets of the 70 x 50 frame -> (xy [n,2], t float32 [n,64,4], samples float32 [n,9,64,4]):
    t finite and positive, or +inf on a miss; normals of the lengths 0, 1e-20, ~1 and 1e3 and axis-aligned unit normals on the hit lanes (exact
    zeros among them), zeros on a lane that missed (the sample buffer's convention)"""
    s = synth()
    rng = np.random.RandomState(9001)
    xy = s.packet_xy(20)
    n = len(xy)
    t = rng.uniform(0.5, 50.0, size=(n, 64, 4)).astype(np.float32)
    p_hit = [1.0, 0.0, 0.5, 0.9, 0.1][:] * 4
    hit = rng.rand(n, 64, 4) < np.array(p_hit)[:n, None, None]
    t = np.where(hit, t, INF).astype(np.float32)
    v = rng.normal(size=(n, 64, 3, 4)); v /= np.sqrt((v * v).sum(axis=2, keepdims=True))
    kind = rng.randint(0, 5, size=(n, 64, 1, 4))
    length = np.array(NORMAL_LENGTHS + [1.0])[kind] * np.where(kind == 2, rng.uniform(0.8, 1.2, size=kind.shape), 1.0)
    axis = np.eye(3)[rng.randint(0, 3, size=(n, 64, 4))].transpose(0, 1, 3, 2) * rng.choice([-1.0, 1.0], size=(n, 64, 1, 4))
    nrm = np.where(kind == 4, axis, v * length)
    nrm = np.where(hit[:, :, None, :], nrm, 0.0).astype(np.float32)
    smp = rng.uniform(0.0, 1.0, size=(n, 9, 64, 4)).astype(np.float32)
    smp[:, 0:3] = nrm.transpose(0, 2, 1, 3)
    for a in (xy, t, smp):
        a.setflags(write=False)
    return xy, t, smp


@functools.lru_cache(maxsize=None)
def expected_mirror(mode):
    """BounceRef.mirror on mirror_inputs(), pos = d * t + cam in the restatement's operation order -> dict of stacked arrays, selected lanes"""
    xy, t, smp = mirror_inputs()
    org = CAM13[:3].reshape(1, 3, 1)
    outs = []
    for p in range(len(xy)):
        d = primary_dirs(int(xy[p, 0]), int(xy[p, 1]), mode)
        with np.errstate(all="ignore"):
            pos = (d * t[p].reshape(64, 1, 4) + org).astype(np.float32)
        outs.append(B.BounceRef.mirror(None, d, pos, np.ascontiguousarray(smp[p, 0:3].transpose(1, 0, 2)), t[p] < INF, mode))
    want = {k: np.ascontiguousarray(np.stack([o[k] for o in outs])) for k in ("origin", "dir", "idir", "mask", "distance", "object")}
    return want, int((t < INF).sum())
