"""Synthetic hit records for the sample stage of instanced full shading, k_imat_sample (tests/test_instances_materials_synth_host.py,
tests/test_gpu_instances_materials_synth.py).  The stage takes its hit records -- t, u, v, instance slot, triId -- from the caller
(include/snail_instances_materials.h), so a test can hand it any record of the documented domain without a scene whose traversal would
produce it.  Here: the ten texture shapes, 14 materials and the triangle soup of tests/materials_synth.py as BLAS "big" (with triangles of
dyadic normals added), the 12-triangle "box" and a one-triangle "tiny" BLAS, each behind a map of its own into ONE material list; 13
instances (the identity twice, three exact signed permutations, three general rotations) addressed by BUILDER slot; and a list of 48 packets
whose 16 blocks follow one recipe each: (slot, triId) equalities built on purpose, ids valid in one BLAS and out of range in another, slots
outside the scene, the (slot 0, triId 0) quirk and its two neighbours.  The restatement is tests/instances_materials_ref.py's behind the
clamp rule of clamp_records(), written from the reference's text and the header, not from the kernel.  Seeded numpy, float32; nothing here
touches a device or the product library.

Left out:
  - non-finite barycentrics and t = NaN (the header does not define them);
  - slots at or above the count on a handle that an update shrank (they read stale records: undefined);
  - normals or rotations that make subnormal products (the reference's flush mode is not established by the oracle);
  - non-rigid matrices;
  - k_imat_light on synthetic samples (it needs a scene to walk; the frame tests cover it);
  - texDiff products at or above 2^32, as in tests/materials_synth.py."""
from __future__ import annotations

import functools

import numpy as np

from tests import dbvh_ref as R
from tests import instances_materials_cases as K
from tests import instances_materials_ref as IM
from tests import materials_cases as MK
from tests import materials_synth as Y
from tests import oracle_lib as O

F = np.float32
INF = F(np.inf)
N_PACKETS = 48
MAP = Y.MAP                                     # BLAS 0 "big": class -> material
BOX_MAP = [12, 3, -1, 7, 12, 0, 10]             # BLAS 1 "box": another shuffle of another length.  Class 0 is UBER 12 here and TEX 5 in "big"; classes 0 and 4 are ONE material
TINY_MAP = [-1, 12]                             # BLAS 2 "tiny": its one triangle is of class 1, the UBER material that all three maps name
MAPS = [MAP, BOX_MAP, TINY_MAP]
UBER_SHARED, TEX_SHARED = 12, 3                 # materials that several maps name (TEX 3 is without N.R)
PERM3 = np.array([[0, -1, 0], [-1, 0, 0], [0, 0, -1]], dtype=np.float32)      # an exact rotation with a negative entry in every row
BIG, BOX, TINY = 0, 1, 2
# the entries of MAP that the dyadic-normal triangles take: TEX without N.R (materials 1, 3), TEX with (0), SIMPLE (10), UBER (12), default
DYADIC_ENTRIES = [MAP.index(m) for m in (1, 3, 0, 10, 12, -1)]


def rot_general(k):
    """three general rotations, nine non-zero entries each"""
    if k == 0:
        return K.general_rotation()
    a = [(0.9, -0.6, 0.3), (-0.2, 1.1, 2.0)][k - 1]
    r = (K.rot_axis((0, 0, 1), a[0]).astype(np.float64) @ K.rot_axis((0, 1, 0), a[1]).astype(np.float64) @ K.rot_axis((1, 0, 0), a[2]).astype(np.float64)).astype(np.float32)
    assert (r != 0).all()
    return r


# the instances in INPUT order: (BLAS, rotation, x of the translation).  The builder sorts them along x, so the slot order is not this one.
I3 = np.eye(3, dtype=np.float32)
INSTANCES = [
    (BIG, "identity", 30.0), (BIG, "identity", -12.0), (BIG, "rot90y", 6.0), (BIG, "rot180z", 48.0), (BIG, "perm3", -30.0), (BIG, "general0", -48.0),
    (BOX, "identity", 18.0), (BOX, "general1", -24.0), (BOX, "rot90y", 42.0),
    (TINY, "identity", -6.0), (TINY, "general2", 36.0), (TINY, "rot180z", 12.0),
    (BOX, "identity", -36.0),
]
ROTATIONS = {"identity": I3, "rot90y": K.ROT90Y, "rot180z": K.ROT180Z, "perm3": PERM3, "general0": rot_general(0), "general1": rot_general(1), "general2": rot_general(2)}
EXACT = ("rot90y", "rot180z", "perm3")


# ---- the shading data ----------------------------------------------------------------------------------------------------------------------
class Blas:
    def __init__(self, tv, uv, nrm, mat_index, flat, material_map, meta):
        self.tv = np.ascontiguousarray(np.asarray(tv, dtype=np.float32).reshape(-1, 9))
        self.n = len(self.tv)
        self.uv, self.nrm = np.asarray(uv, dtype=np.float32), np.asarray(nrm, dtype=np.float32)
        self.mat_index, self.flat = np.asarray(mat_index, dtype=np.int32), np.asarray(flat, dtype=bool)
        self.map, self.meta = list(material_map), meta
        self.osc = O.OracleScene(self.tv)
        self.input_of = np.asarray(self.osc.perm, dtype=np.int64)                 # triId -> input triangle
        self.tri_of = np.zeros(self.n, dtype=np.int64)                            # input triangle -> triId
        self.tri_of[self.input_of] = np.arange(self.n)
        self.material = np.asarray(self.map, dtype=np.int64)[self.mat_index[self.input_of]]      # triId -> material (-1: the default)
        self.tris_of_material = {int(m): np.flatnonzero(self.material == m).tolist() for m in np.unique(self.material)}
        self.per_blas = (self.uv, self.nrm, self.mat_index, self.flat, self.map)
        ln = np.sqrt((self.nrm.astype(np.float64) ** 2).sum(axis=2))
        self.good_normals = (ln > 0.5).all(axis=1)[self.input_of]                 # triId -> its three normals are of length ~1 or 1e3


def dyadic_normals(rng, variant):
    """three normals with components that are multiples of 1/64, 1/64 <= |.| <= 4, every component of ONE sign on all three vertices (no
    interpolated normal can be zero); variant 1: one component exactly zero on all three"""
    sign = rng.choice([-1.0, 1.0], size=(1, 3))
    v = rng.randint(1, 257, size=(3, 3)) / 64.0 * sign
    if variant:
        v[:, int(rng.randint(0, 3))] = 0.0
    return v


@functools.lru_cache(maxsize=None)
def blases():
    s = Y.synth()
    rng = np.random.RandomState(31007)
    # "big": the soup of tests/materials_synth.py as it is, then the dyadic-normal triangles (coordinates of class "unit")
    uv, nrm, entry, flat, meta, tv = [s.uv], [s.nrm], list(s.mat_index), list(s.flat), [dict(m) for m in s.meta], [s.tv]
    for variant in (0, 1):
        for j, e in enumerate(DYADIC_ENTRIES):
            uv.append(rng.uniform(-3.0, 3.0, size=(1, 3, 2))); nrm.append(dyadic_normals(rng, variant)[None])
            entry.append(e); flat.append(j % 3 == 0); meta.append(dict(cls="dyadic_normal", variant=variant))
            c = rng.uniform(-2.0, 2.0, size=(1, 1, 3))
            tv.append(np.round((c + rng.uniform(-0.2, 0.2, size=(1, 3, 3))) * 1024.0) / 1024.0)
    big = Blas(np.concatenate(tv), np.concatenate(uv), np.concatenate(nrm), entry, flat, MAP, meta)
    # "box": normals of length about 1, negative and positive components, every class of its map
    btv = K.box_tris()
    v = rng.normal(size=(12, 3, 3)); v /= np.linalg.norm(v, axis=2, keepdims=True)
    box = Blas(btv, rng.uniform(-3.0, 3.0, size=(12, 3, 2)), v * rng.uniform(0.8, 1.2, size=(12, 3, 1)), np.arange(12) % len(BOX_MAP), np.arange(12) % 2 == 1, BOX_MAP,
               [dict(cls="unit") for _ in range(12)])
    # "tiny": ONE triangle (HostBVH.build and OracleScene accept it): every triId clamps to 0
    v = rng.normal(size=(1, 3, 3)); v /= np.linalg.norm(v, axis=2, keepdims=True)
    tiny = Blas(np.array([[[0.0, 0.0, 0.0], [0.5, 0.0, 0.125], [0.0, 0.5, 0.25]]]), rng.uniform(-3.0, 3.0, size=(1, 3, 2)), v, [1], [False], TINY_MAP, [dict(cls="unit")])
    return [big, box, tiny]


def material_kind(m):
    return "default" if m < 0 else Y.material_descs()[m][0]


# ---- the instances ---------------------------------------------------------------------------------------------------------------------------
class Arrangement:
    """Instances in input order -> the restated tree and the records in BUILDER-SLOT order (perm from tests/dbvh_ref.build, as
    instances_materials_cases.cpu_ref takes it)."""

    def __init__(self, rot, tr, bi, names):
        self.rot, self.tr, self.bi_input = np.asarray(rot, dtype=np.float32), np.asarray(tr, dtype=np.float32), np.asarray(bi, dtype=np.int32)
        self.names = list(names)
        self.n = len(self.rot)
        oscs = [b.osc for b in blases()]
        self.xf_input = np.concatenate([self.rot.reshape(-1, 9), self.tr.reshape(-1, 3)], axis=1).astype(np.float32)
        bb = np.stack([np.concatenate([o.nodes[0]["bmin"], o.nodes[0]["bmax"]]) for o in oscs]).astype(np.float32)
        nodes, _depth, perm = R.build(self.xf_input, self.bi_input, bb)
        self.perm = np.asarray(perm, dtype=np.int64)                              # slot -> input instance
        assert not np.array_equal(self.perm, np.arange(self.n)), "the slot order must differ from the input order"
        self.slot_of = np.zeros(self.n, dtype=np.int64)                           # input instance -> slot
        self.slot_of[self.perm] = np.arange(self.n)
        self.ref = R.Ref(oscs, nodes, self.xf_input[self.perm], self.bi_input[self.perm])
        self.ref_input_order = R.Ref(oscs, nodes, self.xf_input, self.bi_input)   # the MISTAKE of reading slots as input order (to show the tests can fail)
        self.bi = self.ref.bi.astype(np.int64)                                    # slot -> BLAS
        self.n_tris = np.array([blases()[b].n for b in self.bi], dtype=np.int64)  # slot -> nTris of its BLAS
        self.name = [self.names[i] for i in self.perm]                            # slot -> rotation name
        self.slots_of_blas = [np.flatnonzero(self.bi == b).tolist() for b in range(3)]

    def slots(self, blas=None, names=None):
        return [s for s in range(self.n) if (blas is None or self.bi[s] == blas) and (names is None or self.name[s] in names)]


@functools.lru_cache(maxsize=None)
def arrangement(key="main"):
    """"main": INSTANCES.  Its slot 0 is the instance of smallest x: "big" under general0 (asserted), so the (slot 0, triId 0) quirk and its
    (slot 0, triId != 0) neighbour are tested on a rotated "big" slot.  "updated": every rotation replaced by a turn of it, the translations
    mirrored and those of instances 3 and 8 exchanged, the same BLAS indices: there slot 0 is a "box" instance (asserted), so the same records
    meet the quirk on another BLAS and the neighbour's triId clamps to the box's last; no rotation is exact any more."""
    bi = [b for b, _, _ in INSTANCES]
    rot = np.stack([ROTATIONS[r] for _, r, _ in INSTANCES])
    tr = np.array([[x, 0.25 * (k % 3), -0.5 * (k % 2)] for k, (_, _, x) in enumerate(INSTANCES)], dtype=np.float32)
    names = [r for _, r, _ in INSTANCES]
    if key == "updated":
        turn = K.rot_axis((0, 1, 0), 0.2).astype(np.float64)
        rot = np.stack([(turn @ r.astype(np.float64)).astype(np.float32) for r in rot])
        tr = (tr * F(-1.0)).astype(np.float32)
        tr[[3, 8]] = tr[[8, 3]]
        names = ["turned " + r for r in names]
    a = Arrangement(rot, tr, bi, names)
    assert (a.bi[0], a.name[0]) == ((BIG, "general0") if key == "main" else (BOX, "turned rot90y")), (a.bi[0], a.name[0])
    return a


def clamp_records(slot, tri, arr=None):
    """The header's rule for a record outside the scene -> (slot, key triId, record triId):
      the slot is clamped to [0, nInst - 1] (a freshly created handle: its record capacity is its instance count);
      the triId is clamped below to 0 -- the block and quad comparisons and the quirk are taken on (clamped slot, lower-clamped triId);
      the record read is that of min(triId, nTris(BLAS of the slot) - 1)."""
    arr = arr or arrangement()
    s = np.clip(np.asarray(slot, dtype=np.int64), 0, arr.n - 1)
    key = np.maximum(np.asarray(tri, dtype=np.int64), 0)
    return s, key, np.minimum(key, arr.n_tris[s] - 1)


class SynthRef(IM.InstMaterialsRef):
    """InstMaterialsRef with "key compared" apart from "record read": samples() compares the (slot, triId) it is given, selement() reads the
    record of min(triId, nTris - 1) of the slot's BLAS"""

    def selement(self, slot, tri):
        return super().selement(slot, min(int(tri), len(self.tab[int(self.ref.bi[slot])][0]) - 1))


@functools.lru_cache(maxsize=None)
def reference(key="main", transform=True, input_order=False):
    a = arrangement(key)
    return SynthRef(a.ref_input_order if input_order else a.ref, [b.per_blas for b in blases()], MK.ref_materials(Y.material_descs()), Y.ref_textures(), transform=transform)


# ---- the packet list ---------------------------------------------------------------------------------------------------------------------
# the mixed part: (recipe, how many blocks); what is left of the 768 blocks behind the covering part is filled by FILL in turn
MIXED = [("same_tri_two_slots", 29), ("same_tri_two_blas", 16), ("shared_material", 16), ("materials", 19), ("partial_one_material", 31), ("odd_lane", 9),
         ("none", 1), ("lane0_missed", 12), ("garbage_misses", 8), ("outside_hits", 16)]
FILL = ["partial_one_material", "materials", "partial_one_material"]
OUTSIDE = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 2, 3, 4, 6, 0, 5]      # the variants of outside_hits, by arg


class Lists:
    def __init__(self, key="main"):
        self.arr = a = arrangement(key)
        self.B = B = blases()
        self.s = Y.synth()
        rng = np.random.RandomState(4100)
        # the covering part: every triangle of every BLAS in a full block under an identity slot and under a rotated one (by INPUT instance, so
        # that the same list serves another arrangement).  "big": the rotated slot by the input triangle's index -- general0 for every even one
        # (all normal-length classes, index mod 5, meet it), the three exact rotations in turn for the odd ones; the ladders are among them.
        so = a.slot_of
        cover = []
        for t in range(B[BIG].n):
            i = int(B[BIG].input_of[t])
            cover.append((int(so[i % 2]), t))
            cover.append((int(so[[5, 2, 5, 3, 5, 4][i % 6]]), t))
        for t in range(B[BOX].n):
            cover += [(int(so[[6, 12][t % 2]]), t), (int(so[[7, 8][t % 2]]), t)]
        cover += [(int(so[9]), 0), (int(so[10]), 0), (int(so[11]), 0)]
        self.cover = [cover[k] for k in rng.permutation(len(cover))]
        mixed = [(r, k) for r, cnt in MIXED for k in range(cnt)]
        left = 16 * N_PACKETS - len(cover) - len(mixed)
        assert left >= 0, left
        mixed += [(FILL[k % len(FILL)], 1000 + k) for k in range(left)]
        self.mixed = [mixed[k] for k in rng.permutation(len(mixed))]
        self.ident = {b: [int(so[i]) for i, (bb, r, _) in enumerate(INSTANCES) if bb == b and r == "identity"] for b in range(3)}

    # ---- barycentrics of a block on one triangle: materials_synth's flavours by the triangle's class
    def bary_for(self, rng, blas, tri, flavour):
        cls = self.B[blas].meta[int(self.B[blas].input_of[tri])]["cls"]
        bx, by = self.s.bary(rng, "span" if cls == "ladder" else 2 if cls in ("int", "near", "huge") else flavour)
        if cls in ("int", "near", "huge"):
            bx[0, 0:3], by[0, 0:3] = (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
        return bx, by

    def draw(self, rng, m, among=(BIG, BOX, TINY)):
        """a (slot, triId) whose material is m, the BLAS, its slot and its triangle drawn in turn"""
        bs = [b for b in among if self.B[b].tris_of_material.get(m)]
        b = bs[int(rng.randint(0, len(bs)))]
        sl = self.arr.slots_of_blas[b]
        tl = self.B[b].tris_of_material[m]
        return sl[int(rng.randint(0, len(sl)))], tl[int(rng.randint(0, len(tl)))], b

    def draw_any(self, rng):
        s = int(rng.randint(0, self.arr.n))
        return s, int(rng.randint(0, self.arr.n_tris[s]))

    @staticmethod
    def spread(rng, values):
        """[4, 4] of the values, each at least once, the first one on the block's first lane"""
        out = np.array(values)[rng.randint(0, len(values), size=16)]
        out[rng.permutation(15)[:len(values) - 1] + 1] = values[1:]
        out[0] = values[0]
        return out.reshape(4, 4)

    # ---- the recipes: -> (t, slot, tri, bx, by, info), arrays [4 quads, 4 lanes]
    def block(self, rng, recipe, arg):
        a, B = self.arr, self.B
        t = rng.uniform(0.5, 50.0, size=(4, 4)).astype(np.float32)
        flavour = int(rng.randint(0, 3))
        pick = lambda seq: seq[int(rng.randint(0, len(seq)))]      # noqa: E731
        info = dict(recipe=recipe, arg=arg)
        hit = np.full((4, 4), True)
        slot = np.zeros((4, 4), dtype=np.int64); tri = np.zeros((4, 4), dtype=np.int64)
        if recipe == "one":                       # a full block on one pair
            s, tr = arg
            slot[...], tri[...] = s, tr
            bx, by = self.bary_for(rng, int(a.bi[s]), tr, flavour)
            return t, slot, tri, bx, by, info
        bx, by = self.s.bary(rng, flavour)
        if recipe == "same_tri_two_slots":        # a full block with ONE triId of one BLAS in 2 to 4 slots
            b = [BIG, BOX, BIG, TINY, BIG, BOX][arg % 6]
            identity_only = arg % 6 in (0, 1)     # ... of which a third in the two identity slots alone: the records are equal, only the branch differs
            kind = ["tex", "uber", "simple"][(arg // 6) % 3]
            if b == TINY:
                kind = "uber"
            if b == BOX and kind == "simple":
                kind = "tex"
            if b == BOX and identity_only:        # (the box has no ladder: equal records of a TEX material may sample alike in (a) and (b))
                kind = "uber"
            ok = [x for x in range(B[b].n) if material_kind(int(B[b].material[x])) == kind and B[b].good_normals[x]]
            if identity_only and kind == "tex":   # equal records: the ladders of level 1 and above, where (a)'s texDiff picks another level than (b)'s 0
                lad = [x for x in range(B[b].n) if B[b].meta[int(B[b].input_of[x])].get("level", 0) >= 1 and B[b].good_normals[x]]      # (N.R of a zero normal hides the texture)
                ok = lad if b == BIG else ok
            tr = pick(ok)
            if identity_only and B[b].meta[int(B[b].input_of[tr])]["cls"] != "ladder" and kind != "tex":
                ok = [x for x in ok if not B[b].flat[B[b].input_of[x]]]      # equal records: lerp_right against lerp_left must be there to see
                tr = pick(ok)
            cand = self.ident[b] if identity_only else a.slots_of_blas[b]
            chosen = [int(x) for x in rng.permutation(cand)[:min(len(cand), 2 + arg % 3)]]
            slot, tri[...] = self.spread(rng, chosen), tr
            bx, by = self.bary_for(rng, b, tr, 0)
            info.update(identity_only=identity_only, kind=kind, blas=b, flat=bool(B[b].flat[B[b].input_of[tr]]))
        elif recipe == "same_tri_two_blas":       # a full block with ONE triId in slots of different BLASes
            bs = [(BIG, BOX), (BIG, BOX, TINY), (BOX, TINY), (BIG, TINY)][arg % 4]
            tr = 0 if TINY in bs else int(rng.randint(0, B[BOX].n))
            slot, tri[...] = self.spread(rng, [pick(a.slots_of_blas[b]) for b in rng.permutation(bs)]), tr
        elif recipe == "shared_material":         # a full block over two or three BLASes whose lanes all map to ONE material
            m = [UBER_SHARED, TEX_SHARED, -1][arg % 3]
            bs = [b for b in (BIG, BOX, TINY) if B[b].tris_of_material.get(m)]
            for q in range(4):
                for l in range(4):
                    slot[q, l], tri[q, l], _ = self.draw(rng, m, among=[bs[(4 * q + l) % len(bs)]] if 4 * q + l < len(bs) else bs)
            info.update(material=m)
        elif recipe == "materials":               # a full block of several materials, the default among them
            ms = [-1] + [int(x) for x in rng.choice(14, size=int(rng.randint(1, 4)), replace=False)]
            for q in range(4):
                for l in range(4):
                    slot[q, l], tri[q, l], _ = self.draw(rng, pick(ms))
            slot[1, 2], tri[1, 2], _ = self.draw(rng, ms[0]); slot[2, 1], tri[2, 1], _ = self.draw(rng, ms[1])
        elif recipe == "partial_one_material":    # a partial block of one material, on several pairs or on one
            m = arg % 15 - 1
            one = self.draw(rng, m) if rng.rand() < 0.3 else None
            for q in range(4):
                for l in range(4):
                    slot[q, l], tri[q, l], _ = one or self.draw(rng, m)
            hit = rng.rand(4, 4) < 0.7
            hit[int(rng.randint(0, 4)), int(rng.randint(0, 4))] = False
            if not hit.any():
                hit[2, 1] = True
        elif recipe == "odd_lane":                # one odd lane in an otherwise single-pair block: in the slot only, the triId only, or both
            s, tr = self.draw_any(rng)
            b = int(a.bi[s])
            slot[...], tri[...] = s, tr
            q, l = int(rng.randint(0, 4)), int(rng.randint(0, 4))
            if arg % 3 != 1:
                others = [x for x in (a.slots_of_blas[b] if arg % 3 == 0 else range(a.n)) if x != s]
                slot[q, l] = pick(others)
            if arg % 3 != 0:
                n_other = int(a.n_tris[slot[q, l]])
                tri[q, l] = (tr + 1 + int(rng.randint(0, max(n_other - 1, 1)))) % n_other if n_other > 1 else 0
            bx, by = self.bary_for(rng, b, tr, flavour)
        elif recipe == "none":                    # no hit
            hit[...] = False
        elif recipe == "lane0_missed":            # lane 0 of every quad missed (carrying garbage); beside it ONE pair per block:
            # (slot 0, tri 0): the quirk | (slot k != 0, tri 0) and (slot 0, tri != 0): their own records | (-3, -5): clamps to (0, 0), the quirk too
            v = arg % 4
            s, tr = [(0, 0), (int(rng.randint(1, a.n)), 0), (0, int(rng.randint(1, a.n_tris[0]))), (-3, -5)][v]
            slot[...], tri[...] = s, tr
            hit = rng.rand(4, 4) < 0.85
            hit[:, 0] = False; hit[:, 1] = True
            if arg % 2:
                slot[:, 0], tri[:, 0] = rng.choice(Y.GARBAGE_IDS, size=4), rng.choice(Y.GARBAGE_IDS, size=4)
            info.update(variant=v)
        elif recipe == "garbage_misses":          # missed lanes that carry slots and ids far outside the scene (and any barycentrics)
            m = arg % 15 - 1
            for q in range(4):
                for l in range(4):
                    slot[q, l], tri[q, l] = self.draw(rng, m)[:2] if arg % 2 == 0 else self.draw_any(rng)
            hit = rng.rand(4, 4) < 0.6
            hit[1, 0] = False; hit[3, 3] = True
            slot = np.where(hit, slot, rng.choice(Y.GARBAGE_IDS, size=(4, 4))); tri = np.where(hit, tri, rng.choice(Y.GARBAGE_IDS, size=(4, 4)))
        elif recipe == "outside_hits":            # HIT lanes with slots and ids outside the scene
            v = OUTSIDE[arg % len(OUTSIDE)]
            s, tr = self.draw_any(rng)
            slot[...], tri[...] = s, tr
            some = rng.rand(4, 4) < 0.3
            if v == 0:                            # slots -3 and nInst + 5 among the lanes of a pair
                slot = np.where(some, rng.choice([-3, a.n + 5], size=(4, 4)), slot)
                slot[0, 3], slot[2, 0] = -3, a.n + 5
            elif v == 1:                          # triId -5 among them
                tri = np.where(some, -5, tri)
                tri[0, 3] = -5
            elif v in (2, 3, 4):                  # 16 lanes of nTris + 7 in one slot, for each BLAS: ONE pair, branch (a)
                slot[...] = pick(a.slots_of_blas[v - 2])
                tri[...] = B[v - 2].n + 7
            elif v == 5:                          # an id that is valid in "big" and out of range in "box" and "tiny", in slots of all three
                slot = self.spread(rng, [pick(a.slots_of_blas[b]) for b in (BIG, BOX, TINY)])
                tri[...] = 200 + arg
            elif v == 6:                          # n + 7 and n + 9 in one slot: ONE record, two keys -- not a single triangle
                b = (arg // 2) % 3
                slot[...] = pick(a.slots_of_blas[b])
                tri = self.spread(rng, [B[b].n + 7, B[b].n + 9])
                info.update(mixed_n7_n9=True)
            elif v == 7:                          # -5 and n + 7 among the lanes of a pair
                n = int(a.n_tris[s])
                tri = np.where(some, rng.choice([-5, n + 7], size=(4, 4)), tri)
                tri[0, 3], tri[2, 0] = -5, n + 7
            else:                                 # 16 lanes of slot nInst + 5 (v = 8) or -3 (v = 9): the last / the first slot's records, two triangles
                slot[...] = a.n + 5 if v == 8 else -3
                n = int(a.n_tris[a.n - 1 if v == 8 else 0])
                tri = self.spread(rng, [int(x) for x in rng.permutation(n)[:2]])
            info.update(variant=v)
        else:
            raise KeyError(recipe)
        t = np.where(hit, t, INF).astype(np.float32)
        return t, slot, tri, bx, by, info

    def packet(self, p):
        """packet p -> dict(t [64,4] float32, slot / tri [64,4] int32, bary [64,8] float32, info [16])"""
        rng = np.random.RandomState(8000 + p)
        t = np.zeros((64, 4), dtype=np.float32); slot = np.zeros((64, 4), dtype=np.int64); tri = np.zeros((64, 4), dtype=np.int64)
        bary = np.zeros((64, 8), dtype=np.float32)
        infos = []
        for b in range(16):
            g = 16 * p + b
            r, arg = ("one", self.cover[g]) if g < len(self.cover) else self.mixed[g - len(self.cover)]
            bt, bs, bi, bx, by, info = self.block(rng, r, arg)
            qs = slice(4 * b, 4 * b + 4)
            t[qs], slot[qs], tri[qs], bary[qs, 0:4], bary[qs, 4:8] = bt, bs, bi, bx, by
            infos.append(info)
        assert not np.isnan(t).any() and (t > 0).all() and np.isfinite(bary).all()
        return dict(t=t, slot=slot.astype(np.int32), tri=tri.astype(np.int32), bary=bary, info=infos)


@functools.lru_cache(maxsize=None)
def lists(key="main"):
    return Lists(key)


def stack(pk):
    """packets -> the arrays of a record list: t, slot, tri [n,64,4], bary [n,64,8], info [n][16] (read-only)"""
    out = dict(t=np.stack([p["t"] for p in pk]), slot=np.stack([p["slot"] for p in pk]), tri=np.stack([p["tri"] for p in pk]), bary=np.stack([p["bary"] for p in pk]))
    for v in out.values():
        v.setflags(write=False)
    out["info"] = [p.get("info", [{}] * 16) for p in pk]
    return out


@functools.lru_cache(maxsize=None)
def records(key="main"):
    """the 48-packet list of an arrangement"""
    ls = lists(key)
    return stack([ls.packet(p) for p in range(N_PACKETS)])


def packet_xy(n=N_PACKETS):
    return Y.synth().packet_xy(n)


def expected_of(recs, mode, key="main", ref=None, diag=None):
    """the restatement's samples of a record list under an arrangement (rays of oracle_lib.gen_packet in `mode`, packet p at packet_xy()[p]) ->
    (float32 [n,9,64,4], Diag).  The records go through clamp_records first."""
    arr = arrangement(key)
    ref = ref or reference(key)
    diag = diag or IM.Diag()
    n = len(recs["t"])
    xy = packet_xy(n)
    out = np.zeros((n, 9, 64, 4), dtype=np.float32)
    for p in range(n):
        d = Y.primary_dirs(int(xy[p, 0]), int(xy[p, 1]), mode)
        s, key_tri, _ = clamp_records(recs["slot"][p], recs["tri"][p], arr)
        _, nrm, diff, spec = ref.samples(d, recs["t"][p], s, key_tri, recs["bary"][p], diag)
        out[p] = Y.to_planes(nrm, diff, spec)
    out.setflags(write=False)
    return out, diag


@functools.lru_cache(maxsize=None)
def expected(mode, key="main"):
    """the 48-packet list through the restatement: computed once, shared, never changed -> (float32 [48,9,64,4], diagnostics)"""
    smp, d = expected_of(records(key), mode, key)
    count_records(records(key), arrangement(key), d)
    return smp, d


def collapse_slots_by_tri(recs):
    """The MISTAKE of comparing triIds alone: a lane whose triId equals that of the lane it is compared with gets that lane's slot (the block's
    first lane when all 16 triIds are equal, else its quad's lane 0; a missed lane counts as (0, 0)) -> records with the slots rewritten"""
    hit = recs["t"] < INF
    slot = np.where(hit, recs["slot"], 0).astype(np.int32); tri = np.where(hit, np.maximum(recs["tri"], 0), 0)
    n = len(slot)
    for p in range(n):
        for b in range(16):
            qs = slice(4 * b, 4 * b + 4)
            if hit[p, qs].all() and (tri[p, qs] == tri[p, 4 * b, 0]).all():
                slot[p, qs] = slot[p, 4 * b, 0]
                continue
            for q in range(4 * b, 4 * b + 4):
                same = hit[p, q] & (tri[p, q] == tri[p, q, 0])
                slot[p, q] = np.where(same, slot[p, q, 0], slot[p, q])
    return dict(recs, slot=slot)


def collapse_identity_blocks(recs):
    """every same_tri_two_slots block whose slots are identity instances: each slot replaced by the block's first -> (records, bool [n, 16])"""
    slot = np.array(recs["slot"])
    which = np.zeros((len(slot), 16), dtype=bool)
    for p, infos in enumerate(recs["info"]):
        for b, info in enumerate(infos):
            if info.get("recipe") == "same_tri_two_slots" and info["identity_only"]:
                slot[p, 4 * b:4 * b + 4] = slot[p, 4 * b, 0]
                which[p, b] = True
    return dict(recs, slot=slot), which


# ---- lists on the dyadic-normal triangles -----------------------------------------------------------------------------------------------------
def dyadic_tris(variants=(0, 1)):
    b = blases()[BIG]
    return [t for t in range(b.n) if b.meta[int(b.input_of[t])].get("variant") in variants and b.meta[int(b.input_of[t])]["cls"] == "dyadic_normal"]


def dyadic_records(slot, variants=(0, 1), n_packets=2, mixed=False):
    """packets in ONE slot of "big" on the dyadic-normal triangles alone: full single-triangle blocks over the triangles in turn; with `mixed`
    every second block draws a triangle per lane, of one material or of any with some lanes missed (branches (b) and (c), the quirk aside: no triId 0 among them)"""
    tris = dyadic_tris(variants)
    assert 0 not in tris
    s, big = Y.synth(), blases()[BIG]
    pk = []
    for p in range(n_packets):
        rng = np.random.RandomState(9100 + p)
        t = rng.uniform(0.5, 50.0, size=(64, 4)).astype(np.float32)
        tri = np.zeros((64, 4), dtype=np.int32); bary = np.zeros((64, 8), dtype=np.float32)
        for b in range(16):
            qs = slice(4 * b, 4 * b + 4)
            bary[qs, 0:4], bary[qs, 4:8] = s.bary(rng, int(rng.randint(0, 3)))
            tri[qs] = tris[(16 * p + b) % len(tris)]
            if mixed and b % 4 == 1:              # several triangles of one material: (b), unmasked
                m = big.material[tris[(p + b // 4) % len(tris)]]
                tri[qs] = rng.choice([x for x in tris if big.material[x] == m], size=(4, 4))
                tri[4 * b, 0:2] = [x for x in tris if big.material[x] == m][:2]
            elif mixed and b % 4 == 3:            # any of them, some lanes missed: (c)
                tri[qs] = rng.choice(tris, size=(4, 4))
                t[qs] = np.where(rng.rand(4, 4) < 0.3, INF, t[qs])
        pk.append(dict(t=t, slot=np.full((64, 4), slot, dtype=np.int32), tri=tri, bary=bary))
    return stack(pk)


# ---- diagnostics counted from the records themselves ---------------------------------------------------------------------------------------
def count_records(recs, arr, d):
    """adds to the restatement's Diag what only the records show"""
    B = blases()
    hit = recs["t"] < INF
    slot, tri = recs["slot"].astype(np.int64), recs["tri"].astype(np.int64)
    cs, key, _ = clamp_records(slot, tri, arr)
    d.clamped_slot_lanes = int((hit & (cs != slot)).sum())
    out_tri = hit & ((tri < 0) | (tri >= arr.n_tris[cs]))
    d.clamped_tri_lanes = [int((out_tri & (arr.bi[cs] == b)).sum()) for b in range(3)]
    d.lanes_of_slot = [int((hit & (cs == s)).sum()) for s in range(arr.n)]
    missed0 = ~hit[:, :, 0:1] & hit
    d.neighbour_other_slot = int((missed0 & (cs != 0) & (key == 0)).sum())       # (k != 0, 0) beside a missed lane 0
    d.neighbour_other_tri = int((missed0 & (cs == 0) & (key != 0)).sum())        # (0, != 0) beside a missed lane 0
    d.quirk_from_records = int((missed0 & (cs == 0) & (key == 0)).sum())
    d.mixed_n7_n9_blocks = 0
    d.general_by_length = [0, 0, 0, 0]       # single-pair blocks under a general rotation on "big" triangles of normal length 0, 1e-20, ~1, 1e3
    general = np.array([(arr.ref.xf[s][:9] != 0).all() for s in range(arr.n)])
    for p in range(len(slot)):
        for b in range(16):
            qs = slice(4 * b, 4 * b + 4)
            if not hit[p, qs].all() or len(np.unique(cs[p, qs])) != 1:
                continue
            s0 = int(cs[p, 4 * b, 0]); n = int(arr.n_tris[s0])
            if set(tri[p, qs].reshape(-1).tolist()) == {n + 7, n + 9}:
                d.mixed_n7_n9_blocks += 1
            if len(np.unique(key[p, qs])) == 1 and arr.bi[s0] == BIG and general[s0] and key[p, 4 * b, 0] < n:
                i = int(B[BIG].input_of[key[p, 4 * b, 0]])
                if i < Y.synth().n and i % 5 < 4:
                    d.general_by_length[i % 5] += 1
    return d


def check_conditions(d):
    """the conditions that keep a comparison over the list from passing vacuously, on the restatement's diagnostics: minima that the
    restatement alone meets"""
    assert min(d.blocks_a, d.blocks_b, d.blocks_c, d.blocks_masked_one) >= 48, (d.blocks_a, d.blocks_b, d.blocks_c, d.blocks_masked_one)
    assert d.cross_instance_same_tri >= 32 and d.cross_blas_same_tri >= 16, (d.cross_instance_same_tri, d.cross_blas_same_tri)
    assert d.shared_material_unmasked >= 16 and d.shared_material_unmasked_uber >= 4, (d.shared_material_unmasked, d.shared_material_unmasked_uber)
    assert d.quirk_lanes >= 16 and d.quirk_lanes == d.quirk_from_records, (d.quirk_lanes, d.quirk_from_records)
    assert d.neighbour_other_slot >= 16 and d.neighbour_other_tri >= 16, (d.neighbour_other_slot, d.neighbour_other_tri)
    assert d.clamped_slot_lanes >= 32 and min(d.clamped_tri_lanes) >= 32, (d.clamped_slot_lanes, d.clamped_tri_lanes)
    assert d.mixed_n7_n9_blocks >= 1
    assert d.rotated_lanes >= 2000, d.rotated_lanes
    assert min(d.lanes_of_slot) >= 64, d.lanes_of_slot
    assert min(d.general_by_length) >= 16, d.general_by_length
    for k, (w, h) in enumerate(Y.SHAPES):
        got = sorted(lv for (t, lv) in d.mips if t == k)
        want = list(range(Y.levels_of(w, h))) if min(w, h) >= 2 else [0]
        assert got == want, (k, (w, h), got, want)


def describe(d):
    return ("blocks a/b/c/masked-one %d/%d/%d/%d | same tri across instances %d, across BLASes %d | shared material unmasked %d (uber %d) | quirk lanes %d, "
            "neighbours (k,0) %d (0,k) %d | clamped lanes: slot %d, triId per BLAS %s | n+7/n+9 blocks %d | rotated lanes %d | lanes per slot min %d | "
            "general rotation by normal length %s | levels per texture %s" % (
                d.blocks_a, d.blocks_b, d.blocks_c, d.blocks_masked_one, d.cross_instance_same_tri, d.cross_blas_same_tri, d.shared_material_unmasked,
                d.shared_material_unmasked_uber, d.quirk_lanes, d.neighbour_other_slot, d.neighbour_other_tri, d.clamped_slot_lanes, d.clamped_tri_lanes,
                d.mixed_n7_n9_blocks, d.rotated_lanes, min(d.lanes_of_slot), d.general_by_length,
                {k: sorted(lv for (t, lv) in d.mips if t == k) for k in range(len(Y.SHAPES))}))
