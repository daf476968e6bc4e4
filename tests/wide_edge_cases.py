"""The edges of include/snail_wide.h that tests/wide_cases.py leaves alone: intermediates in the denormal range, trees as deep as the
per-lane stack, index lists with duplicates and numbers that name no ray, every node as start node, and -- for the photon pass -- block
patterns that take the scan's carry round and distances that are NaN, -inf or negative.  Shared by tests/test_wide_edges_host.py (which
shows that each case reaches the edge it is named for) and tests/test_gpu_wide_edges.py / test_gpu_photons_edges.py.

A case is what tests/wide_cases.py calls one: dict(name, scene, origin, dir, idir, dist, indices, start).  Everything is seeded."""
import functools

import numpy as np

from snail_amd import HostBVH, scenes
from tests import wide_cases as WC
from tests import wide_ref as WR

F = np.float32

SCALES = (-38, -35, -33, 20, 60)       # the box times 2^k; -33 .. -38: squared normal components are denormal, and the hits stay
DEAD_SCALES = (-40, 60)                # the squares underflow to zero / overflow: t0 is 0 / inf and no triangle is ever hit
CHAIN_SCENES = ("chain64", "chain63", "chain50", "chain64_left")      # tests/test_bvh_fast_host.py: CHAINS; left_leaning() below


# ---- comparing floats ----
def float_mismatches(got, want):
    """-> the flat positions where `got` is not what `want` asks for.  Where the restatement has a NaN the device must have a NaN (the
    header fixes no payload; sign and payload of an invalid operation differ between x86 and gfx950); everything else by bit pattern,
    +-0 told apart."""
    g = np.ascontiguousarray(got, dtype=F).reshape(-1)
    w = np.ascontiguousarray(want, dtype=F).reshape(-1)
    assert g.shape == w.shape, (g.shape, w.shape)
    ok = np.where(np.isnan(w), np.isnan(g), g.view(np.uint32) == w.view(np.uint32))
    return np.flatnonzero(~ok)


def same_floats(got, want):
    return len(float_mismatches(got, want)) == 0


# ---- scenes ----
def scale_name(k):
    return "scaled_%+d" % k if k > 0 else "scaled_%d" % k


@functools.lru_cache(maxsize=None)
def verts(name):
    if name.startswith("scaled_"):
        return np.ascontiguousarray(scenes.box_scene() * F(2.0 ** int(name[7:])))      # a power of two: exact
    if name.startswith("chain"):
        from tests.test_bvh_fast_host import CHAINS
        return CHAINS[int(name[5:7])]()
    return WC.verts(name)


@functools.lru_cache(maxsize=None)
def bvh(name):
    """"scaled_<k>": the sweep builder's tree; "chain<depth>": the fast builder's, on the host; anything else: tests/wide_cases.py's"""
    if name.startswith("scaled_"):
        return HostBVH.build(verts(name))
    if name == "chain64_left":
        return left_leaning(bvh("chain64"))
    if name.startswith("chain"):
        from tests.test_bvh_fast_host import host_build
        return host_build(verts(name))
    return WC.bvh(name)


def is_leaf(nodes):
    return (nodes["sub"] & 0x80000000) != 0


def inner_nodes_on_the_longest_path(nodes, start=0):
    """the largest number of INNER nodes on a path from `start` to a leaf (the depth as the builders count it; what a ray has stacked on
    that path is most_stacked's number, which reaches this one only where every turn is a left turn)"""
    best, todo = 0, [(int(start), 0)]
    leaf = is_leaf(nodes)
    while todo:
        k, above = todo.pop()
        if leaf[k]:
            best = max(best, above)
        else:
            c = int(nodes["sub"][k])
            todo += [(c, above + 1), (c + 1, above + 1)]
    return best


def most_stacked(nodes, start=0):
    """-> (the most entries a ray can have stacked, the leaf where it has them).  An entry is a right sibling that waits for the left
    subtree; it is popped BEFORE the right subtree is entered, so what counts on a path are its turns to the LEFT, not its length."""
    best, where, todo = -1, -1, [(int(start), 0)]
    leaf = is_leaf(nodes)
    while todo:
        k, stacked = todo.pop()
        if leaf[k]:
            if stacked > best:
                best, where = stacked, k
        else:
            c = int(nodes["sub"][k])
            todo += [(c, stacked + 1), (c + 1, stacked)]
    return best, where


def left_leaning(b):
    """The same tree with the two records of every child pair swapped where the right subtree is the deeper one: every box, leaf and
    triangle as before (the walk reads neither axis nor firstNode), but the longest path now turns left at every node, so a ray that
    walks it has as many entries stacked as the path has inner nodes -- with the fast builder's 64-level chain, all 64 slots."""
    nodes = b.nodes.copy()

    def height(k):
        return 0 if is_leaf(nodes[k:k + 1])[0] else 1 + max(height(int(nodes["sub"][k])), height(int(nodes["sub"][k]) + 1))
    todo = [0]
    while todo:
        k = todo.pop()
        if is_leaf(nodes[k:k + 1])[0]:
            continue
        c = int(nodes["sub"][k])
        if height(c + 1) > height(c):
            nodes[[c, c + 1]] = nodes[[c + 1, c]]
        todo += [c, c + 1]
    return HostBVH(b.tris, nodes, b.depth, b.perm)


def denormal_squares(tris):
    """how many n[c] * n[c] of Collide0's recomputed normal are denormal (non-zero, below 2^-126), over the records"""
    with np.errstate(all="ignore"):
        a = tris["a"]
        nrm = WR._cross((tris["ba"] + a) - a, (tris["ca"] + a) - a)
        sq = nrm * nrm
    return int(((sq != 0) & (np.abs(sq) < WR.TINY)).sum())


# ---- wide-walk cases ----
def scaled(k):
    """256 box rays, scene and origins times 2^k; every other pair carries an initial distance of 0.5 * 2^k or 3 * 2^k"""
    s = F(2.0 ** k)
    o, d = WC.box_rays(256, 300 + k)
    dist = np.full(256, np.inf, dtype=F)
    i = np.arange(256)
    dist[(i % 8 == 2) | (i % 8 == 3)] = F(0.5) * s
    dist[(i % 8 == 6) | (i % 8 == 7)] = F(3.0) * s
    return WC._case(scale_name(k), scale_name(k), o * s, d, dist=dist)


def tiny_rays():
    """On the box times 2^-35: origins whose components are themselves denormal (the box rays of a box of 2^-130), and initial distances
    that are denormal, -0.0 and -inf among +inf and an ordinary one."""
    o, d = WC.box_rays(96, 77)
    o = o * F(2.0 ** -65) * F(2.0 ** -65)
    assert ((o != 0) & (np.abs(o) < WR.TINY)).all()
    dist = np.resize(np.asarray([np.inf, 2.0 ** -140, -0.0, -np.inf, 2.0 ** -36, 2.0 ** -149], dtype=F), 96)
    return WC._case("tiny_rays", "scaled_-35", o, d, dist=dist)


def chain_rays(scene):
    """About 200 rays at a deep_chain (triangles {(x, 0, 0), (x + s, 0, 0), (x, s, s)}, s = 1e-3 |x|, at x = +-2^k: all in the plane
    y = z, which holds the x axis):
      - along the x axis from |x| = 2^70 inwards, lateral offsets 1e-3 * 2^j: (e, e) lies in every triangle's plane (0 / 0), (e, e / 2)
        runs beside it (+-x / 0);
      - from the origin and from just off it outwards;
      - at every eighth triangle (every fourth binade of each sign of x) and at the first one of the leaf that takes the most stack
        (most_stacked), along the normal (Collide0 passes no ray that runs against it) from a quarter of its size off its plane: from
        in front (a finite hit at that binade) and from behind (the leaf is visited from inside its box: a negative distance).  The
        squared normal is s^4-sized: t0 is a number only for 2^-37 < s < 2^32, x = 2^-27 .. 2^41 -- half the chain; below and above
        it t0 is 0 or inf and nothing is hit;
      - seeded random ones from a shell."""
    depth = int(scene[5:7])
    tv = verts(scene).reshape(-1, 3, 3).astype(np.float64)
    b = bvh(scene)
    rng = np.random.RandomState(640 + depth)
    origin, d = [], []

    def ray(o, direction):
        origin.append(o)
        d.append(direction)

    for n, j in enumerate(range(-76, 60, 4)):
        e = 1e-3 * 2.0 ** j
        for sg in (1.0, -1.0):
            ray([sg * 2.0 ** 70, e, e if (n + (sg > 0)) % 2 else 0.5 * e], [-sg, 0.0, 0.0])
    for v in ([1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, 0, -1], [1, 1e-3, 1e-3], [-1, 5e-4, 2.5e-4]):
        ray([0.0, 0.0, 0.0], v)
    out = WC._unit(rng.randn(24, 3)).astype(np.float64)
    for n in range(24):
        ray([0.0, 0.0, 0.0] if n % 2 else (out[n] * 2.0 ** (-70 + 5 * n)).tolist(), out[n])
    nrm = np.asarray([0.0, -1.0, 1.0]) / np.sqrt(2.0)
    rec = b.tris[int(b.nodes["sub"][most_stacked(b.nodes)[1]]) & 0x7fffffff]
    a = rec["a"].astype(np.float64)
    deepest = np.stack([a, a + rec["ba"], a + rec["ca"]])
    for n, t in enumerate([deepest, deepest] + list(tv[0::8]) + list(tv[1::8])):      # x > 0, then x < 0
        s = t[1, 0] - t[0, 0]
        p = t[0] + ((t[1] - t[0]) + (t[2] - t[0])) * (0.2 + 0.1 * (n % 3))
        ray(p + (1.0 if n % 2 else -1.0) * nrm * 0.25 * abs(s), nrm)
    shell = WC._unit(rng.randn(30, 3)).astype(np.float64) * 2.0 ** rng.uniform(-60.0, 66.0, size=(30, 1))
    for n in range(30):
        ray(shell[n], -shell[n] / np.linalg.norm(shell[n]) + rng.uniform(-1e-3, 1e-3, size=3))
    return WC._case("depth64" if scene == "chain64" else scene, scene, np.asarray(origin), np.asarray(d, dtype=np.float64))


OUTSIDE = (-1, 130, 2 ** 31 - 1, -2 ** 31)     # numbers that name none of 130 rays


def dups():
    """130 box rays under a 200-entry list that holds every ray at least once, some twice -- in the same wave and in different waves --,
    numbers outside the ray arrays at list positions 0, 63, 64 and 127, and nothing but such numbers in its last eight entries (the last,
    partial wave is made of skipped entries only).  -> (case, the distinct valid entries, sorted)"""
    o, d = WC.box_rays(130, 17)
    rng = np.random.RandomState(18)
    dist = np.full(130, np.inf, dtype=F)
    dist[::3] = rng.uniform(0.5, 9.0, size=len(dist[::3])).astype(F)
    perm = rng.permutation(130).tolist()
    valid = [perm[0], perm[0]] + perm[1:] + perm[:57]       # 188 entries: perm[0] twice in a row, 57 rays again 130 entries later
    idx = []
    for p in range(192):
        idx.append(OUTSIDE[(0, 63, 64, 127).index(p)] if p in (0, 63, 64, 127) else valid.pop(0))
    assert not valid
    idx += [OUTSIDE[p % 4] for p in range(8)]
    idx = np.asarray(idx, dtype=np.int64).astype(np.int32)
    assert len(idx) == 200
    return WC._case("dups", "box", o, d, dist=dist, indices=idx), valid_entries(idx, 130)


def valid_entries(idx, n_rays):
    idx = np.asarray(idx, dtype=np.int64)
    return np.unique(idx[(idx >= 0) & (idx < n_rays)]).astype(np.int32)


def half_outside():
    """64 distinct valid entries, then 64 that name no ray: a whole wave of skipped lanes; the counters are defined here"""
    o, d = WC.box_rays(130, 19)
    rng = np.random.RandomState(20)
    idx = np.concatenate([rng.permutation(130)[:64], np.resize(np.asarray(OUTSIDE, dtype=np.int64), 64)]).astype(np.int32)
    dist = rng.uniform(0.5, 9.0, size=130).astype(F)
    dist[::2] = np.inf
    return WC._case("half_outside", "box", o, d, dist=dist, indices=idx)


def two_rays(n, seed):
    """n rays at the two triangles of `two`, from both sides of their planes"""
    rng = np.random.RandomState(seed)
    origin = np.stack([rng.uniform(-1.2, 1.7, n), rng.uniform(-1.2, 1.7, n), rng.uniform(0.0, 5.0, n)], axis=1)
    target = np.stack([rng.uniform(-0.8, 1.2, n), rng.uniform(-0.8, 1.2, n), np.where(np.arange(n) % 2 == 0, 2.0, 3.0)], axis=1)
    return origin.astype(F), WC._unit(target - origin)


def start_cases():
    """every node of the box's tree and of `two`'s as start node (the node counts come from the trees), 65 rays each"""
    out = []
    for scene, rays in (("box", WC.box_rays), ("two", two_rays)):
        for k in range(len(bvh(scene).nodes)):
            o, d = rays(65, 400 + k)
            out.append(WC._case("start_%s%d" % (scene, k), scene, o, d, start=k))
    return out


def a_leaf_start():
    """a start node that is a leaf of a tree with inner nodes"""
    leaf = is_leaf(bvh("box").nodes)
    return [c for c in start_cases() if c["scene"] == "box" and leaf[c["start"]]][0]


@functools.lru_cache(maxsize=None)
def walk_cases():
    return tuple([scaled(k) for k in SCALES + (-40,)] + [tiny_rays()] + [chain_rays(k) for k in CHAIN_SCENES] + [half_outside()] + start_cases())


def case(name):
    return [c for c in walk_cases() if c["name"] == name][0]


def expected(c, mutation=None, tree=None, **kw):
    """tests/wide_ref.py on a case -> (dist, visits); `tree` = another tree of the same scene (one read back from the device)"""
    b = bvh(c["scene"]) if tree is None else tree
    idx = c["indices"]
    if idx is not None:       # a number outside the ray arrays is skipped
        idx = idx[(idx >= 0) & (idx < len(c["dist"]))]
    return WR.wide_trace(b.nodes, b.tris, c["origin"], c["dir"], c["dist"], idir=c["idir"], indices=idx, start_node=c["start"],
                         mutation=mutation, **kw)


# ---- photon cases ----
def pattern(n, seed=5):
    """-> bool [n]: which rays are "hit" rays.  By block of 256 (b = i // 256, j = i % 256), b % 7: 0 none, 1 all, 2 j = 0 only, 3 j = 255 only,
    4 j in {63, 64, 127, 128, 191, 192} (the wave boundaries), 5 odd j, 6 a seeded coin."""
    i = np.arange(n)
    b, j = i // 256, i % 256
    coin = np.random.RandomState(seed).randint(0, 2, size=n).astype(bool)
    kind = b % 7
    return ((kind == 1) | ((kind == 2) & (j == 0)) | ((kind == 3) & (j == 255)) | ((kind == 4) & np.isin(j, (63, 64, 127, 128, 191, 192))) |
            ((kind == 5) & (j % 2 == 1)) | ((kind == 6) & coin))


def photon_rays(hit, seed):
    """hit rays: origin uniform in [-0.5, 0.5]^3 inside the inward box, a unit direction; the others: from (50, 0, 0) with direction x > 0"""
    n = len(hit)
    rng = np.random.RandomState(seed)
    o = rng.uniform(-0.5, 0.5, size=(n, 3)).astype(F)
    d = rng.randn(n, 3)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    miss = ~np.asarray(hit, dtype=bool)
    o[miss] = [50.0, 0.0, 0.0]
    d[miss, 0] = np.abs(d[miss, 0]) + F(0.01)
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


PHOTON_SIZES = {                      # name -> (lights, count); the scan takes 1024 blocks = 262 144 rays a round
    "one_round": (2, 131072),         # exactly one round
    "one_block_more": (2, 131200),    # one block into the second round
    "three_rounds": (2, 262400),      # the third round holds one block
    "odd_one_light": (1, 524801),     # ... and one ray in a block of its own
    "a_round_of_zeros": (2, 262400),  # blocks 1024 .. 2047 keep nothing: the carry passes through a round that adds nothing
}


def photon_pattern(name):
    lights, count = PHOTON_SIZES[name]
    hit = pattern(lights * count)
    if name == "a_round_of_zeros":
        hit[1024 * 256:2048 * 256] = False
    return hit


def odd_photon_rays():
    """64 + 3 rays of one light at `two` (both triangles in ONE leaf, normals +z, planes z = 2 and z = 3), interleaved:
      0 a zero direction from a point in the plane of the triangle tested last (0 / 0: a NaN, kept; the position NaN),
      1 a zero direction from above both planes (-x / 0 = -inf: kept, the position 0 * -inf = NaN),
      2 a zero direction from below both planes (+inf: no record),
      3 pointing away from the triangles from above them (a negative distance: the position lies behind the origin),
      4 an ordinary hit, 5 an ordinary miss."""
    last = bvh("two").tris["a"][-1]
    z_last = float(last[2])
    rays = []          # (origin, direction)
    for i in range(67):
        x, y = 0.05 + 0.003 * i, 0.2 - 0.002 * i       # over both triangles
        kind = i % 6
        if kind == 0:
            rays.append(([x, y, z_last], [0.0, 0.0, -0.0 if i % 12 else 0.0]))
        elif kind == 1:
            rays.append(([x, y, 4.0 + 0.01 * i], [0.0, 0.0, 0.0]))
        elif kind == 2:
            rays.append(([x, y, 1.0 - 0.01 * i], [0.0, -0.0, 0.0]))
        elif kind == 3:
            rays.append(([x, y, 5.0 + 0.01 * i], [0.001 * i, 0.0, 1.0]))
        elif kind == 4:
            rays.append(([x, y, 0.5], [0.0, 0.001 * i, 1.0]))
        else:
            rays.append(([x + 5.0, y, 0.0], [0.3, 0.0, 1.0]))
    origin, d = [r[0] for r in rays], [r[1] for r in rays]
    return np.asarray(origin, dtype=F), np.asarray(d, dtype=F)


def odd_photon_distances():
    o, d = odd_photon_rays()
    b = bvh("two")
    return WR.wide_trace(b.nodes, b.tris, o, d, np.full(len(o), np.inf, dtype=F))[0]


# ---- the photon scratch: SnailScene::wide[wideCount++ % 8] ----
SLOTS = 8                                # SNAIL_DEFER_SLOTS; photon call i of a fresh scene takes slot i % 8
SLOT_COUNTS = (300, 70001, 5, 4097)
SLOT_CALLS = 20


def slot_plan(i):
    """-> (rays, stream number) of call i.  Both cycles step once more at every turn round the slots (8 is a multiple of their periods:
    without the step slot s would see the same count on the same stream every time)."""
    k = i + i // SLOTS
    return SLOT_COUNTS[k % len(SLOT_COUNTS)], k % 2
