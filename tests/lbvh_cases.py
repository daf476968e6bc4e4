"""Seeded inputs for the device LBVH builder (tests/test_lbvh_ref_host.py, tests/test_gpu_lbvh.py): each is built for one thing natural
meshes do not reach, and tests/test_lbvh_ref_host.py asserts with the restatement alone that it reaches it."""
import functools

import numpy as np

from tests import lbvh_ref as R
from tests.test_bvh_fast_host import identical_tris, soup

F = np.float32
MAX_LEAF = (1, 4, 64)
# the root leaf (n <= max_leaf), a root over two collapsed children (65 at 64), the 256-thread block edge, several blocks
SOUP_SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1025, 5003)


def boxed_tri(lo, hi):
    """a triangle of positive area whose box is exactly [lo, hi] on every axis where lo < hi"""
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    return np.array([lo[0], lo[1], lo[2], hi[0], lo[1], hi[2], lo[0], hi[1], hi[2]], F)


def centred_tri(c, h):
    c, h = np.asarray(c, np.float64), np.asarray(h, np.float64) * np.ones(3)
    return boxed_tri(c - h, c + h)


def identical300():
    """one triangle 300 times: one Morton code, the whole tree comes from the index in the key's low word"""
    return identical_tris(300)


def clusters():
    """8 cells x 40 triangles: in each cell all 40 boxes share their centre exactly (dyadic coordinates) and differ in size"""
    rows = [centred_tri((cx, cy, cz), (j + 1) / 64.0) for cx in (2.0, 6.0) for cy in (2.0, 6.0) for cz in (2.0, 6.0) for j in range(40)]
    return np.array(rows, F)


def flat():
    """every vertex at one z: the scene has no extent on that axis (ext > 0 ? ... : 0)"""
    tv = soup(200, 311).reshape(-1, 3, 3).copy()
    tv[:, :, 2] = F(0.75)
    return tv.reshape(-1, 9)


COMB_CELL0 = slice(30, 286)


def comb():
    """A comb-shaped key set: the thirty one-bit Morton codes (one tiny triangle each, its centre at (2^b + 0.5) / 1024 on one axis and
    0.25 / 1024 on the others), 256 identical triangles in cell 0, and two corner triangles that pin the bounds to [0, 1]^3.  Karras'
    search runs its longest ranges here, and the tree is some 30 levels of comb over the index tree of cell 0."""
    h, base = 2.0 ** -13, 0.25 / 1024
    rows = []
    for k in range(3):
        for b in range(10):
            c = [base] * 3
            c[k] = (2.0 ** b + 0.5) / 1024
            rows.append(centred_tri(c, h))
    rows += [centred_tri([base] * 3, h)] * 256
    rows.append(boxed_tri([0, 0, 0], [h, h, h]))
    rows.append(boxed_tri([1 - h] * 3, [1, 1, 1]))
    return np.array(rows, F)


WALLS_LO, WALLS_EXT = np.array([-3.0, 1.0, 10.0]), np.array([8.0, 1.0, 4.0])
WALLS_CELLS = (1, 2, 511, 512, 513, 1023)


def walls():
    """Triangles lying in the six bounding planes of the scene (centre on the scene minimum: t = 0; on the maximum: t = 1, 1024 cells,
    clamped to 1023), and triangles whose centre sits exactly on the cell boundary k / 1024 (the extents are powers of two)."""
    rng = np.random.default_rng(77)
    lo, ext = WALLS_LO, WALLS_EXT
    rows = []
    for k in range(3):
        for side in (0.0, 1.0):
            for _ in range(6):
                a = lo + ext * rng.integers(64, 448, 3) / 512.0
                b = a + ext * rng.integers(1, 64, 3) / 512.0
                a[k] = b[k] = lo[k] + side * ext[k]
                rows.append(boxed_tri(a, b))
    for k in range(3):
        for cell in WALLS_CELLS:
            c = lo + ext * rng.integers(64, 448, 3) / 512.0
            c[k] = lo[k] + ext[k] * cell / 1024.0
            rows.append(centred_tri(c, ext / 4096.0))
    return np.array(rows, F)


WALLS_BOUNDARY = slice(36, 36 + 3 * len(WALLS_CELLS))


def scaled(which):
    tv = soup(257, 557)
    if which == "up":
        return (tv * F(2.0 ** 20)).astype(F)
    if which == "down":
        return (tv * F(2.0 ** -20)).astype(F)
    return (tv + F(1.0e6)).astype(F)


CASES = {"soup%d" % n: functools.partial(soup, n, 300 + n) for n in SOUP_SIZES}
CASES.update(identical300=identical300, clusters=clusters, flat=flat, comb=comb, walls=walls, scaled_up=functools.partial(scaled, "up"),
             scaled_down=functools.partial(scaled, "down"), shifted=functools.partial(scaled, "shift"))
NAMES = list(CASES)
ALL = [(name, m) for name in NAMES for m in MAX_LEAF]


@functools.lru_cache(maxsize=None)
def verts(name):
    tv = np.ascontiguousarray(CASES[name](), F).reshape(-1, 9)
    tv.setflags(write=False)
    return tv


@functools.lru_cache(maxsize=None)
def ref(name, max_leaf):
    """the restated tree of a case: (nodes, perm, depth), computed once and shared"""
    nodes, perm, depth = R.build(verts(name), max_leaf)
    nodes.setflags(write=False); perm.setflags(write=False)
    return nodes, perm, depth


# ---- inputs of the flag tests ----
def magnitude_tri():
    """every record field (a, b - a, c - a) within 1e9, the box maximum 1.7e9 beyond it"""
    return np.array([[9e8, 0, 0, 1.7e9, 1e3, 0, 9e8, 1e3, 0]], F)


def zero_area_soup():
    tv = soup(300, 91).copy()
    tv[17, 3:6] = tv[17, 0:3]; tv[17, 6:9] = tv[17, 0:3]
    return tv


def nonfinite_soup(value):
    tv = soup(300, 91).copy()
    tv[123, 4] = value
    return tv


# ---- what the walks of tests/test_gpu_lbvh.py look at ----
WALK_TREES = (("soup1025", 64), ("comb", 1), ("identical300", 4))


class Region:
    """The box the camera, the packets and the light are placed by (tests.util's packet makers read nodes[0] of what they are given): the
    triangles the walk is aimed at -- cell 0 of the comb, whose other triangles are specks in a unit cube -- padded by a quarter of the
    largest extent, so that a flat or a single-triangle scene still has a box with a volume."""

    def __init__(self, name):
        tv = verts(name)
        v = (tv[COMB_CELL0] if name == "comb" else tv).reshape(-1, 3)
        lo, hi = v.min(axis=0), v.max(axis=0)
        pad = F(0.25) * (hi - lo).max()
        self.nodes = np.zeros(1, dtype=R.NODE_DTYPE)
        self.nodes["bmin"][0], self.nodes["bmax"][0] = lo - pad, hi + pad

    def camera(self):
        from snail_amd import survey_camera
        nd = self.nodes[0]
        return survey_camera(np.concatenate([nd["bmin"], nd["bmax"], nd["bmin"]]).reshape(1, 9))

    def light(self):
        nd = self.nodes[0]
        c, e = (nd["bmin"] + nd["bmax"]) * F(0.5), nd["bmax"] - nd["bmin"]
        return np.array([[c[0], c[1] + 0.35 * e[1], c[2], 1.0, 0.9, 0.8, 2.0 * float(e.max())]], F)
