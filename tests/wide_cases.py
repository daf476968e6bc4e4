"""Scenes and rays of the tests of include/snail_wide.h, shared by tests/test_wide_host.py (which shows that they discriminate the
mutations of tests/wide_ref.py) and tests/test_gpu_wide.py / test_gpu_photons.py (which hold the device to wide_ref on them).

A case = dict(name, scene, origin [n, 3], dir [n, 3], idir [n, 3] or None, dist [n], indices or None, start).  Everything is seeded."""
import functools

import numpy as np

from snail_amd import HostBVH, scenes

F = np.float32


def two_triangles():
    """Two triangles, which the builder keeps in ONE leaf: the root is a leaf and no box is ever tested."""
    return np.asarray([[[0.0, 0.0, 2.0], [1.5, 0.0, 2.0], [0.0, 1.5, 2.0]],
                       [[0.25, 0.25, 3.0], [-1.0, 0.25, 3.0], [0.25, -1.0, 3.0]]], dtype=F)


def offcentre(n=300, seed=71):
    """Random triangles far from the origin (|a| ~ 300 against edges of a few units): the float grid at `a` is coarser than the grid of
    an edge, which is what `edited_records` below needs."""
    rng = np.random.RandomState(seed)
    c = np.asarray([311.7, -287.3, 295.1]) + rng.uniform(-3.0, 3.0, size=(n, 1, 3))
    return np.ascontiguousarray((c + rng.uniform(-2.0, 2.0, size=(n, 3, 3))).astype(F))


def edited_records(tris, seed=73):
    """Triangle records whose stored edges carry bits BELOW the float grid at `a` (a caller hands in records, not vertices: include/snail_hip.h),
    with t0 / it0 / plane computed from those stored edges as Triangle::ComputeData does (src/triangle.h:123-131).  For records made from
    vertices (ba + a) - a == ba always; here it rounds, so the edges, normal and t0 that Collide0 recomputes differ from the stored ones."""
    rng = np.random.RandomState(seed)
    t = tris.copy()
    with np.errstate(all="ignore"):
        for k in ("ba", "ca"):
            t[k] = (t[k].astype(np.float64) * (1.0 + rng.uniform(-3e-6, 3e-6, size=t[k].shape))).astype(F)
        b, c, a = t["ba"], t["ca"], t["a"]
        nrm = np.stack([b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1], b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2], b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]], axis=1)
        ln = np.sqrt(nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1] + nrm[:, 2] * nrm[:, 2])
        nrm = nrm * (F(1.0) / ln)[:, None]
        t["t0"] = ln
        t["it0"] = F(1.0) / ln
        t["plane"][:, :3] = nrm
        t["plane"][:, 3] = nrm[:, 0] * a[:, 0] + nrm[:, 1] * a[:, 1] + nrm[:, 2] * a[:, 2]
    return t


SCENES = {
    "two": two_triangles,
    "edited": offcentre,
    "box": scenes.box_scene,
    "chain": scenes.chain,
    "offgrid": lambda: scenes.offgrid(n_blob=500),
}


@functools.lru_cache(maxsize=None)
def verts(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def bvh(name):
    """The sweep builder's tree of the scene (HostBVH: TRI_DTYPE / NODE_DTYPE records); "edited": over edited_records."""
    if name != "edited":
        return HostBVH.build(verts(name))
    import ctypes as C
    from snail_amd import _lib
    from snail_amd.bvh import NODE_DTYPE
    tris = edited_records(HostBVH.triangles(verts(name)))
    nodes = np.zeros(2 * len(tris) + 2, dtype=NODE_DTYPE)
    perm = np.zeros(len(tris), dtype=np.int32)
    nn, depth = C.c_int(0), C.c_int(0)
    _lib.check(_lib.lib().snail_bvh_build(_lib.ptr(tris), len(tris), _lib.ptr(nodes), C.addressof(nn), C.addressof(depth), _lib.ptr(perm)), "snail_bvh_build")
    return HostBVH(tris, np.ascontiguousarray(nodes[:nn.value]), depth.value, perm)


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def _case(name, scene, origin, dir, dist=None, idir=None, indices=None, start=0):
    origin = np.ascontiguousarray(origin, dtype=F).reshape(-1, 3)
    dir = np.ascontiguousarray(dir, dtype=F).reshape(-1, 3)
    n = len(origin)
    dist = np.full(n, np.inf, dtype=F) if dist is None else np.ascontiguousarray(dist, dtype=F)
    assert len(dir) == n and len(dist) == n
    return dict(name=name, scene=scene, origin=origin, dir=dir, idir=idir, dist=dist, indices=indices, start=start)


def box_rays(n, seed):
    """n rays at the box: every other one from inside, the rest from a shell around it aimed near its middle."""
    rng = np.random.RandomState(seed)
    inside = rng.uniform(-0.9, 0.9, size=(n, 3))
    shell = _unit(rng.randn(n, 3)).astype(np.float64) * rng.uniform(2.5, 6.0, size=(n, 1))
    origin = np.where((np.arange(n) % 2 == 0)[:, None], inside, shell)
    target = rng.uniform(-1.2, 1.2, size=(n, 3))
    d = np.where((np.arange(n) % 2 == 0)[:, None], rng.randn(n, 3), target - origin)
    return origin.astype(F), _unit(d)


def root_leaf():
    # towards the triangles, away from them (negative distances must come back), past them, and parallel to them
    origin = [[0.3, 0.3, 0.0], [0.3, 0.3, 5.0], [0.3, 0.3, 2.5], [5.0, 5.0, 0.0], [0.1, 0.1, 0.0], [-0.5, -0.5, 4.0], [0.3, 0.3, 0.0]]
    d = [[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.1, 0.05, 1.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]
    return _case("root_leaf", "two", origin, d)


def box_sizes():
    return [_case("box_%d" % n, "box", *box_rays(n, 100 + n)) for n in (1, 63, 64, 65, 130)]


def box_subset():
    o, d = box_rays(130, 7)
    rng = np.random.RandomState(8)
    idx = rng.permutation(130)[:77].astype(np.int32)      # a shuffled proper subset
    dist = rng.uniform(0.5, 9.0, size=130).astype(F)      # the rays left out keep these bytes
    return _case("box_subset", "box", o, d, dist=dist, indices=idx)


def box_start(k):
    o, d = box_rays(65, 20 + k)
    return _case("box_start%d" % k, "box", o, d, start=k)


def box_idir():
    """idir is used as given: once what 1 / dir gives (the same bytes as NULL), once a skewed one no caller would compute."""
    o, d = box_rays(65, 31)
    with np.errstate(all="ignore"):
        inv = (F(1.0) / d).astype(F)
    skew = (inv * np.asarray([1.5, 0.75, -1.0], dtype=F)).astype(F)
    return [_case("box_idir_same", "box", o, d, idir=inv), _case("box_idir_skew", "box", o, d, idir=skew)]


def axis_parallel():
    """Axis-parallel rays from origins ON the box's planes (0 * inf = NaN in the slabs) and zero directions (every 1 / dir infinite; a zero
    direction in a triangle's plane gives a NaN distance, which the select keeps and fminf would drop)."""
    origin, d = [], []
    for axis in range(3):
        for sign in (1.0, -1.0):
            for plane in (-1.0, 1.0):
                for other in (0.0, 0.5, -1.0, 1.0):
                    o = [other, other * 0.5, other]
                    o[(axis + 1) % 3] = plane            # on a plane the ray runs parallel to
                    o[axis] = -3.0 * sign
                    e = [0.0, 0.0, 0.0]
                    e[axis] = sign
                    origin.append(o); d.append(e)
    for o in ([0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [-1.0, 0.5, 0.25], [0.5, -1.0, 0.5], [0.25, 0.25, 1.0], [3.0, 0.0, 0.0], [1.0, 1.0, -1.0]):
        origin.append(o); d.append([0.0, 0.0, 0.0])
        origin.append(o); d.append([-0.0, 0.0, -0.0])
    return _case("axis_parallel", "box", origin, d)


def prune():
    """Initial distances that prune: below the nearest hit, negative, NaN, +inf -- the same rays under each."""
    o, d = box_rays(16, 41)
    origin = np.concatenate([o] * 5)
    dd = np.concatenate([d] * 5)
    dist = np.concatenate([np.full(16, v, dtype=F) for v in (0.05, -1.0, np.nan, np.inf, 100.0)])
    return _case("prune", "box", origin, dd, dist=dist)


def chain_rays():
    """Down the chain (the deepest stack; the last leaf holds more than 64 triangles), straight and swaying."""
    rng = np.random.RandomState(51)
    n = 96
    origin = np.stack([np.full(n, 14.0), rng.uniform(-0.5, 2.5, size=n), rng.uniform(-0.5, 2.5, size=n)], axis=1)
    target = np.stack([np.zeros(n), rng.uniform(-0.02, 0.02, size=n), rng.uniform(-0.02, 0.02, size=n)], axis=1)
    d = _unit(target - origin)
    # the chain shrinks to ~1e-24 around the origin: only rays ALONG the x axis, within that of it, enter every box down to the last leaf
    e = np.asarray([0.0, 1e-24, -1e-24, 4e-24, 1e-20, 1e-12])
    for k, (x, dx) in enumerate(((-1.0, 1.0), (14.0, -1.0))):
        origin[6 * k:6 * k + 6] = np.stack([np.full(6, x), e, e * 0.5], axis=1)
        d[6 * k:6 * k + 6] = [dx, 0.0, 0.0]
    return _case("chain", "chain", origin, d)


def edited_rays():
    rng = np.random.RandomState(72)
    n = 200
    c = np.asarray([311.7, -287.3, 295.1])
    origin = c + rng.uniform(-7.0, 7.0, size=(n, 3))
    return _case("edited", "edited", origin, _unit(c + rng.uniform(-2.0, 2.0, size=(n, 3)) - origin))


FUZZ_RAYS = 2000


def fuzz():
    """2 000 seeded rays on offgrid(n_blob = 500): full mantissas around an origin far from zero."""
    rng = np.random.RandomState(61)
    n = FUZZ_RAYS
    c = np.asarray(scenes.OFFGRID_ORIGIN, dtype=np.float64)
    origin = c[None, :] + rng.uniform(-22.0, 22.0, size=(n, 3))
    target = c[None, :] + rng.uniform(-12.0, 12.0, size=(n, 3))
    d = np.where((np.arange(n) % 4 == 0)[:, None], rng.randn(n, 3), target - origin)
    dist = np.full(n, np.inf, dtype=F)
    dist[::7] = rng.uniform(0.5, 30.0, size=len(dist[::7])).astype(F)
    return _case("fuzz", "offgrid", origin, _unit(d), dist=dist)


@functools.lru_cache(maxsize=None)
def small_cases():
    return tuple([root_leaf()] + box_sizes() + [box_subset(), box_start(1), box_start(2)] + box_idir() + [axis_parallel(), prune(), chain_rays(), edited_rays()])


def expected(case, mutation=None):
    """tests/wide_ref.py on a case -> (dist, visits)."""
    from tests import wide_ref
    b = bvh(case["scene"])
    return wide_ref.wide_trace(b.nodes, b.tris, case["origin"], case["dir"], case["dist"], idir=case["idir"], indices=case["indices"],
                               start_node=case["start"], mutation=mutation)
