"""The case of the tests of include/snail_instances_materials_dynamic.h (tests/test_instances_materials_dynamic_host.py,
tests/test_gpu_instances_materials_dynamic.py): instances_materials_cases.case("main") whose sheet BLAS deforms between two poses A and B by a
smooth displacement of every vertex (shared vertices stay shared), as tests/test_gpu_materials_dynamic.py's poses do; the box BLAS stays built
from host triangles.  Everything is host data, computed once and read-only; nothing here touches a device.  What the poses must exercise --
another permutation and another root box, so that neither stale records nor a stale top-level tree could pass -- is asserted here, on the
host's fast builder alone (check_poses)."""
from __future__ import annotations

import functools

import numpy as np

from snail_amd import HostBVH
from tests import instances_materials_cases as IK

F = np.float32
SHEET, BOX = 0, 1


@functools.lru_cache(maxsize=None)
def poses():
    """-> dict(A = (tv, nrm), B = (tv, nrm) of the sheet; uv, mat_index, flat, material_map of the sheet; box = (tv, host 5-tuple);
    rot, tr, bi, cams, lights of the main case)"""
    c = IK.case("main")
    tvA = np.ascontiguousarray(c["tvs"][SHEET], dtype=F).reshape(-1, 3, 3)
    uv, nrmA, mat_index, flat, mmap = c["per_blas"][SHEET]
    x, y = tvA[..., 0].astype(np.float64), tvA[..., 1].astype(np.float64)
    tvB = tvA.copy()
    tvB[..., 2] = (tvA[..., 2] + 0.35 * np.sin(1.9 * x + 0.4) * np.cos(1.3 * y - 0.2)).astype(F)
    tvB[..., 0] = (tvA[..., 0] + 0.08 * np.sin(2.1 * y)).astype(F)
    nrmA = np.ascontiguousarray(nrmA, dtype=F)
    rng = np.random.RandomState(47)
    nrmB = (nrmA + (rng.rand(*nrmA.shape) - 0.5) * 0.5).astype(F)
    out = dict(A=(tvA, nrmA), B=(tvB, nrmB), uv=np.ascontiguousarray(uv, dtype=F), mat_index=np.ascontiguousarray(mat_index, dtype=np.int32),
               flat=np.ascontiguousarray(flat).astype(np.uint8), material_map=list(mmap),
               box=(np.ascontiguousarray(c["tvs"][BOX], dtype=F).reshape(-1, 3, 3), c["per_blas"][BOX]),
               rot=c["rot"], tr=c["tr"], bi=c["bi"], cams=c["cams"], lights=c["lights"])
    for v in (tvA, tvB, nrmA, nrmB, out["uv"], out["mat_index"], out["flat"]):
        v.setflags(write=False)
    return out


def sheet_data(pose, nrm=None):
    """the host 5-tuple of the sheet in a pose (nrm: other normals than the pose's own)"""
    p = poses()
    return (p["uv"], p[pose][1] if nrm is None else nrm, p["mat_index"], p["flat"], p["material_map"])


@functools.lru_cache(maxsize=None)
def fast_trees():
    """the host's fast tree of the sheet in each pose (HostBVH.build_fast: byte-equal to the device's, tests/test_gpu_bvh_fast.py)"""
    p = poses()
    return {k: HostBVH.build_fast(p[k][0]) for k in "AB"}


def root_box(bvh):
    n0 = bvh.nodes[0]
    return np.concatenate([n0["bmin"], n0["bmax"]]).astype(F)


def check_poses():
    """the two conditions that hold for the twin alone, on the CPU: the poses' trees number the triangles differently, and the sheet's root
    box differs (so the top-level tree must be rebuilt too)"""
    t = fast_trees()
    pa, pb = np.asarray(t["A"].perm), np.asarray(t["B"].perm)
    n = len(poses()["uv"])
    assert sorted(pa.tolist()) == list(range(n)) and sorted(pb.tolist()) == list(range(n))
    moved = int((pa != pb).sum())
    assert moved > n // 8, moved
    ba, bb = root_box(t["A"]), root_box(t["B"])
    assert (ba != bb).any(), (ba, bb)
    return moved, ba, bb
