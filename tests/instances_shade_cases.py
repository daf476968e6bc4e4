"""The instanced scenes, cameras and lights of the lit-frame tests (tests/test_instances_shade_host.py, tests/test_gpu_instances_shade.py),
buildable without a GPU: the top-level tree through tests/dbvh_ref.py's restated builder, so that the restatement alone can be asked
whether a case exercises what the tests claim (hits, lit and shadowed pixels, culled lights, mirrored hits).  Test infrastructure only."""
from __future__ import annotations

import os

import numpy as np

from snail_amd import FPSCamera, scenes, survey_camera
from tests import dbvh_ref as R
from tests import dbvh_shade_ref as S
from tests import oracle_lib as O

GOLD = os.path.join(os.path.dirname(__file__), "golden")
_tv = {}
_orc = {}


def tri_verts(name):
    if name not in _tv:
        if name == "lancia":
            _tv[name] = np.load(os.path.join(GOLD, "lancia_tris.npz"))["tris"].reshape(-1, 9).astype(np.float32)
        elif name == "chain":
            _tv[name] = scenes.chain()
        else:
            _tv[name] = scenes.scene_by_name(name)
    return _tv[name]


def oracle(name):
    if name not in _orc:
        _orc[name] = O.OracleScene(tri_verts(name))
    return _orc[name]


def layout(names, n, seed, spread=1.0):
    """rotations, translations, BLAS indices of a field (the set-up of tests/test_gpu_instances.py::make)"""
    lo = np.min([oracle(nm).nodes[0]["bmin"] for nm in names], axis=0)
    hi = np.max([oracle(nm).nodes[0]["bmax"] for nm in names], axis=0)
    rot, tr, bi = scenes.instance_field(lo, hi, n, seed=seed, n_blas=len(names))
    return rot, (tr * np.float32(spread)).astype(np.float32), bi


def cpu_ref(names, rot, tr, bi):
    """The restatement's scene, its tree from the restated builder (equal to snail_instances_build's: tests/test_instances_host.py)"""
    xf = np.concatenate([np.asarray(rot, dtype=np.float32).reshape(-1, 9), np.asarray(tr, dtype=np.float32).reshape(-1, 3)], axis=1)
    bb = np.stack([np.concatenate([oracle(nm).nodes[0]["bmin"], oracle(nm).nodes[0]["bmax"]]) for nm in names]).astype(np.float32)
    nodes, _depth, perm = R.build(xf, bi, bb)
    return R.Ref([oracle(nm) for nm in names], nodes, xf[perm], np.asarray(bi)[perm])


def field_camera(nodes, shrink=1.0):
    """survey_camera over the field's box shrunk about its centre: shrink < 1 moves the camera in, so that more of the frame is covered"""
    nd = nodes[0]
    c, h = (nd["bmin"] + nd["bmax"]) * np.float32(0.5), (nd["bmax"] - nd["bmin"]) * np.float32(0.5 * shrink)
    return survey_camera(np.concatenate([c - h, c + h, c - h]).astype(np.float32).reshape(1, 9))


def field_lights(nodes, spec):
    """spec = [(fx, fy, fz, (r, g, b), radius as a fraction of the field box's diagonal)]: positions as fractions of the field's box"""
    lo, hi = nodes[0]["bmin"].astype(np.float64), nodes[0]["bmax"].astype(np.float64)
    diag = float(np.linalg.norm(hi - lo))
    return np.array([[*(lo + (hi - lo) * np.array(f[:3])), *f[3], f[4] * diag] for f in spec], dtype=np.float32)


# name -> (BLAS names, instances, seed, spread, resx, resy, camera (field_camera's shrink, or "inside": in the middle of the last, identity, instance), lights)
# Seeds are those of tests/test_gpu_instances.py; cameras and lights were chosen with the restatement alone (no GPU) so that every frame meets
# the conditions the tests assert on it (hit, lit and shadowed pixels, culled packets, mirrored hits).
WHITE, WARM = (1.0, 1.0, 1.0), (1.0, 0.7, 0.4)
FIELD_CASES = {
    "field": (["box", "lancia"], 24, 3, 0.1, 128, 96, 0.6, [(0.5, 0.8, 0.5, WHITE, 1.0), (0.3, 0.5, 0.4, WARM, 0.12)]),
    "overlap": (["box"], 16, 8, 0.002, 96, 64, 0.6, [(0.5, 3.0, 0.5, WHITE, 6.0), (-1.5, 0.3, 2.5, WARM, 6.0)]),
    "inside": (["lancia"], 8, 5, 1.0, 96, 64, "inside", [(0.5, 0.6, 0.5, WHITE, 1.0), (0.45, 0.5, 0.55, WARM, 0.5)]),
    "deep": (["chain", "box"], 6, 4, 0.05, 64, 64, 0.25, [(0.5, -2.0, 0.5, WHITE, 6.0), (2.5, 2.5, 2.5, WARM, 6.0)]),
}


def case(name):
    """-> (names, rot, tr, bi, resx, resy, camera, lights7, restatement scene) of a FIELD_CASES entry"""
    names, n, seed, spread, resx, resy, camk, lspec = FIELD_CASES[name]
    rot, tr, bi = layout(names, n, seed, spread)
    ref = cpu_ref(names, rot, tr, bi)
    if camk == "inside":
        c = oracle(names[0]).nodes[0]
        cam = FPSCamera(((c["bmin"] + c["bmax"]) * 0.5).astype(np.float32), 0.3, 0.1).camera()
    else:
        cam = field_camera(ref.nodes, camk)
    return names, rot, tr, bi, resx, resy, cam, field_lights(ref.nodes, lspec), ref
