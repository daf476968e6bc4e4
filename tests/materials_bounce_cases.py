"""The cases of the bounce under full shading (tests/test_gpu_materials_bounce.py, tests/test_materials_bounce_host.py): the cases of
tests/materials_cases.py, taken through materials_cases.case, and one more, `mirror`: none of those reaches branch (a) -- one triangle for a
full block -- on a MASKED nested packet, the one place where the packet's hasMask shows.  Chosen with the restatement
(tests/materials_bounce_ref.py) alone, on the CPU; what each must exercise is asserted on the restatement's diagnostics by
tests/test_materials_bounce_host.py.  Nothing here touches the product library."""
from __future__ import annotations

import functools

import numpy as np

from snail_amd import FPSCamera
from tests import materials_bounce_ref as B
from tests import materials_cases as K
from tests import materials_ref as M
from tests import oracle_lib as O

FRAMES = [(96, 64), (70, 50)]


def mirror_scene():
    """A floor of two triangles below the camera and, behind its far edge, a wall of two large triangles: the floor fills the lower part of
    the frame only (partially hit primary packets -> masked nested packets), and what it mirrors is the wall, whose triangles are large enough
    that whole blocks of mirrored rays land on one of them; mirrored rays near the floor's far edge pass below the wall and miss."""
    a, b, c, d = (-2.0, 0.0, 0.0), (2.0, 0.0, 0.0), (2.0, 0.0, 4.0), (-2.0, 0.0, 4.0)
    w0, w1, w2, w3 = (-8.0, 0.5, 6.0), (8.0, 0.5, 6.0), (8.0, 9.0, 6.0), (-8.0, 9.0, 6.0)
    return np.ascontiguousarray(np.array([(a, c, b), (a, d, c), (w0, w1, w2), (w0, w2, w3)], dtype=np.float32))


@functools.lru_cache(maxsize=None)
def case(name):
    """as materials_cases.case"""
    if name != "mirror":
        return K.case(name)
    tv = mirror_scene()
    osc = O.OracleScene(tv)
    uv, nrm, flat = K.vertex_data(osc, tv, 31)
    descs = [("simple", (0.8, 0.7, 0.6), True), ("uber", (0.2, 0.5, 0.9), (0.9, 0.2, 0.1), 0.0), ("tex", 0, True)]
    mmap = [0, 0, 1, 2]
    mat_index = np.arange(len(tv), dtype=np.int32)
    cam = FPSCamera(np.array([0.0, 1.5, -2.0], dtype=np.float32), 0.0, 0.35).camera()
    # the first reaches floor and wall; the second, close to the wall's left end, has a radius that lets the packet-level cull remove it for
    # the nested packets whose mirrored hits lie on the wall's right half
    lights = np.array([[0.5, 3.0, 1.0, 1.0, 0.9, 0.8, 30.0], [-6.0, 3.0, 5.0, 0.4, 0.6, 1.0, 4.0]], dtype=np.float32)
    return dict(cam70=cam, tv=tv, osc=osc, uv=uv, nrm=nrm, mat_index=mat_index, flat=flat, descs=descs, material_map=mmap, textures=K.TEXTURES(), cam=cam, lights=lights)


def camera(name, resx):
    c = case(name)
    return c["cam70"] if resx == 70 else c["cam"]


def eight_lights(name):
    """eight lights spread over the case's box, radii large enough that most reach something"""
    osc = case(name)["osc"]
    return K.centre_lights(osc, [(0.1 + 0.11 * k, 0.3 + 0.08 * k, 0.2 + 0.09 * k, (1.0 - 0.1 * k, 0.5, 0.2 + 0.1 * k), 0.5 + 0.15 * k) for k in range(8)])


def lights_of(name, key):
    return case(name)["lights"] if key == "case" else None if key == "none" else eight_lights(name)


def materials_ref(name):
    c = case(name)
    return M.MaterialsRef(c["osc"], c["uv"], c["nrm"], c["mat_index"], c["flat"], c["material_map"], K.ref_materials(c["descs"]), [M.RefTexture(t) for t in c["textures"]])


@functools.lru_cache(maxsize=None)
def reference(name, resx, resy, mode, lights_key="case"):
    """the restatement's bounce frame, TreeStats, per-packet intermediates, packet list and diagnostics: computed once, shared, never changed"""
    d = B.BounceDiag()
    frame, st, inter, xy = B.BounceRef(materials_ref(name)).render(camera(name, resx).as_array13(), resx, resy, lights_of(name, lights_key), mode=mode, diag=d)
    for a in (frame, st, xy):
        a.setflags(write=False)
    return frame, st, inter, xy, d
