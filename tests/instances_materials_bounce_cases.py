"""The cases of the instanced bounce tests (tests/test_instances_materials_bounce_host.py, tests/test_gpu_instances_materials_bounce.py): those
of tests/instances_materials_cases.py -- main, degenerate, updated, quirk, deep -- by import, and ONE more, `mirror`, for what their mirrored
rays do not reach: nested single-triangle blocks with the UBER material on masked and on unmasked nested packets, and the nested (slot 0,
triId 0) quirk (the `quirk` case's own mirrored rays leave its one sheet almost at once: 28 nested hits, none beside triangle 0).  Chosen with
the restatement (tests/instances_materials_bounce_ref.py) alone, on the CPU; what the cases must exercise together is asserted on the
restatement's counters in tests/test_instances_materials_bounce_host.py.  Nothing here touches a device."""
from __future__ import annotations

import functools

import numpy as np

from snail_amd import FPSCamera
from tests import instances_materials_bounce_ref as IB
from tests import instances_materials_cases as K
from tests import instances_materials_ref as IM
from tests import materials_cases as MK
from tests import oracle_lib as O

FRAMES = [(96, 64), (70, 50)]       # 24 and 20 packets, the second with partial packets
# (case, resx, resy) of every frame the tests render; `deep` 64 x 64, nothing larger than 96 x 64
ALL = [("main", 96, 64), ("main", 70, 50), ("mirror", 96, 64), ("mirror", 70, 50), ("updated", 96, 64), ("quirk", 48, 32), ("deep", 64, 64),
       ("degenerate", 96, 64), ("degenerate", 70, 50)]


def mirror_instances():
    """(rot, tr, blas index); BLAS 0 = the sheet, 1 = the box.  Given order:
      0  box, the identity, at the origin: the MIRROR.  The camera looks at its face z = -0.5 from close by; its records are flat, so a full
         block of one triangle with a material that is not textured reflects about ONE normal (the plane's, bent a little): coherent rays
      1  sheet, the identity, BEHIND the camera: its backdrop (two large triangles of the shared UBER material) faces the mirror, so whole
         blocks of mirrored rays meet one triangle -- in packets the mirror fills (unmasked) and in packets across its upper and lower
         edge, whose rows are wholly on it or wholly off it (masked)
      2  box, an exact quarter turn about y, far behind and beside the backdrop with nothing behind it: the builder gives it slot 0, the turn
         brings the face of its triangle 0 towards the mirror, and mirrored quads across that triangle's outline have lanes that miss"""
    rot = np.stack([np.eye(3, dtype=np.float32), np.eye(3, dtype=np.float32), K.ROT90Y])
    tr = np.array([[0.0, 0.0, 0.0], [0.5, -0.2, -9.0], [-4.5, 0.0, -12.0]], dtype=np.float32)
    return rot, tr, np.array([1, 0, 1], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def case(name):
    """instances_materials_cases.case(name), or the `mirror` case in the same form"""
    if name != "mirror":
        return K.case(name)
    m = K.case("main")
    rot, tr, bi = mirror_instances()
    cam = FPSCamera(np.array([0.0, 0.0, -1.6], dtype=np.float32), 0.0, 0.0).camera()
    return dict(tvs=m["tvs"], oscs=m["oscs"], per_blas=m["per_blas"], rot=rot, tr=tr, bi=bi, ref=K.cpu_ref(m["oscs"], rot, tr, bi), cams={96: cam, 70: cam},
                lights=m["lights"])


def materials_ref(name, transform=True):
    c = case(name)
    return IM.InstMaterialsRef(c["ref"], c["per_blas"], MK.ref_materials(K.DESCS), K.ref_textures(), transform=transform)


def lights_of(name, key):
    """the case's lights, none, or eight lights before the main case's sheets with radii large enough that none is culled everywhere"""
    if key == "case":
        return case(name)["lights"]
    if key == "none":
        return None
    return np.array([[-2.0 + 0.6 * k, -0.8 + 0.3 * k, -1.6 - 0.2 * k, 1.0 - 0.1 * k, 0.5, 0.2 + 0.1 * k, 3.0 + 0.8 * k] for k in range(8)], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def reference(name, resx, resy, mode=O.MODE_IEEE, lights_key="case", mutation=None):
    """the restatement's frame, TreeStats, per-packet intermediates, packet list and counters: computed once per argument list, shared, never
    changed"""
    c = case(name)
    d = IB.BounceDiag()
    frame, st, inter, xy = IB.InstBounceRef(materials_ref(name), mutation).render(c["cams"][resx].as_array13(), resx, resy, lights_of(name, lights_key), mode=mode,
                                                                                  diag=d)
    for a in (frame, st, xy):
        a.setflags(write=False)
    return frame, st, inter, xy, d


@functools.lru_cache(maxsize=None)
def plain_reference(name, resx, resy, mode=O.MODE_IEEE, lights_key="case"):
    """the frame WITHOUT the bounce (tests/instances_materials_ref.py): what flags == 0 must give"""
    c = case(name)
    frame, st, _smp, _xy = materials_ref(name).render(c["cams"][resx].as_array13(), resx, resy, lights_of(name, lights_key), mode=mode)
    frame.setflags(write=False); st.setflags(write=False)
    return frame, st
