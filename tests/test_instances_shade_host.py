"""Lit frames of instanced scenes, the parts that need no GPU: the test-side restatement tests/dbvh_shade_ref.py is pinned to the oracle's
Scene::RayTrace (one identity instance reproduces every operand bit of the plain scene), and the new C-ABI is a contract: the header is
plain C and every new symbol is exported by libsnailhip.so."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import dbvh_shade_ref as S
from tests import instances_shade_cases as K
from tests import oracle_lib as O
from tests import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "snail_amd")


def identity_ref(name):
    return K.cpu_ref([name], np.eye(3, dtype=np.float32)[None], np.zeros((1, 3), np.float32), np.zeros(1, np.int32))


def scene_lights(name, cam):
    """two lights: a wide one beside the camera, and one inside the scene's box whose radius leaves part of the scene beyond its reach"""
    nd = K.oracle(name).nodes
    lights = K.field_lights(nd, [(0.5, 0.8, 0.5, K.WHITE, 4.0), (0.3, 0.4, 0.6, K.WARM, 0.4)])
    lights[0, :3] = cam.as_array13()[:3] + np.float32(0.25)
    return lights


@pytest.mark.parametrize("mode", [O.MODE_IEEE, O.MODE_SSE], ids=["ieee", "host_sse"])
@pytest.mark.parametrize("reflections", [False, True], ids=["plain", "reflections"])
@pytest.mark.parametrize("name", ["box", "lancia"])
def test_restatement_of_an_identity_instance_equals_the_oracle(name, reflections, mode):
    """Frame bytes only: the instanced inner walk runs in exact mode and counts differently, so TreeStats are not compared here."""
    resx, resy = 64, 48
    cam = U.camera_for(name, K.tri_verts(name))
    lights = scene_lights(name, cam)
    diag = S.Diag()
    got, _ = S.ShadeRef(identity_ref(name)).render(cam.as_array13(), resx, resy, lights, reflections=reflections, mode=mode, diag=diag)
    want, _ = K.oracle(name).render_whitted(cam.as_array13(), resx, resy, lights, mode=mode, reflections=reflections)
    print(name, reflections, mode, "hit", diag.hit_pixels, "lit", diag.lit_pixels, "occluded", diag.occluded_pixels, "mirrored hits", diag.mirrored_hits)
    assert diag.hit_pixels >= 100 and diag.lit_pixels >= 50      # (the pin is not vacuous: lights contribute to hit pixels)
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())


def test_zero_lights_is_the_diffuse_colour():
    cam = U.camera_for("box", K.tri_verts("box"))
    got, _ = S.ShadeRef(identity_ref("box")).render(cam.as_array13(), 32, 32, None)
    want, _ = K.oracle("box").render_whitted(cam.as_array13(), 32, 32, np.zeros((0, 7), np.float32))
    assert np.array_equal(got, want) and got.any()


def test_shade_signatures_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "snail_instances_shade.h")).read()
    declared = sorted(set(re.findall(r"^int (snail_instances_[a-z_0-9]+)\s*\(", hdr, flags=re.M)))
    from snail_amd._lib import INSTANCES_SHADE_SIGNATURES, INSTANCES_SIGNATURES, SIGNATURES, lib
    assert sorted(INSTANCES_SHADE_SIGNATURES) == declared and len(declared) == 3
    assert not set(INSTANCES_SHADE_SIGNATURES) & (set(SIGNATURES) | set(INSTANCES_SIGNATURES))
    assert '#include "snail_instances_shade.h"' in open(os.path.join(ROOT, "include", "snail_instances.h")).read()
    L = lib()
    for name in declared:
        assert hasattr(L, name), "libsnailhip.so does not export " + name


def test_shade_header_is_a_c_header(tmp_path):
    exe = str(tmp_path / "instances_shade_c")
    src = os.path.join(ROOT, "tests", "c", "instances_shade_c.c")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", src, "-o", exe, "-L" + LIBDIR, "-lsnailhip", "-Wl,-rpath," + LIBDIR])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "C instances shade ABI ok: 3 symbols" in r.stdout, (r.returncode, r.stdout, r.stderr)
    from snail_amd._lib import INSTANCES_SHADE_SIGNATURES
    assert set(re.findall(r"ADDR\((snail_[a-z0-9_]+)\)", open(src).read())) == set(INSTANCES_SHADE_SIGNATURES)
