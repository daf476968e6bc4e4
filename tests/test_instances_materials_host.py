"""Full shading of instanced scenes without a GPU (include/snail_instances_materials.h): the header as a C contract, what a set must refuse
before anything touches a device, the restatement (tests/instances_materials_ref.py) checked against the two restatements it must coincide
with in their common cases, and the committed cases (tests/instances_materials_cases.py) checked for what the GPU tests claim they exercise,
so that a vacuous case is caught here."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from snail_amd import _lib
from snail_amd import instances_materials as IP
from snail_amd import materials as P
from tests import dbvh_shade_ref as S
from tests import instances_materials_cases as K
from tests import instances_materials_ref as IM
from tests import materials_cases as MK
from tests import materials_ref as M
from tests import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "snail_amd")


# ---- the C-ABI ----
def test_signatures_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "snail_instances_materials.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|void|SnailInstancesMaterials \*)\s*(snail_[a-z_0-9]+)\s*\(", hdr, flags=re.M)))
    L = _lib.lib()
    assert sorted(_lib.INSTANCES_MATERIALS_SIGNATURES) == declared and len(declared) == 6, declared
    for table in (_lib.SIGNATURES, _lib.INSTANCES_SIGNATURES, _lib.INSTANCES_SHADE_SIGNATURES, _lib.INSTANCES_TILES_SIGNATURES, _lib.INSTANCES_BUILD_SIGNATURES,
                  _lib.HEATMAP_SIGNATURES, _lib.MATERIALS_SIGNATURES, _lib.MATERIALS_BOUNCE_SIGNATURES, _lib.MATERIALS_TILES_SIGNATURES,
                  _lib.MATERIALS_TRANSPARENCY_SIGNATURES, _lib.MATERIALS_TREE_SIGNATURES, _lib.MATERIALS_HEAT_SIGNATURES, _lib.MATERIALS_DYNAMIC_SIGNATURES):
        assert not set(_lib.INSTANCES_MATERIALS_SIGNATURES) & set(table)
    for name in declared:
        assert hasattr(L, name), "libsnailhip.so does not export " + name
        assert getattr(L, name).argtypes == _lib.INSTANCES_MATERIALS_SIGNATURES[name][1]
    assert not re.search(r"#include\s+<|//", hdr)      # plain C: no system header of its own, no C++ comment


def test_header_is_a_c_header(tmp_path):
    exe = str(tmp_path / "instances_materials_c")
    src = os.path.join(ROOT, "tests", "c", "instances_materials_c.c")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", src, "-o", exe, "-L" + LIBDIR, "-lsnailhip", "-Wl,-rpath," + LIBDIR])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "C instances materials ABI ok: 6 symbols" in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert set(re.findall(r"ADDR\((snail_[a-z0-9_]+)\)", open(src).read())) == set(_lib.INSTANCES_MATERIALS_SIGNATURES)


# ---- refusals that precede the handle ----
def one_record(mat_index=0):
    return P.pack_shtris(np.zeros((1, 3, 2), np.float32), np.ones((1, 3, 3), np.float32), [mat_index])


def refused(shtris_list, map_list, materials, textures, word):
    """the set is refused with a text that names the reason -- with NO instances handle: the checks come before the handle is looked at"""
    with pytest.raises(_lib.SnailError) as e:
        IP.create_instanced_set(None, shtris_list, map_list, materials, textures)
    assert word in str(e.value), str(e.value)


def test_transparent_kinds_are_refused_with_the_plain_creators_words():
    refused([one_record()], [[0]], [P.Material.transparent()], [], "transparent")
    for dissolve in (0.5, 1e-6, 0.999, float("nan")):
        refused([one_record()], [[0]], [P.Material.uber((1, 1, 1), (1, 1, 1), dissolve)], [], "dissolve")
    for dissolve in (0.0, 1.0, -1.0, 2.0):      # ... and these are stopped by the missing handle only
        refused([one_record()], [[0]], [P.Material.uber((1, 1, 1), (1, 1, 1), dissolve)], [], "invalid instances handle")
    # the same words as snail_materials_create's
    with pytest.raises(_lib.SnailError) as plain:
        P.create_set(None, one_record(), [0], [P.Material.uber((1, 1, 1), (1, 1, 1), 0.5)], [])
    with pytest.raises(_lib.SnailError) as inst:
        IP.create_instanced_set(None, [one_record()], [[0]], [P.Material.uber((1, 1, 1), (1, 1, 1), 0.5)], [])
    tail = str(plain.value).split("material 0", 1)[1]
    assert tail in str(inst.value)


def test_out_of_range_entries_and_textures_are_refused_for_any_blas():
    good = (one_record(), [-1])
    refused([good[0], one_record()], [good[1], [1]], [P.Material.simple((1, 1, 1))], [], "map entry")
    refused([one_record()], [[-2]], [], [], "map entry")
    refused([good[0], one_record(3)], [good[1], [-1]], [], [], "outside the map")
    refused([good[0], one_record(3)], [good[1], [-1]], [], [], "BLAS 1")
    refused([one_record()], [[0]], [P.Material.textured(0)], [], "texture index")

    class T:
        levels, width, height = np.zeros(64 * 48 * 3 * 2, np.uint8), 48, 64
    refused([one_record()], [[0]], [P.Material.textured(0)], [T], "powers of two")
    refused([], [], [], [], "no per-BLAS")


def test_nonzero_flags_are_refused_and_nothing_is_written():
    L = _lib.lib()
    cam, amb, img = np.zeros(13, np.float32), np.full(3, 0.1, np.float32), np.full(48, 7, np.uint8)
    for flags in (1, 2, 4, 0x100):
        assert L.snail_instances_render_materials_image(None, _lib.ptr(cam), 4, 4, None, 0, _lib.ptr(amb), flags, _lib.ptr(img), 12, None) != 0
        assert b"flags" in L.snail_last_error()
        assert L.snail_instances_render_materials_dev(None, _lib.ptr(cam), 4, 4, None, 0, _lib.ptr(amb), flags, _lib.ptr(img), 12, None, None) != 0
        assert b"flags" in L.snail_last_error()
        assert L.snail_instances_render_materials_packets_dev(None, _lib.ptr(cam), 4, 4, None, 1, None, 0, _lib.ptr(amb), flags, _lib.ptr(img), None, None) != 0
        assert b"flags" in L.snail_last_error()
    # flags 0 and a null set: refused by the handle check
    assert L.snail_instances_render_materials_image(None, _lib.ptr(cam), 4, 4, None, 0, _lib.ptr(amb), 0, _lib.ptr(img), 12, None) != 0
    assert b"invalid instanced material set handle" in L.snail_last_error()
    assert L.snail_instances_materials_shade_packets_dev(None, _lib.ptr(cam), 4, 4, None, 1, None, None, None, None, None, None, None) != 0
    assert (img == 7).all()


def test_the_python_class_refuses_a_wrong_blas_count_and_a_device_built_blas():
    class Bvh:
        perm = None

    class DevScene:
        _fast_dev, bvh, _h = True, Bvh, None

    class Isc:
        blas, _h = [DevScene()], None
    z = (np.zeros((1, 3, 2), np.float32), np.ones((1, 3, 3), np.float32), [0], None, [-1])
    with pytest.raises(_lib.SnailError, match="2 BLASes"):
        IP.InstancedMaterialSet(Isc(), [z, z])
    with pytest.raises(_lib.SnailError, match="no host permutation"):
        IP.InstancedMaterialSet(Isc(), [z])


# ---- the restatement against the restatements it must coincide with ----
def test_transform_restates_the_reference():
    """Rot per row, left to right; differences with the ROTATED nrm0; the identity's round trip is not the identity"""
    nr = np.array([[0.3, -0.7, 0.2], [1e-3, 2e-3, -3e-3], [0.11, 0.07, -0.05]], dtype=np.float32)
    rot = K.general_rotation()
    got = IM.transform(nr, rot)
    f = np.float32
    n1 = (nr[1] + nr[0]).astype(f)
    want0 = np.array([f(f(f(nr[0, 0] * rot[k, 0]) + f(nr[0, 1] * rot[k, 1])) + f(nr[0, 2] * rot[k, 2])) for k in range(3)], dtype=f)
    want1 = np.array([f(f(f(n1[0] * rot[k, 0]) + f(n1[1] * rot[k, 1])) + f(n1[2] * rot[k, 2])) for k in range(3)], dtype=f)
    assert got[0].tobytes() == want0.tobytes() and got[1].tobytes() == (want1 - want0).astype(f).tobytes()
    ident = IM.transform(nr, np.eye(3, dtype=f))
    assert ident[0].tobytes() == nr[0].tobytes() and ident[1].tobytes() != nr[1].tobytes()      # (a + b) - a != b in fp32


def test_one_identity_instance_with_flat_records_equals_the_plain_restatement():
    """records flat (the three normals equal) with no zero component: Transform leaves them bit for bit, so the samples are
    materials_ref.MaterialsRef.samples of that BLAS as a plain scene -- all three branches, every material kind"""
    tv, osc, (uv, _nrm, cls, _flat, mmap) = K.blas_data()[0]
    rng = np.random.RandomState(9)
    one = ((rng.rand(len(tv), 1, 3) + 0.2) * np.where(rng.rand(len(tv), 1, 3) < 0.5, -1.0, 1.0)).astype(np.float32)
    nrm = np.repeat(one, 3, axis=1)
    assert (nrm != 0).all()
    flat = np.ones(len(tv), dtype=bool)
    ref = K.cpu_ref([osc], np.eye(3, dtype=np.float32)[None], np.zeros((1, 3), np.float32), np.zeros(1, dtype=np.int32))
    mats, texs = MK.ref_materials(K.DESCS), K.ref_textures()
    inst = IM.InstMaterialsRef(ref, [(uv, nrm, cls, flat, mmap)], mats, texs)
    plain = M.MaterialsRef(osc, uv, nrm, cls, flat, mmap, mats, texs)
    cam = np.asarray(K.case("main")["cams"][96].as_array13(), dtype=np.float32)
    org = np.repeat(cam[:3].reshape(1, 3, 1), 4, axis=2).astype(np.float32)
    di, dp = IM.Diag(), M.Diag()
    for px, py in S.frame_packets(96, 64).tolist():
        dd, ii = O.gen_packet(cam, 96, 64, px, py, O.MODE_IEEE)
        d = dd.reshape(64, 3, 4).copy()
        dist = np.full((64, 4), np.inf, dtype=np.float32)
        obj = np.zeros((64, 4), dtype=np.int32); elem = np.zeros((64, 4), dtype=np.int32); bary = np.zeros((64, 8), dtype=np.float32)
        ref.traverse(org, d, ii.reshape(64, 3, 4).copy(), None, dist, obj, elem, bary, True, False, O.MODE_IEEE)
        a = inst.samples(d, dist, obj, elem, bary, di)
        b = plain.samples(d, dist, elem, bary, dp)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
    assert dp.blocks_a >= 1 and dp.blocks_b >= 1 and dp.blocks_c >= 1 and dp.uber_masked >= 1 and dp.uber_unmasked >= 1 and sum(dp.mips.values()) >= 100
    assert (di.blocks_a, di.blocks_b, di.blocks_c, di.mips) == (dp.blocks_a, dp.blocks_b, dp.blocks_c, dp.mips) and di.rotated_lanes == 0


@pytest.mark.parametrize("resx,resy", [(96, 64), (70, 50)])
def test_the_degenerate_set_equals_the_simple_shading_restatement(resx, resy):
    """every map entry -1 and every record flat with the triangle's plane normal: dbvh_shade_ref.ShadeRef's frame with color (1, 1, 1) and
    no reflections, byte for byte, and equal TreeStats"""
    c = K.case("degenerate")
    cam = c["cams"][resx].as_array13()
    frame, st, _smp, _xy = K.reference("degenerate").render(cam, resx, resy, c["lights"])
    want, wst = S.ShadeRef(c["ref"]).render(cam, resx, resy, c["lights"], color=(1.0, 1.0, 1.0), reflections=False)
    assert np.array_equal(frame, want) and np.array_equal(st, wst)
    assert want.any() and len(np.unique(want.reshape(-1, 3), axis=0)) > 16


# ---- the committed cases exercise what the GPU tests claim ----
@functools.lru_cache(maxsize=None)
def diag_of(name, resx, resy, transform=True):
    c = K.case(name)
    d = IM.Diag()
    frame, st, _smp, _xy = K.reference(name, transform).render(c["cams"][resx].as_array13(), resx, resy, c["lights"], diag=d)
    return frame, st, d


def test_skipping_transform_changes_the_main_frame():
    a, _, _ = diag_of("main", 96, 64)
    b, _, _ = diag_of("main", 96, 64, False)
    assert int((a != b).any(axis=2).sum()) >= 100


def test_the_main_case_exercises_every_branch():
    c = K.case("main")
    rot, _tr, bi = K.main_instances()
    assert 5 <= len(rot) <= 8 and set(bi.tolist()) == {0, 1}
    assert np.array_equal(rot[0], np.eye(3)) and (K.general_rotation() != 0).all()
    assert 200 <= len(c["oscs"][0].tris) <= 999 and len(c["oscs"][1].tris) == 12
    assert K.SHEET_MAP[5] == K.BOX_MAP[0] == 4 and K.DESCS[4][0] == "uber"          # ONE scene-wide UBER material in both maps
    assert K.TEXTURES()[1].shape[0] != K.TEXTURES()[1].shape[1]
    _, _, d = diag_of("main", 96, 64)
    assert min(d.blocks_a, d.blocks_b, d.blocks_c, d.normals_flat, d.normals_right, d.normals_left_a) >= 1, vars(d)
    assert any(mip > 0 for (_t, mip) in d.mips)
    assert d.uber_unmasked >= 1 and d.uber_masked >= 1
    assert d.cross_instance_same_tri >= 1 and d.shared_material_unmasked >= 1 and d.rotated_lanes >= 100


@pytest.mark.parametrize("resx,resy", [(96, 64), (70, 50)])
def test_the_main_cases_lights(resx, resy):
    _, _, d = diag_of("main", resx, resy)
    assert d.hit_pixels >= resx * resy // 5 and d.lit_pixels >= 100 and d.occluded_pixels >= 100
    assert d.culled and d.not_culled
    assert {n for _, n in d.culled} == {1} and any(n == 1 for _, n in d.not_culled)      # the second light: culled for some packets, not for all


def test_the_quirk_case_and_the_updated_case():
    _, _, d = diag_of("quirk", 48, 32)
    assert d.quirk_lanes >= 1
    a, _, _ = diag_of("main", 96, 64)
    b, _, du = diag_of("updated", 96, 64)
    assert int((a != b).any(axis=2).sum()) >= 500 and du.hit_pixels >= 96 * 64 // 5 and du.rotated_lanes >= 100
    m, u = K.case("main"), K.case("updated")
    assert not np.array_equal(np.sort(m["ref"].bi), np.sort(u["ref"].bi))
