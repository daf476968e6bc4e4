"""The per-frame step of a deforming instanced scene in one call (snail_instances_materials_rebuild_all_dev,
include/snail_instances_materials_rebuild_all.h; InstancedMaterialSet.rebuild_all_dev) against the calls it stands for, on a second handle
over the same data: rebuild_blas_dev, then update_dev, then the frame.  Every comparison is for equality.  The handle is the one of
tests/test_gpu_instances_materials_dynamic.py: BLASes of 257, 1 and 256 triangles that deform, beside a static box."""
import ctypes as C

import numpy as np
import pytest

from snail_amd import _lib
from snail_amd import instances_materials as IP
from tests import instances_materials_dynamic_cases as DK
from tests.test_gpu_bvh_fast_batch import rebuilds
from tests.test_gpu_instances_materials_dynamic import SIZES, check_records, dev, entries, four, records
from tests.test_gpu_instances_materials_transparency import set_arith

pytestmark = pytest.mark.gpu
F = np.float32
ARITH = ["ieee", "host_sse"]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def transforms(torch, step):
    """the four instances' transforms of a step (the translations move with it, so that the call's own transforms can be told from the old)"""
    tr = np.array([[0, 0, 0], [12, 0, 0], [0, 12, 0], [0, 0, 12]], dtype=F) + F(0.25 * step)
    xf = np.concatenate([np.tile(np.eye(3, dtype=F).reshape(1, 9), (4, 1)), tr], axis=1).astype(F)
    return dev(torch, xf), dev(torch, np.arange(4, dtype=np.int32))


def tree(isc):
    """the top-level tree as snail_instances_read_tree gives it: nodes, slot transforms, slot BLAS indices"""
    isc._dirty = True
    xs, bs = isc.slot_transforms()
    return isc.nodes().tobytes(), xs.tobytes(), bs.tobytes()


def frames(torch, isc, ms):
    """{arith: (frame, TreeStats)} from a camera that looks at the whole handle"""
    from snail_amd import survey_camera
    nd = isc.nodes()[0]
    cam = survey_camera(np.concatenate([nd["bmin"], nd["bmax"], nd["bmin"]]).reshape(1, 9))
    c, e = (nd["bmin"] + nd["bmax"]) * F(0.5), nd["bmax"] - nd["bmin"]
    lights = np.array([[c[0], c[1] + 0.6 * e[1], c[2] - 0.4 * e[2], 1.0, 0.9, 0.8, 3.0 * float(e.max())]], dtype=F)
    out = {}
    for arith in ARITH:
        set_arith(isc, arith)
        try:
            st = isc.new_stats()
            out[arith] = (ms.render(cam, 96, 64, lights, stats=st).cpu().numpy(), st.cpu().numpy())
        finally:
            set_arith(isc, "ieee")
    return out


def three_calls(torch, isc, ms, e, xf):
    info = ms.rebuild_blas_dev(e)
    perm, top = isc.update_dev(*xf)
    return info, perm, top


def compare(torch, one, three, what):
    (isc1, ms1), (isc3, ms3) = one, three
    torch.cuda.synchronize()
    assert tree(isc1) == tree(isc3), what
    assert np.array_equal(isc1.perm(), isc3.perm()), what
    for b, n in list(SIZES.items()) + [(1, isc1.blas[1].bvh.tris.shape[0])]:
        assert np.array_equal(records(ms1, b, n), records(ms3, b, n)), (what, b)
    for b in SIZES:
        s1, s3 = isc1.blas[b], isc3.blas[b]
        s1._stale = s3._stale = True
        assert s1.bvh.nodes.tobytes() == s3.bvh.nodes.tobytes() and s1.bvh.tris.tobytes() == s3.bvh.tris.tobytes() and np.array_equal(s1.perm, s3.perm), (what, b)
    f1, f3 = frames(torch, isc1, ms1), frames(torch, isc3, ms3)
    for arith in ARITH:
        assert np.array_equal(f1[arith][0], f3[arith][0]) and np.array_equal(f1[arith][1], f3[arith][1]), (what, arith, f1[arith][1], f3[arith][1])
    return f1


def test_one_call_equals_the_three_calls(torch_mod):
    torch = torch_mod
    isc1, ms1, data = four(torch)
    isc3, ms3, _ = four(torch)
    f0 = frames(torch, isc1, ms1)
    xf = transforms(torch, 1)
    count0 = {b: rebuilds(isc1.blas[b]) for b in SIZES}
    binfo, perm, top = ms1.rebuild_all_dev(entries(data, 1, [0, 2, 3]), *xf)
    info3, perm3, top3 = three_calls(torch, isc3, ms3, entries(data, 1, [0, 2, 3]), xf)
    torch.cuda.synchronize()
    assert binfo.cpu().numpy().tolist() == info3.cpu().numpy().tolist() and binfo.cpu().numpy()[:, 0].tolist() == [0, 0, 0]
    assert top.cpu().numpy().tolist() == top3.cpu().numpy().tolist() and top.cpu().numpy()[0] == 0 and top.cpu().numpy()[3] == 4
    assert np.array_equal(perm.cpu().numpy(), perm3.cpu().numpy())
    assert {b: rebuilds(isc1.blas[b]) for b in SIZES} == {b: c + 1 for b, c in count0.items()}
    check_records(isc1, ms1, data, {0: 1, 2: 1, 3: 1}, "after rebuild_all_dev")
    f1 = compare(torch, (isc1, ms1), (isc3, ms3), "all three BLASes")
    assert (f1["ieee"][0] != f0["ieee"][0]).any() and len(np.unique(f1["ieee"][0].reshape(-1, 3), axis=0)) > 8       # the step shows, and the frame is not empty
    # a second step over a part of the list, in another order, and on a stream of its own
    xf2 = transforms(torch, 2)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    e = entries(data, 2, [3])
    e.update(entries(data, 2, [0]))
    ms1.rebuild_all_dev(e, *xf2, stream=s)
    three_calls(torch, isc3, ms3, e, xf2)
    check_records(isc1, ms1, data, {0: 2, 2: 1, 3: 2}, "after the second rebuild_all_dev")
    compare(torch, (isc1, ms1), (isc3, ms3), "two of three BLASes")
    for m, i in ((ms1, isc1), (ms3, isc3)):
        m.close(); i.close()


def test_a_refused_build_keeps_its_box_in_the_new_top_level_tree(torch_mod):
    """the middle entry has a NaN vertex: status 1, the BLAS keeps tree, perm and records, the others commit, and the top-level tree is built
    over the refused BLAS's OLD root box -- all as the three calls leave it"""
    torch = torch_mod
    isc1, ms1, data = four(torch)
    isc3, ms3, _ = four(torch)
    bad = data[3]["tv"][1].copy()
    bad[100, 1, 2] = np.nan
    e = entries(data, 1, [0])
    e[3] = (dev(torch, bad), None)
    e[2] = entries(data, 1, [2])[2]
    xf = transforms(torch, 1)
    old_root = isc1.blas[3].bvh.nodes[0].copy()
    before = (records(ms1, 3, 256), isc1.blas[3].d_perm.cpu().numpy().copy())
    binfo, perm, top = ms1.rebuild_all_dev(e, *xf)
    three_calls(torch, isc3, ms3, e, xf)
    torch.cuda.synchronize()
    b = binfo.cpu().numpy()
    assert b[1].tolist() == [1, 0, 0, 256, 0, 0] and b[0][0] == 0 and b[2][0] == 0 and b[0][4] == 1 and b[2][4] == 1, b.tolist()
    assert top.cpu().numpy()[0] == 0
    assert np.array_equal(records(ms1, 3, 256), before[0]) and np.array_equal(isc1.blas[3].d_perm.cpu().numpy(), before[1])
    check_records(isc1, ms1, data, {0: 1, 2: 1, 3: 0}, "after the partly refused rebuild_all_dev")
    compare(torch, (isc1, ms1), (isc3, ms3), "one build refused")
    # the refused BLAS's instance sits in the new tree with its old box: identity rotation, so the leaf box is the root box moved by the translation
    isc1.blas[3]._stale = True
    root = isc1.blas[3].bvh.nodes[0]
    assert root.tobytes() == old_root.tobytes()
    xs, bs = isc1.slot_transforms()
    slot = int(np.argwhere(bs == 3).ravel()[0])
    nodes = isc1.nodes()
    leaf = nodes[nodes["sub"] == np.uint32(0x80000000 | slot)]
    t = xs[slot][9:12]
    assert len(leaf) == 1
    assert np.allclose(leaf[0]["bmin"], old_root["bmin"] + t, rtol=0, atol=1e-3) and np.allclose(leaf[0]["bmax"], old_root["bmax"] + t, rtol=0, atol=1e-3)
    tv_new = data[3]["tv"][1].reshape(-1, 3)          # (the box the refused vertices would have had is another one)
    assert not np.allclose(leaf[0]["bmin"], tv_new.min(axis=0) + t, rtol=0, atol=1e-3) or not np.allclose(leaf[0]["bmax"], tv_new.max(axis=0) + t, rtol=0, atol=1e-3)
    for m, i in ((ms1, isc1), (ms3, isc3)):
        m.close(); i.close()


def test_the_union_of_refusals_enqueues_nothing(torch_mod):
    torch = torch_mod
    L = _lib.lib()
    isc, ms, data = four(torch)
    xf = transforms(torch, 0)
    ms.rebuild_all_dev(entries(data, 0, [0, 2, 3]), *xf)        # (the one-off host wait of the first update_dev, and a tree read back from the device)
    torch.cuda.synchronize()
    tree0 = tree(isc)
    count0 = {b: rebuilds(isc.blas[b]) for b in SIZES}
    states0 = {b: isc.blas[b].d_perm.cpu().numpy().copy() for b in SIZES}
    xf1 = transforms(torch, 1)
    topinfo = torch.full((4,), 7, dtype=torch.int32, device="cuda:0")
    topperm = torch.full((4,), 7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()

    def call(set_handle, arr, n_list, d_xf, n):
        return L.snail_instances_materials_rebuild_all_dev(set_handle, C.cast(arr, C.c_void_p) if arr is not None else None, n_list, d_xf, xf1[1].data_ptr(), n,
                                                           topperm.data_ptr(), topinfo.data_ptr(), None)

    def listed(blases):
        arr = (IP._BlasRebuild * len(blases))()
        for k, b in enumerate(blases):
            arr[k].blas, arr[k].d_verts9, arr[k].d_perm = b, data[b if b in data else 0]["dtv"][1].data_ptr(), None
        return arr

    good = listed([0, 2, 3])
    nov = listed([0, 2, 3])
    nov[1].d_verts9 = None
    static = IP.InstancedMaterialSet(*static_twin(isc))
    fn = "snail_instances_materials_rebuild_all_dev: "
    cases = [
        # snail_instances_materials_rebuild_dev's
        ("no list", lambda: call(ms._h, None, 3, xf1[0].data_ptr(), 4), fn + "no BLAS listed"),
        ("nList 0", lambda: call(ms._h, good, 0, xf1[0].data_ptr(), 4), fn + "no BLAS listed"),
        ("out of range", lambda: call(ms._h, listed([0, 4]), 2, xf1[0].data_ptr(), 4), "BLAS index 4 is out of range (the handle has 4)"),
        ("never rebuilt", lambda: call(ms._h, listed([0, 1]), 2, xf1[0].data_ptr(), 4), "BLAS 1 is never rebuilt"),
        ("twice", lambda: call(ms._h, listed([0, 3, 0]), 3, xf1[0].data_ptr(), 4), "BLAS 0 is listed twice"),
        ("null vertices", lambda: call(ms._h, nov, 3, xf1[0].data_ptr(), 4), "entry 1 (BLAS 2): null vertices"),
        ("null set", lambda: call(None, good, 3, xf1[0].data_ptr(), 4), fn + "invalid instanced material set handle"),
        ("a set of another kind", lambda: call(static._h, good, 3, xf1[0].data_ptr(), 4), "not made by snail_instances_materials_create_dev"),
        # snail_instances_rebuild_dev's
        ("n 0", lambda: call(ms._h, good, 3, xf1[0].data_ptr(), 0), fn + "0 instances"),
        ("n too large", lambda: call(ms._h, good, 3, xf1[0].data_ptr(), (1 << 30) + 1), fn + "1073741825 instances"),
        ("null transforms", lambda: call(ms._h, good, 3, None, 4), fn + "null transforms"),
    ]
    for what, run, text in cases:
        rc = run()
        err = L.snail_last_error().decode()
        assert rc != 0 and text in err, (what, rc, err)
    # a stale set: a BLAS rebuilt behind its back (this rebuild is counted below)
    isc.blas[2].rebuild_fast_dev(data[2]["dtv"][0])
    count0[2] += 1
    assert call(ms._h, good, 3, xf1[0].data_ptr(), 4) != 0 and "rebuilt" in L.snail_last_error().decode() and "BLAS 2" in L.snail_last_error().decode()
    with pytest.raises(_lib.SnailError, match="rebuilt"):
        ms.rebuild_all_dev(entries(data, 1, [0, 2, 3]), *xf1)
    torch.cuda.synchronize()
    assert {b: rebuilds(isc.blas[b]) for b in SIZES} == count0
    assert tree(isc) == tree0
    assert topinfo.cpu().numpy().tolist() == [7] * 4 and topperm.cpu().numpy().tolist() == [7] * 4
    for b in SIZES:
        assert np.array_equal(isc.blas[b].d_perm.cpu().numpy(), states0[b])
    # healed, the call is taken
    ms.update_blas_dev({2: (None, data[2]["dtv"][0])})
    assert call(ms._h, good, 3, xf1[0].data_ptr(), 4) == 0, L.snail_last_error()
    torch.cuda.synchronize()
    assert topinfo.cpu().numpy().tolist()[0::3] == [0, 4] and tree(isc) != tree0
    static.close(); ms.close(); isc.close()


def static_twin(isc):
    """the arguments of an InstancedMaterialSet of the constructor's kind (no device rebuild) over a handle of host-built boxes"""
    from snail_amd.instances import InstancedScene
    from snail_amd.scene import Scene
    p = DK.poses()
    box = Scene.from_fast(p["box"][0], 0)
    tw = InstancedScene([box], np.eye(3, dtype=F)[None], np.zeros((1, 3), dtype=F), np.zeros(1, dtype=np.int32))
    return tw, [(p["box"][1][0], p["box"][1][1], p["box"][1][2], p["box"][1][3], [-1] * 3)]
