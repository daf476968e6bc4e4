"""Full shading of instanced scenes whose BLASes deform on the device, on the MI355X (include/snail_instances_materials_dynamic.h;
InstancedMaterialSet.from_dev / .rebuild_blas_dev / .update_blas_dev).  Every comparison is for equality against code that is pinned already:
the records against snail_shtris_pack on the host over the downloaded perm, frames and TreeStats against a STATIC TWIN -- an InstancedScene
over Scene.from_fast BLASes plus the existing InstancedMaterialSet, over the same vertices, shading data and transforms (the device's fast
tree and the device's top-level tree are byte-equal to the host's, so object and triId mean the same thing in both).  The scene is
tests/instances_materials_dynamic_cases.py's: the main case of the instanced full-shading tests whose sheet BLAS deforms between poses A, B."""
import ctypes as C

import numpy as np
import pytest

from snail_amd import _lib
from snail_amd import instances_materials as IP
from snail_amd import materials as P
from snail_amd.instances import InstancedScene
from snail_amd.scene import Scene
from tests import instances_materials_cases as IK
from tests import instances_materials_dynamic_cases as DK
from tests import shtris_dev_ref as R
from tests.test_gpu_instances_materials_transparency import product_materials, set_arith

pytestmark = pytest.mark.gpu
ARITH = ["ieee", "host_sse"]
FRAMES = [(96, 64), (70, 50)]       # 24 and 20 packets, the second with partial packets
F = np.float32
TINT = (0.9, 1.0, 0.6)
SHEET, BOX = DK.SHEET, DK.BOX


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")      # (a copy: the cached host arrays are read-only)


def records(ms, b, n):
    """the records the set holds now for BLAS b (the workbench library's read-back: test-only, in no header)"""
    fn = _lib.debug_lib().snail_instances_materials_debug_records
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    out = np.zeros((n, 64), dtype=np.uint8)
    assert fn(ms._h, b, _lib.ptr(out), n) == 0, _lib.debug_lib().snail_last_error()
    return out


def materials(transparent):
    """the main case's list; the transparent set has UBER with dissolve 0.5 and the transparent kind instead of the two opaque UBERs"""
    descs = list(IK.DESCS)
    if transparent:
        descs[3], descs[4] = ("uber", (0.9, 0.4, 0.1), (0.2, 0.6, 1.0), 0.5), ("transp", 0, 1, True)
    return product_materials(descs, IK.TEXTURES())


def xf12():
    p = DK.poses()
    return np.ascontiguousarray(np.concatenate([np.asarray(p["rot"], dtype=F).reshape(-1, 9), np.asarray(p["tr"], dtype=F).reshape(-1, 3)], axis=1), dtype=F)


# ---- the static twin: built once per (pose, kind of set), never changed ----
_twins = {}


def twin(pose, perm_of=None):
    """(InstancedScene over Scene.from_fast BLASes, its InstancedMaterialSet, its transparent InstancedMaterialSet) of a pose.  perm_of =
    another pose: the WRONG sets on purpose, the pose's tree with the records permuted by the other pose's tree -- what stale records would be"""
    key = (pose, perm_of)
    if key not in _twins:
        p = DK.poses()
        sheet = Scene.from_fast(p[pose][0], 0)
        box = Scene.from_fast(p["box"][0], 0)
        isc = InstancedScene([sheet, box], p["rot"], p["tr"], p["bi"])
        sets = []
        for transparent in (False, True):
            mats, texs = materials(transparent)
            if perm_of is None:
                sets.append(IP.InstancedMaterialSet(isc, [DK.sheet_data(pose), p["box"][1]], mats, texs, transparent=transparent))
                continue
            uv, nrm, mi, flat, mmap = DK.sheet_data(pose)
            buv, bnrm, bmi, bflat, bmap = p["box"][1]
            sh = [P.pack_shtris(uv, nrm, mi, flat, DK.fast_trees()[perm_of].perm), P.pack_shtris(buv, bnrm, bmi, bflat, box.bvh.perm)]
            ms = IP.InstancedMaterialSet.__new__(IP.InstancedMaterialSet)
            ms.isc, ms.shtris = isc, sh
            ms._h = IP.create_instanced_set(isc._h, sh, [mmap, bmap], mats, texs, transparent)
            sets.append(ms)
        _twins[key] = (isc, sets[0], sets[1])
    return _twins[key]


def dynamic(torch, transparent=False, pose="A", face=False):
    """a fresh (InstancedScene with the sheet from Scene.from_fast_dev, InstancedMaterialSet.from_dev, the poses' device tensors)"""
    p = DK.poses()
    d = {k: (dev(torch, p[k][0]), dev(torch, p[k][1])) for k in "AB"}
    sheet = Scene.from_fast_dev(d[pose][0], 0)
    box = Scene.from_fast(p["box"][0], 0)
    isc = InstancedScene([sheet, box], p["rot"], p["tr"], p["bi"])
    mats, texs = materials(transparent)
    sh = IP.DevBlasShading(dev(torch, p["uv"]), dev(torch, p["mat_index"]), dev(torch, p["flat"]), p["material_map"], d_nrm=None if face else d[pose][1],
                           d_verts=d[pose][0])
    ms = IP.InstancedMaterialSet.from_dev(isc, [sh, p["box"][1]], mats, texs, transparent=transparent)
    return isc, ms, d


def to_pose(torch, isc, ms, d, pose, stream=None):
    """the per-frame sequence: the BLAS and its records, then the top-level tree"""
    info = ms.rebuild_blas_dev({SHEET: d[pose]}, stream=stream)
    p = DK.poses()
    keep = (dev(torch, xf12()), dev(torch, np.asarray(p["bi"], dtype=np.int32)))
    isc.update_dev(keep[0], keep[1], stream=stream)
    isc._keep = keep        # (read on the stream: alive until the scene goes)
    return info


def packet_list(torch, resx, resy):
    pw, ph = (resx + 15) // 16, (resy + 15) // 16
    return dev(torch, np.array([[x * 16, y * 16] for y in range(ph) for x in range(pw)], dtype=np.int32))


def frames_of(torch, isc, ms, tms, resx, resy, arith):
    """{what: (bytes, TreeStats [+ truncated])} of the five entry families on an opaque set ms and a transparent set tms of one scene"""
    p = DK.poses()
    cam, lights = p["cams"][resx], p["lights"]
    xy = packet_list(torch, resx, resy)
    out = {}
    set_arith(isc, arith)
    try:
        st = isc.new_stats()
        out["render"] = (ms.render(cam, resx, resy, lights, stats=st).cpu().numpy(), st.cpu().numpy())
        st = isc.new_stats()
        out["reflections"] = (ms.render(cam, resx, resy, lights, stats=st, reflections=True).cpu().numpy(), st.cpu().numpy())
        st = isc.new_stats()
        fr, trunc = tms.render_transparent(cam, resx, resy, lights, stats=st, max_depth=3)
        out["render_transparent"] = (fr.cpu().numpy(), np.concatenate([st.cpu().numpy(), trunc.cpu().numpy()]))
        st = isc.new_stats()
        fr, trunc = tms.tree_frame_packets(cam, resx, resy, xy, lights, flags=P.RENDER_AA4, tint=TINT, stats=st)
        out["tree_frame_packets"] = (fr.cpu().numpy(), np.concatenate([st.cpu().numpy(), trunc.cpu().numpy()]))
        st = isc.new_stats()
        ps, trunc = tms.packet_stats(cam, resx, resy, xy, lights, reflections=True, stats=st)
        out["packet_stats"] = (ps.cpu().numpy(), np.concatenate([st.cpu().numpy(), trunc.cpu().numpy()]))
    finally:
        set_arith(isc, "ieee")
    return out


def same(what, got, want):
    bad = int((got[0] != want[0]).sum())
    print("%s: %d differing values of %d; stats %s / %s" % (what, bad, want[0].size, got[1].tolist(), want[1].tolist()))
    assert got[0].shape == want[0].shape and bad == 0, (what, bad)
    assert np.array_equal(got[1], want[1]), (what, got[1], want[1])


def differ(a, b):
    return a[0].shape != b[0].shape or bool((a[0] != b[0]).any())


# ---- 1. and 2.: the records, and the commit rule per entry ----
SIZES = {0: 257, 2: 1, 3: 256}       # an entry boundary inside, at the end of and right after a 256-thread workgroup; BLAS 2 is a root leaf


def four(torch):
    """a handle of four BLASes (dynamic 257 triangles, the static box, dynamic 1, dynamic 256) over random finite data, one instance each"""
    rng = np.random.RandomState(911)
    p = DK.poses()
    data = {}
    for b, n in SIZES.items():
        data[b] = dict(tv=[(rng.rand(n, 3, 3) * 4.0 - 2.0 + rng.rand(n, 1, 3) * 6.0).astype(F) for _ in range(3)], uv=(rng.rand(n, 3, 2) * 6.0 - 3.0).astype(F),
                       nrm=[(rng.rand(n, 3, 3) * 2.0 - 1.0).astype(F) for _ in range(3)], mi=rng.randint(0, 7, size=n).astype(np.int32),
                       flat=(rng.rand(n) < 0.4).astype(np.uint8), given=(b == 0))
        data[b]["dtv"] = [dev(torch, t) for t in data[b]["tv"]]
        data[b]["dnrm"] = [dev(torch, t) for t in data[b]["nrm"]]
    scs = [Scene.from_fast_dev(data[0]["dtv"][0], 0), Scene.from_fast(p["box"][0], 0), Scene.from_fast_dev(data[2]["dtv"][0], 0), Scene.from_fast_dev(data[3]["dtv"][0], 0)]
    tr = np.array([[0, 0, 0], [12, 0, 0], [0, 12, 0], [0, 0, 12]], dtype=F)
    isc = InstancedScene(scs, np.stack([np.eye(3, dtype=F)] * 4), tr, np.arange(4, dtype=np.int32))
    per = [None, (p["box"][1][0], p["box"][1][1], p["box"][1][2], p["box"][1][3], [-1] * 3), None, None]
    for b in SIZES:
        D = data[b]
        per[b] = IP.DevBlasShading(dev(torch, D["uv"]), dev(torch, D["mi"]), dev(torch, D["flat"]), [-1] * 7, d_nrm=D["dnrm"][0] if D["given"] else None, d_verts=D["dtv"][0])
    ms = IP.InstancedMaterialSet.from_dev(isc, per)
    return isc, ms, data


def want_records(D, step, perm):
    return P.pack_shtris(D["uv"], D["nrm"][step] if D["given"] else R.vertex_normals_from_faces(D["tv"][step]), D["mi"], D["flat"], perm)


def check_records(isc, ms, data, steps, what):
    for b, n in SIZES.items():
        perm = isc.blas[b].d_perm.cpu().numpy()
        assert sorted(perm.tolist()) == list(range(n))
        got, want = records(ms, b, n), want_records(data[b], steps[b], perm)
        bad = np.argwhere((got != want).any(axis=1)).ravel()
        print("%s: BLAS %d (%d triangles, pose %d): %d differing records" % (what, b, n, steps[b], len(bad)))
        assert len(bad) == 0, (what, b, bad[:5].tolist(), got[bad[0]].view(np.uint32).tolist(), want[bad[0]].view(np.uint32).tolist())


def entries(data, step, blases):
    return {b: (data[b]["dtv"][step], data[b]["dnrm"][step] if data[b]["given"] else None) for b in blases}


def test_records_equal_the_host_pack(torch_mod):
    """at creation, after one batched rebuild of all three dynamic BLASes (an entry with given normals and entries with face normals in one
    call) and after a rebuild of {3} alone; the static BLAS's records are the constructor's, untouched"""
    torch = torch_mod
    isc, ms, data = four(torch)
    box = DK.poses()["box"][1]
    box_want = P.pack_shtris(box[0], box[1], box[2], box[3], isc.blas[1].bvh.perm)
    steps = {0: 0, 2: 0, 3: 0}
    check_records(isc, ms, data, steps, "creation")
    assert np.array_equal(records(ms, 1, len(box_want)), box_want)
    info = ms.rebuild_blas_dev(entries(data, 1, [0, 2, 3])).cpu().numpy()
    assert info[:, 0].tolist() == [0, 0, 0] and info[:, 3].tolist() == [257, 1, 256] and info[:, 4:].tolist() == [[1, 0]] * 3, info
    steps = {0: 1, 2: 1, 3: 1}
    check_records(isc, ms, data, steps, "after the batched rebuild")
    for b in SIZES:
        assert np.array_equal(isc.blas[b].d_perm.cpu().numpy(), isc.blas[b].perm)       # the scene's read-back tree is the one the perm belongs to
    info = ms.rebuild_blas_dev(entries(data, 2, [3])).cpu().numpy()
    assert info.tolist()[0][0::3] == [0, 256] and info.tolist()[0][4:] == [1, 0]
    steps[3] = 2
    check_records(isc, ms, data, steps, "after the rebuild of BLAS 3 alone")
    assert np.array_equal(records(ms, 1, len(box_want)), box_want)
    # an update with new normals alone, batched over two BLASes: the perm stays, the records follow the normals
    data[0]["nrm"][1] = data[0]["nrm"][2]
    info = ms.update_blas_dev({0: (data[0]["dnrm"][2], None), 2: (None, data[2]["dtv"][1])}).cpu().numpy()
    assert info.tolist() == [[1, 0], [1, 0]]
    check_records(isc, ms, data, steps, "after update_blas_dev")
    ms.close(); isc.close()


def test_the_commit_rule_is_per_entry(torch_mod):
    """the middle entry of a three-entry rebuild has a non-finite vertex: it keeps tree, perm and records, the other two commit"""
    torch = torch_mod
    isc, ms, data = four(torch)
    before = {b: (records(ms, b, n), isc.blas[b].d_perm.cpu().numpy()) for b, n in SIZES.items()}
    bad = data[3]["tv"][1].copy()
    bad[100, 1, 2] = np.nan
    e = entries(data, 1, [0])
    e[3] = (dev(torch, bad), None)
    e[2] = entries(data, 1, [2])[2]
    assert list(e) == [0, 3, 2]
    info = ms.rebuild_blas_dev(e).cpu().numpy()
    print(info.tolist())
    assert info[1].tolist() == [1, 0, 0, 256, 0, 0], info[1]
    assert info[0][0] == 0 and info[0][3:].tolist() == [257, 1, 0] and info[2][0] == 0 and info[2][3:].tolist() == [1, 1, 0]
    assert np.array_equal(records(ms, 3, 256), before[3][0]) and np.array_equal(isc.blas[3].d_perm.cpu().numpy(), before[3][1])
    check_records(isc, ms, data, {0: 1, 2: 1, 3: 0}, "after the partly refused rebuild")
    assert not np.array_equal(records(ms, 0, 257), before[0][0])
    # the set is still accepted by a frame function (after the top-level tree has followed the two new root boxes)
    xf = np.concatenate([np.tile(np.eye(3, dtype=F).reshape(1, 9), (4, 1)), np.array([[0, 0, 0], [12, 0, 0], [0, 12, 0], [0, 0, 12]], dtype=F)], axis=1)
    dxf, dbi = dev(torch, xf), dev(torch, np.arange(4, dtype=np.int32))
    isc.update_dev(dxf, dbi)
    cam = DK.poses()["cams"][96]
    fr = ms.render(cam, 96, 64, DK.poses()["lights"])
    torch.cuda.synchronize()
    assert fr.shape == (64, 96, 3)
    ms.close(); isc.close()


# ---- 3. frames: pose A, rebuild to B, back to A, through five entry families ----
def test_the_twin_alone_tells_the_poses_and_stale_records_apart(torch_mod):
    """before the dynamic path is looked at: the twin's 96 x 64 frames of A and B differ, and a twin made from pose B's tree with pose A's
    perm differs from the correct one -- without this the frame tests could pass with stale records"""
    torch = torch_mod
    DK.check_poses()
    A = frames_of(torch, *twin("A"), 96, 64, "ieee")
    B = frames_of(torch, *twin("B"), 96, 64, "ieee")
    for k in A:
        assert differ(A[k], B[k]), k
    assert len(np.unique(A["render"][0].reshape(-1, 3), axis=0)) > 16
    S = frames_of(torch, *twin("B", perm_of="A"), 96, 64, "ieee")
    for k in ("render", "reflections", "render_transparent", "tree_frame_packets"):
        assert differ(S[k], B[k]), k


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("resx,resy", FRAMES)
def test_frames_follow_the_rebuild(torch_mod, resx, resy, arith):
    torch = torch_mod
    isc, ms, d = dynamic(torch)
    p = DK.poses()
    mats, texs = materials(True)
    sh = IP.DevBlasShading(dev(torch, p["uv"]), dev(torch, p["mat_index"]), dev(torch, p["flat"]), p["material_map"], d_nrm=d["A"][1])
    tms = IP.InstancedMaterialSet.from_dev(isc, [sh, p["box"][1]], mats, texs, transparent=True)
    assert tms.can_select_transparent and not ms.can_select_transparent
    want = {k: frames_of(torch, *twin(k), resx, resy, arith) for k in "AB"}
    for pose in "ABA":
        if pose != "A" or isc._dirty:
            info = to_pose(torch, isc, ms, d, pose).cpu().numpy()
            assert info.tolist()[0][0::3] == [0, len(p["uv"])] and info.tolist()[0][4:] == [1, 0]
            with pytest.raises(_lib.SnailError, match="rebuilt"):          # the second set of the same handle is the earlier tree's
                tms.render_transparent(p["cams"][resx], resx, resy, p["lights"])
            assert tms.update_blas_dev({SHEET: (d[pose][1], None)}).cpu().numpy().tolist() == [[1, 0]]
        got = frames_of(torch, isc, ms, tms, resx, resy, arith)
        for k in got:
            same("%s, pose %s, %dx%d, %s" % (k, pose, resx, resy, arith), got[k], want[pose][k])
    tw = twin("A")[0]
    assert isc.nodes().tobytes() == tw.nodes().tobytes() and np.array_equal(isc.blas[SHEET].perm, tw.blas[SHEET].perm)
    tms.close(); ms.close(); isc.close()


def test_face_normals_and_the_transparent_set_through_one_rebuild(torch_mod):
    """d_nrm = None: the face normals of the new vertices, as the twin gets them from the restatement"""
    torch = torch_mod
    p = DK.poses()
    isc, ms, d = dynamic(torch, face=True)
    to_pose(torch, isc, ms, {"B": (d["B"][0], None)}, "B")
    sheet = Scene.from_fast(p["B"][0], 0)
    box = Scene.from_fast(p["box"][0], 0)
    tisc = InstancedScene([sheet, box], p["rot"], p["tr"], p["bi"])
    tms = IP.InstancedMaterialSet(tisc, [DK.sheet_data("B", R.vertex_normals_from_faces(p["B"][0])), p["box"][1]], *materials(False))
    cam = p["cams"][96]
    got, want = [], []
    for i, m, o in ((isc, ms, got), (tisc, tms, want)):
        st = i.new_stats()
        o += [m.render(cam, 96, 64, p["lights"], stats=st).cpu().numpy(), st.cpu().numpy()]
    same("face normals after a rebuild", got, want)
    assert differ(want, frames_of(torch, *twin("B"), 96, 64, "ieee")["render"])
    tms.close(); tisc.close(); ms.close(); isc.close()


# ---- 4. staleness ----
def set_methods(torch, resx=96, resy=64):
    """every method of InstancedMaterialSet that takes the set to the library, as (name, call)"""
    p = DK.poses()
    cam, lights = p["cams"][resx], p["lights"]
    xy = packet_list(torch, resx, resy)
    n = int(xy.shape[0])
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda:0")      # noqa: E731
    hits = (z(n, 256), z(n, 256), z(n, 256), z(n, 256, dt=torch.int32), z(n, 256, dt=torch.int32))
    rays = z(n, 64, 3, 4) + 1.0
    samples = z(n, 9, 64, 4)
    tiles = np.array([[0, 0, 32, 32]], dtype=np.int32)
    return [
        ("shade_packets", lambda m: m.shade_packets(cam, resx, resy, xy, hits)),
        ("mirror_packets", lambda m: m.mirror_packets(cam, resx, resy, xy, hits[0], samples)),
        ("shade_rays", lambda m: m.shade_rays(rays, None, hits[0], z(n, 64, 2, 4), hits[3], hits[4])),
        ("render", lambda m: m.render(cam, resx, resy, lights)),
        ("render reflections", lambda m: m.render(cam, resx, resy, lights, reflections=True)),
        ("render_packets", lambda m: m.render_packets(cam, resx, resy, xy, lights)),
        ("render_packets reflections", lambda m: m.render_packets(cam, resx, resy, xy, lights, reflections=True)),
        ("render_image_host", lambda m: m.render_image_host(cam, resx, resy, lights)),
        ("render_image_host reflections", lambda m: m.render_image_host(cam, resx, resy, lights, reflections=True)),
        ("can_select_transparent", lambda m: m.can_select_transparent),
        ("shade_packets_transp", lambda m: m.shade_packets_transp(cam, resx, resy, xy, hits)),
        ("shade_rays_transp", lambda m: m.shade_rays_transp(rays, None, hits[0], z(n, 64, 2, 4), hits[3], hits[4])),
        ("continue_packets", lambda m: m.continue_packets(hits[0], z(n, 64, dt=torch.uint8), cam, resx, resy, xy)),
        ("render_transparent", lambda m: m.render_transparent(cam, resx, resy, lights)),
        ("render_transparent_packets", lambda m: m.render_transparent_packets(cam, resx, resy, xy, lights)),
        ("render_transparent_image_host", lambda m: m.render_transparent_image_host(cam, resx, resy, lights)),
        ("mirror_rays", lambda m: m.mirror_rays(rays, rays, None, hits[0], samples)),
        ("tree_frame_packets", lambda m: m.tree_frame_packets(cam, resx, resy, xy, lights)),
        ("render_tree_tiles_host", lambda m: m.render_tree_tiles_host(cam, resx, resy, tiles, lights7=lights)),
        ("render_tree_frame_host", lambda m: m.render_tree_frame_host(cam, resx, resy, lights)),
        ("set_level_budget", lambda m: m.set_level_budget(1 << 26)),
        ("packet_stats", lambda m: m.packet_stats(cam, resx, resy, xy, lights)),
        ("render_heat_packets", lambda m: m.render_heat_packets(cam, resx, resy, xy, lights)),
        ("render_heat_tiles_host", lambda m: m.render_heat_tiles_host(cam, resx, resy, tiles, lights7=lights)),
        ("render_heat_frame_host", lambda m: m.render_heat_frame_host(cam, resx, resy, lights)),
        ("rebuild_blas_dev", None),
    ]


@pytest.fixture(scope="module")
def stale_set(torch_mod):
    """a set made stale by Scene.rebuild_fast_dev behind its back (to the same pose: its records would in fact still fit), for the whole list"""
    torch = torch_mod
    isc, ms, d = dynamic(torch)
    isc.blas[SHEET].rebuild_fast_dev(d["A"][0])
    yield isc, ms, d
    ms.close(); isc.close()


NAMES = ["shade_packets", "mirror_packets", "shade_rays", "render", "render reflections", "render_packets", "render_packets reflections", "render_image_host",
         "render_image_host reflections", "can_select_transparent", "shade_packets_transp", "shade_rays_transp", "continue_packets", "render_transparent",
         "render_transparent_packets", "render_transparent_image_host", "mirror_rays", "tree_frame_packets", "render_tree_tiles_host", "render_tree_frame_host",
         "set_level_budget", "packet_stats", "render_heat_packets", "render_heat_tiles_host", "render_heat_frame_host", "rebuild_blas_dev"]


@pytest.mark.parametrize("name", NAMES)
def test_every_method_refuses_a_stale_set(torch_mod, stale_set, name):
    torch = torch_mod
    isc, ms, d = stale_set
    table = dict(set_methods(torch))
    assert list(table) == NAMES
    # the list is the class's: every public method that reaches the library with the set, but the two that heal or end it
    public = {k for k, v in vars(IP.InstancedMaterialSet).items() if not k.startswith("_") and k not in ("from_dev", "close", "level_bytes", "update_blas_dev")}
    assert public == {k.split(" ")[0] for k in NAMES}, public ^ {k.split(" ")[0] for k in NAMES}
    call = table[name] or (lambda m: m.rebuild_blas_dev({SHEET: d["B"]}))
    with pytest.raises(_lib.SnailError, match="rebuilt") as e:
        call(ms)
    assert "snail_instances_materials_update_dev" in str(e.value) and "BLAS 0" in str(e.value)


def test_update_heals_and_owners_of_one_blas_scene_make_each_other_stale(torch_mod):
    torch = torch_mod
    p = DK.poses()
    resx, resy = 96, 64
    cam = p["cams"][resx]
    isc, ms, d = dynamic(torch)
    sheet = isc.blas[SHEET]
    mmap, mats, texs = p["material_map"], *materials(False)
    plain = P.MaterialSet.from_dev(sheet, dev(torch, p["uv"]), dev(torch, p["mat_index"]), dev(torch, p["flat"]), mmap, mats, texs, d_nrm=d["A"][1])
    wantB = frames_of(torch, *twin("B"), resx, resy, "ieee")["render"]
    wantA = frames_of(torch, *twin("A"), resx, resy, "ieee")["render"]
    xf = (dev(torch, xf12()), dev(torch, np.asarray(p["bi"], dtype=np.int32)))

    def frame():
        st = isc.new_stats()
        return ms.render(cam, resx, resy, p["lights"], stats=st).cpu().numpy(), st.cpu().numpy()

    # behind the set's back, then healed by an update with the current perm
    sheet.rebuild_fast_dev(d["B"][0])
    isc.update_dev(*xf)
    with pytest.raises(_lib.SnailError, match="rebuilt"):
        frame()
    info = ms.update_blas_dev({SHEET: (d["B"][1], None)})
    same("after update_blas_dev", frame(), wantB)
    assert info.cpu().numpy().tolist() == [[1, 0]]
    # the plain set of the same BLAS scene was left behind by that rebuild too; its own rebuild leaves the instanced set behind
    with pytest.raises(_lib.SnailError, match="rebuilt"):
        plain.render(cam, resx, resy, p["lights"])
    plain.update_dev(d_nrm=d["B"][1])
    plain.rebuild_dev(d["A"][0], d["A"][1])
    with pytest.raises(_lib.SnailError, match="rebuilt"):
        frame()
    ms.update_blas_dev({SHEET: (d["A"][1], None)})
    isc.update_dev(*xf)
    same("after the plain set's rebuild and an update", frame(), wantA)
    # and the instanced set's rebuild leaves the plain set behind
    to_pose(torch, isc, ms, d, "B")
    with pytest.raises(_lib.SnailError, match="rebuilt"):
        plain.render(cam, resx, resy, p["lights"])
    same("the instanced set after its own rebuild", frame(), wantB)
    # a second instanced handle over the same BLAS scenes
    isc2 = InstancedScene(isc.blas, p["rot"], p["tr"], p["bi"])
    sh = IP.DevBlasShading(dev(torch, p["uv"]), dev(torch, p["mat_index"]), dev(torch, p["flat"]), mmap, d_nrm=d["B"][1])
    ms2 = IP.InstancedMaterialSet.from_dev(isc2, [sh, p["box"][1]], mats, texs)
    st = isc2.new_stats()
    same("a second handle", (ms2.render(cam, resx, resy, p["lights"], stats=st).cpu().numpy(), st.cpu().numpy()), wantB)
    ms2.rebuild_blas_dev({SHEET: d["A"]})
    with pytest.raises(_lib.SnailError, match="rebuilt"):
        frame()
    # the list refusals that need a set
    L = _lib.lib()
    for bad, text in (({BOX: d["A"]}, "not a Scene.from_fast_dev BLAS"), ({7: d["A"]}, "out of range")):
        with pytest.raises(_lib.SnailError, match=text):
            ms.rebuild_blas_dev(bad)
    arr = (IP._BlasRebuild * 1)()
    arr[0].blas, arr[0].d_verts9, arr[0].d_perm = BOX, d["A"][0].data_ptr(), sheet.d_perm.data_ptr()
    for fn in (L.snail_instances_materials_rebuild_dev, L.snail_instances_materials_update_dev):
        arr[0].blas = BOX
        assert fn(ms._h, C.cast(arr, C.c_void_p), 1, None) != 0 and "BLAS 1 is never rebuilt" in L.snail_last_error().decode()
        arr[0].blas = 2
        assert fn(ms._h, C.cast(arr, C.c_void_p), 1, None) != 0 and "BLAS index 2 is out of range (the handle has 2)" in L.snail_last_error().decode()
        assert fn(twin("A")[1]._h, C.cast(arr, C.c_void_p), 1, None) != 0 and "not made by snail_instances_materials_create_dev" in L.snail_last_error().decode()
    ms2.close(); isc2.close(); plain.close(); ms.close(); isc.close()


# ---- 5. ordering without host waits ----
def test_two_streams_no_host_wait(torch_mod):
    torch = torch_mod
    p = DK.poses()
    resx, resy = 96, 64
    cam = p["cams"][resx]
    isc, ms, d = dynamic(torch)
    wantA = frames_of(torch, *twin("A"), resx, resy, "ieee")["render"]
    wantB = frames_of(torch, *twin("B"), resx, resy, "ieee")["render"]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = [torch.zeros((resy, resx, 3), dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    stats = [isc.new_stats() for _ in range(2)]
    xf = (dev(torch, xf12()), dev(torch, np.asarray(p["bi"], dtype=np.int32)))
    isc.update_dev(*xf)                       # (the one-off host wait of the first update_dev, before the part that has none)
    torch.cuda.synchronize()
    ms.render(cam, resx, resy, p["lights"], out=outs[0], stats=stats[0], stream=s1)
    ms.rebuild_blas_dev({SHEET: d["B"]}, stream=s2)
    isc.update_dev(*xf, stream=s2)
    ms.render(cam, resx, resy, p["lights"], out=outs[1], stats=stats[1], stream=s1)
    torch.cuda.synchronize()
    same("before the rebuild", (outs[0].cpu().numpy(), stats[0].cpu().numpy()), wantA)
    same("after the rebuild", (outs[1].cpu().numpy(), stats[1].cpu().numpy()), wantB)
    ms.close(); isc.close()


# ---- 6. the older creators ----
def test_older_creators_still_refuse_a_device_built_blas(torch_mod):
    torch = torch_mod
    p = DK.poses()
    isc, ms, d = dynamic(torch)
    mats, texs = materials(False)
    with pytest.raises(_lib.SnailError, match="BLAS 0 carries no host permutation"):
        IP.InstancedMaterialSet(isc, [DK.sheet_data("A"), p["box"][1]], mats, texs)
    sh = [P.pack_shtris(*DK.sheet_data("A")[:4], isc.blas[SHEET].perm), P.pack_shtris(*p["box"][1][:4], isc.blas[BOX].bvh.perm)]
    for transparent in (False, True):
        with pytest.raises(_lib.SnailError, match="BLAS 0 is rebuilt on the device, which renumbers its triangles: no records for such a BLAS here"):
            IP.create_instanced_set(isc._h, sh, [p["material_map"], p["box"][1][4]], mats, texs, transparent)
    # and the new creator's two refusals that name the BLAS, through the C-ABI (the Python class sorts the forms out before)
    L = _lib.lib()
    per = (IP._BlasShadingDev * 2)()
    mp = [np.ascontiguousarray(m, dtype=np.int32) for m in (p["material_map"], p["box"][1][4])]
    for b in range(2):
        per[b].shtris64, per[b].nTris, per[b].matMap, per[b].nMap = sh[b].ctypes.data, len(sh[b]), mp[b].ctypes.data, len(mp[b])
    recs = P._material_records(mats)
    tex = P._texture_array(texs)
    create = lambda: L.snail_instances_materials_create_dev(isc._h, C.cast(per, C.c_void_p), 2, _lib.ptr(recs), len(recs), None, C.cast(tex, C.c_void_p), len(texs), None)   # noqa: E731
    assert not create() and "BLAS 0 is rebuilt on the device, which renumbers its triangles, and was given host records" in L.snail_last_error().decode()
    per[0].shtris64 = None
    duv, dmi = dev(torch, p["uv"]), dev(torch, p["mat_index"])
    per[0].d_uv6, per[0].d_matIdx, per[0].d_perm, per[0].d_nrm9 = duv.data_ptr(), dmi.data_ptr(), isc.blas[SHEET].d_perm.data_ptr(), d["A"][1].data_ptr()
    per[1].shtris64 = None
    per[1].d_uv6, per[1].d_matIdx, per[1].d_perm, per[1].d_nrm9 = per[0].d_uv6, per[0].d_matIdx, per[0].d_perm, per[0].d_nrm9
    assert not create() and "BLAS 1 was not made by snail_scene_create_fast_dev and was given device data" in L.snail_last_error().decode()
    ms.close(); isc.close()
