"""Transparent materials under full shading on the MI355X (include/snail_materials_transparency.h): the sample stages with Sample::opacity and the
transSel selector -- k_mat_sample_transp and k_mat_sample_transp_rays -- and the continuation generator -- k_mat_continue and
k_mat_continue_rays (snail_amd/csrc/materials_transparency.inc) -- on the synthetic records of tests/materials_transparency_cases.py, bit for bit
against the restatement (tests/materials_transparency_ref.py) in both arithmetics; a set of the new creator WITHOUT a transparent-capable material
against the existing sample kernels, device against device; two levels down on the hits of existing cases with a material swapped, through the
continuation's walk, with TreeStats; the frames that run the levels on the device -- `panes` through _dev, _packets_dev and _image with the case's
lights, none and eight, the cut at max_depth = 2 with its truncated count, an opaque set against the existing frames --; and the refusal of a
capable set by every older entry point.  What the lists must
exercise is asserted on the restatement's diagnostics here and, without a GPU, by tests/test_materials_transparency_host.py."""
import functools

import numpy as np
import pytest

from snail_amd import HostBVH, _lib
from snail_amd import materials as P
from snail_amd.scene import Scene
from tests import materials_synth as Y
from tests import materials_transparency_cases as TK
from tests import oracle_lib as O
from tests.test_gpu_materials_synth import compare_planes, dev, primary_dirs, records

pytestmark = pytest.mark.gpu
ARITH = [("ieee", O.MODE_IEEE), ("host_sse", O.MODE_SSE)]
INF = np.float32(np.inf)
RESX, RESY = Y.FRAME
CAM = Y.Cam()


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def product_materials(descs):
    out = []
    for d in descs:
        out.append(P.Material.simple(d[1], d[2]) if d[0] == "simple" else P.Material.textured(d[1], d[2]) if d[0] == "tex" else
                   P.Material.transparent(d[1], d[2], d[3]) if d[0] == "transp" else P.Material.uber(d[1], d[2], d[3]))
    return out


@functools.lru_cache(maxsize=None)
def device_sets():
    """(Scene, the set with transparent-capable materials, the new creator's set with opaque stand-ins, the OLD creator's set of the same
    stand-ins) over the synthetic triangles, built once"""
    s = Y.synth()
    hb = HostBVH.build(s.tv)
    assert np.array_equal(hb.perm, s.osc.perm) and hb.nodes.tobytes() == s.osc.nodes.tobytes()
    sc = Scene(hb, 0)
    tx = [P.Texture(t) for t in TK.textures()]
    args = (sc, s.uv, s.nrm, s.mat_index, s.flat, s.material_map)
    capable = P.MaterialSet(*args, product_materials(TK.descs()), tx, transparent=True)
    opaque_new = P.MaterialSet(*args, product_materials(TK.descs_opaque()), tx, transparent=True)
    opaque_old = P.MaterialSet(*args, product_materials(TK.descs_opaque()), tx)
    return sc, capable, opaque_new, opaque_old


def shade_packets_transp(torch, ms, r, xy):
    out = ms.shade_packets_transp(CAM, RESX, RESY, dev(torch, xy), (dev(torch, r["t"]), dev(torch, r["u"]), dev(torch, r["v"]), dev(torch, r["tri"])))
    return [a.cpu().numpy() for a in out]


def shade_rays_transp(torch, ms, r, dirs, mask, pick=None):
    sel = (lambda a: a) if pick is None else (lambda a: a[pick])
    out = ms.shade_rays_transp(dev(torch, sel(dirs)), None if mask is None else dev(torch, sel(mask)), dev(torch, sel(r["t"])), dev(torch, sel(r["u"])),
                               dev(torch, sel(r["v"])), dev(torch, sel(r["tri"])))
    return [a.cpu().numpy() for a in out]


def compare_stage(what, got, want, pick=None):
    """the nine planes, the opacity plane and the selector bytes, all by bit pattern; prints each count before it asserts"""
    w = {k: (a if pick is None else a[pick]) for k, a in want.items()}
    op = np.ascontiguousarray(got[1]).view(np.uint32) != np.ascontiguousarray(w["opacity"]).view(np.uint32)
    se = got[2] != w["sel"]
    print("%s: opacity %d differing words of %d, selector %d differing bytes of %d (%d non-zero expected)" % (what, int(op.sum()), op.size, int(se.sum()), se.size,
                                                                                                              int((w["sel"] != 0).sum())))
    compare_planes(what, got[0], np.ascontiguousarray(w["samples"]))
    assert not op.any(), (what, "opacity", np.argwhere(op)[:4].tolist(), got[1][tuple(np.argwhere(op)[0])], w["opacity"][tuple(np.argwhere(op)[0])])
    assert not se.any(), (what, "selector", np.argwhere(se)[:4].tolist(), int(got[2][tuple(np.argwhere(se)[0])]), int(w["sel"][tuple(np.argwhere(se)[0])]))


# ---- 1. the sample stages with transparency ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_primary_sample_stage_with_transparency(torch_mod, arith, mode):
    sc, ms, _, _ = device_sets()
    want, d = TK.expected_primary(mode)
    sc.set_arith(arith)
    try:
        got = shade_packets_transp(torch_mod, ms, records(False), Y.synth().packet_xy())
    finally:
        sc.set_arith("ieee")
    print(TK.describe(d))
    compare_stage("primary list, %s" % arith, got, want)
    TK.check_conditions(d, False)


@pytest.mark.parametrize("arith,mode", ARITH)
def test_generic_sample_stage_with_transparency(torch_mod, arith, mode):
    """the caller's directions and masks; the packets whose lanes are all selected once more without a mask array"""
    sc, ms, _, _ = device_sets()
    want, d = TK.expected_generic()
    r = records(True)
    full = np.flatnonzero((r["mask"] == 15).all(axis=1))
    sc.set_arith(arith)
    try:
        got = shade_rays_transp(torch_mod, ms, r, r["dirs"], r["mask"])
        got_full = shade_rays_transp(torch_mod, ms, r, r["dirs"], None, full)
    finally:
        sc.set_arith("ieee")
    print(TK.describe(d))
    compare_stage("generic list, %s" % arith, got, want)
    compare_stage("generic list, the %d all-selected packets without a mask array, %s" % (len(full), arith), got_full, want, full)
    TK.check_conditions(d, True)
    assert 8 <= len(full) <= Y.N_PACKETS - 8                         # hasMask takes both values


@pytest.mark.parametrize("arith,mode", ARITH)
def test_the_two_transparency_stages_agree_on_the_primary_list(torch_mod, arith, mode):
    """k_mat_sample_transp_rays on the primary list's records with the generator's directions and no mask is k_mat_sample_transp: device
    against device"""
    sc, ms, _, _ = device_sets()
    r = records(False)
    sc.set_arith(arith)
    try:
        a = shade_packets_transp(torch_mod, ms, r, Y.synth().packet_xy())
        b = shade_rays_transp(torch_mod, ms, r, primary_dirs(mode), None)
    finally:
        sc.set_arith("ieee")
    compare_planes("twins, %s" % arith, b[0], a[0])
    assert b[1].tobytes() == a[1].tobytes() and b[2].tobytes() == a[2].tobytes() and a[2].any() and (a[1] > 0).any()


# ---- 2. a set of the new creator without a capable material: the existing kernels' planes, nothing selected ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_a_set_without_capable_materials_samples_as_the_existing_stages(torch_mod, arith, mode):
    torch = torch_mod
    sc, _, new, old = device_sets()
    assert not new.can_select_transparent and not old.can_select_transparent
    rp, rg = records(False), records(True)
    xy = Y.synth().packet_xy()
    sc.set_arith(arith)
    try:
        p_new = shade_packets_transp(torch, new, rp, xy)
        g_new = shade_rays_transp(torch, new, rg, rg["dirs"], rg["mask"])
        hits = (dev(torch, rp["t"]), dev(torch, rp["u"]), dev(torch, rp["v"]), dev(torch, rp["tri"]))
        # the existing stages: on the old creator's set, and -- the set being acceptable to them -- on the new creator's as well
        p_old = [ms.shade_packets(CAM, RESX, RESY, dev(torch, xy), hits).cpu().numpy() for ms in (old, new)]
        g_old = [ms.shade_rays(dev(torch, rg["dirs"]), dev(torch, rg["mask"]), dev(torch, rg["t"]), dev(torch, rg["u"]), dev(torch, rg["v"]), dev(torch, rg["tri"])).cpu().numpy()
                 for ms in (old, new)]
    finally:
        sc.set_arith("ieee")
    for k in range(2):
        compare_planes("opaque set, primary list, %s, existing stage on set %d" % (arith, k), p_new[0], p_old[k])
        compare_planes("opaque set, generic list, %s, existing stage on set %d" % (arith, k), g_new[0], g_old[k])
    assert not p_new[2].any() and not g_new[2].any()                  # no lane selected
    want_p, _ = TK.expected_primary(mode, True)
    want_g, _ = TK.expected_generic(True)
    assert p_new[1].tobytes() == want_p["opacity"].tobytes() and g_new[1].tobytes() == want_g["opacity"].tobytes()
    assert set(np.unique(p_new[1]).tolist()) == {0.0, 1.0}            # UBER writes its dissolve whether flagged or not


# ---- 3. the continuation generator ----
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("generic", [False, True])
def test_continuation_generator(torch_mod, generic, arith, mode):
    """a level's rays (the camera's, or generic packets with inverse directions that are not SafeInv(dir)), hits and selector bytes -- bits on
    lanes that missed among them -> all six outputs by bytes, the order words, and the nested call's TracingRays"""
    torch = torch_mod
    sc, ms, _, _ = device_sets()
    c = TK.continue_inputs()
    want, selected = TK.expected_continue(mode, generic)
    n = len(c["xy"])
    t = dev(torch, c["t"].reshape(n, 256))
    sel = dev(torch, TK.T.sel_bytes(c["sel"]))
    sc.set_arith(arith)
    try:
        st = sc.new_stats()
        if generic:
            got = ms.continue_packets(t, sel, rays=(dev(torch, c["origin"]), dev(torch, c["dir"]), dev(torch, c["idir"])), stats=st)
        else:
            got = ms.continue_packets(t, sel, cam=CAM, resx=RESX, resy=RESY, packet_xy=dev(torch, c["xy"]), stats=st)
        got = [a.cpu().numpy() for a in got]
        st = st.cpu().numpy()
    finally:
        sc.set_arith("ieee")
    failed = []
    for k, g in zip(TK.KEYS + ("order",), got):
        w = want[k]
        g = np.ascontiguousarray(g.reshape(w.shape))
        assert g.dtype == w.dtype, (k, g.dtype, w.dtype)
        ne = g.view(np.uint8) != w.view(np.uint8)
        print("continue generic=%s %s %s: %d differing bytes of %d" % (generic, arith, k, int(ne.sum()), ne.size))
        if ne.any():
            failed.append((k, int(ne.sum()), np.argwhere(ne)[:4].tolist()))
    assert not failed, failed
    assert st.tolist() == [0, 0, selected, 0] and selected >= 1024
    assert (want["order"] == -1).sum() >= 5 and (want["order"] >= 0).sum() >= 8


# ---- 4. the way down on traced hits: sample -> generator -> the continuation's walk -> sample -> generator ----
_swapped = {}


def swapped_set(name):
    if name not in _swapped:
        c, _ = TK.swapped_case(name)
        hb = HostBVH.build(c["tv"])
        assert np.array_equal(hb.perm, c["osc"].perm) and hb.nodes.tobytes() == c["osc"].nodes.tobytes()
        sc = Scene(hb, 0)
        ms = P.MaterialSet(sc, c["uv"], c["nrm"], c["mat_index"], c["flat"], c["material_map"], product_materials(c["descs"]), [P.Texture(t) for t in c["textures"]],
                           transparent=True)
        _swapped[name] = (c, sc, ms)
    return _swapped[name]


def equal_bytes(what, got, want):
    g, w = np.ascontiguousarray(got.reshape(want.shape)), np.ascontiguousarray(want)
    assert g.dtype == w.dtype, (what, g.dtype, w.dtype)
    ne = g.view(np.uint8) != w.view(np.uint8)
    print("%s: %d differing bytes of %d" % (what, int(ne.sum()), ne.size))
    assert not ne.any(), (what, int(ne.sum()), np.argwhere(ne)[:4].tolist())


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("name", TK.SWAPPED)
def test_two_levels_down_on_an_existing_case_with_a_material_swapped(torch_mod, name, arith, mode):
    """the 70 x 50 frame of a case of tests/materials_cases.py with one material swapped for TRANSPARENT (and UBER 0 for UBER 0.5): the
    device's primary walk, sample stage, generator, the walk of the generated packets by snail_trace_rays_dev, the sample stage on them and the
    generator once more, every intermediate by bytes and the TreeStats for equality against the restatement with the oracle's walks.  The
    order words pick the packets that nest: a packet without a selected lane makes no nested call."""
    torch = torch_mod
    c, sc, ms = swapped_set(name)
    resx, resy = TK.SWAP_FRAME
    cam = c["cam70"]
    levels, wst, xy, d = TK.swapped_descent(name, mode)
    l0, l1, l2 = levels
    sc.set_arith(arith)
    try:
        st = sc.new_stats()
        dxy = dev(torch, xy)
        hits = sc.trace_packets(cam, resx, resy, dxy, stats=st)
        smp0, op0, sel0 = ms.shade_packets_transp(cam, resx, resy, dxy, hits)
        cont1 = ms.continue_packets(hits[0], sel0, cam=cam, resx=resx, resy=resy, packet_xy=dxy, stats=st)
        order1 = cont1[6].cpu().numpy()
        act = torch.from_numpy(np.flatnonzero(order1 >= 0)).to("cuda:0")
        org, dr, idr, mask, dist, obj = (a[act].contiguous() for a in cont1[:6])
        m = int(act.shape[0])
        bary = torch.zeros((m, 64, 8), dtype=torch.float32, device="cuda:0")
        _lib.check(_lib.lib().snail_trace_rays_dev(sc._h, m, 64, 0, _lib.ptr(org), _lib.ptr(dr), _lib.ptr(idr), _lib.ptr(mask), _lib.ptr(dist), _lib.ptr(obj), _lib.ptr(bary),
                                                  _lib.ptr(st), None), "snail_trace_rays_dev")
        u, v = bary[:, :, 0:4].reshape(m, 256).contiguous(), bary[:, :, 4:8].reshape(m, 256).contiguous()
        smp1, op1, sel1 = ms.shade_rays_transp(dr, mask, dist, u, v, obj)
        cont2 = ms.continue_packets(dist, sel1, rays=(org, dr, idr), stats=st)
        torch.cuda.synchronize()
        st = st.cpu().numpy().astype(np.uint64)
    finally:
        sc.set_arith("ieee")
    tag = "%s %s" % (name, arith)
    for k, g in zip(("t", "u", "v", "tri"), hits):
        equal_bytes("%s level 0 %s" % (tag, k), g.cpu().numpy(), l0[k])
    for k, g in (("samples", smp0), ("opacity", op0), ("sel", sel0)):
        equal_bytes("%s level 0 %s" % (tag, k), g.cpu().numpy(), l0[k])
    for k, g in zip(TK.KEYS + ("order",), cont1):
        equal_bytes("%s level 1 generator %s" % (tag, k), g.cpu().numpy(), l1["cont"][k])
    assert np.array_equal(np.flatnonzero(order1 >= 0), l1["packets"]) and 8 <= m < len(xy)          # some packets nest, some do not
    for k, g in (("dist", dist), ("obj", obj), ("bary", bary), ("samples", smp1), ("opacity", op1), ("sel", sel1)):
        equal_bytes("%s level 1 %s" % (tag, k), g.cpu().numpy(), l1[k])
    for k, g in zip(TK.KEYS + ("order",), cont2):
        equal_bytes("%s level 2 generator %s" % (tag, k), g.cpu().numpy(), l2["cont"][k])
    print("%s: stats %s / %s; %s" % (tag, st.tolist(), wst.tolist(), TK.describe(d)))
    assert np.array_equal(st, wst), (st, wst)
    assert (l1["dist"] < INF).sum() >= 1024 and ((l1["dist"] == INF).sum() >= 64)                  # continuation lanes that hit, and that miss
    assert (l1["cont"]["mask"] == 15).all(axis=1).any()                                            # a packet that goes as RayGroup<0, 0>
    if name == "small":
        assert (l2["cont"]["order"] >= 0).sum() >= 4 and (l2["cont"]["order"] == -1).sum() >= 4    # level 1 selects again in some packets


# ---- 5. frames: the levels on the device ----
_frames = {}


def panes_set(opaque=False):
    """(case, Scene, MaterialSet of the new creator) of `panes`, or of `panes` with opaque stand-ins; built once"""
    if opaque not in _frames:
        c = TK.panes()
        hb = HostBVH.build(c["tv"])
        assert np.array_equal(hb.perm, c["osc"].perm) and hb.nodes.tobytes() == c["osc"].nodes.tobytes()
        sc = Scene(hb, 0)
        mats = []
        for d in c["descs"]:
            if opaque and d[0] == "transp":
                d = ("tex", d[1], d[3])
            elif opaque and d[0] == "uber" and 0.0 < d[3] < 1.0:
                d = ("uber", d[1], d[2], 0.0)
            mats += product_materials([d])
        ms = P.MaterialSet(sc, c["uv"], c["nrm"], c["mat_index"], c["flat"], c["material_map"], mats, [P.Texture(t) for t in c["textures"]], transparent=True)
        _frames[opaque] = (c, sc, ms)
    return _frames[opaque]


def check_frame(what, got, want, st, wst, trunc, wtrunc):
    bad = np.argwhere((got != want).any(axis=-1))
    print("%s: %d differing pixels; stats %s / %s; truncated %d / %d" % (what, len(bad), np.asarray(st).tolist(), wst.tolist(), int(trunc), int(wtrunc)))
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())
    assert np.array_equal(np.asarray(st).astype(np.uint64), wst), (what, st, wst)
    assert int(trunc) == int(wtrunc), (what, trunc, wtrunc)


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("lights", ["case", "none", "eight"])
@pytest.mark.parametrize("resx,resy", TK.PANES_FRAMES)
def test_panes_frames_equal_the_restatement(torch_mod, resx, resy, lights, arith, mode):
    """`panes` through _dev, _packets_dev (a shuffled sublist) and _image: frames byte for byte, TreeStats and the truncated count for equality"""
    torch = torch_mod
    c, sc, ms = panes_set()
    want, wst, wtrunc, d, xy = TK.panes_frame(resx, resy, mode, 8, lights)
    L = TK.lights_of(c, lights)
    xy = np.asarray(xy, dtype=np.int32).reshape(-1, 2)
    pick = np.random.RandomState(3).permutation(len(xy))[: (2 * len(xy)) // 3]
    wsub = TK.case_ref(c).render_packets(c["cam"].as_array13(), resx, resy, xy[pick], L, mode=mode, max_depth=8)
    sc.set_arith(arith)
    try:
        st = sc.new_stats()
        frame, tr = ms.render_transparent(c["cam"], resx, resy, L, stats=st, max_depth=8)
        st2 = sc.new_stats()
        sub, tr2 = ms.render_transparent_packets(c["cam"], resx, resy, dev(torch, xy[pick]), L, stats=st2, max_depth=8)
        img, st3, tr3 = ms.render_transparent_image_host(c["cam"], resx, resy, L, max_depth=8)
        frame, sub, st, st2, tr, tr2 = (a.cpu().numpy() for a in (frame, sub, st, st2, tr, tr2))
    finally:
        sc.set_arith("ieee")
    tag = "panes %dx%d %s lights %s" % (resx, resy, lights, arith)
    print(TK.describe_frame(d))
    check_frame(tag + " _dev", frame, want, st, wst, tr[0], wtrunc)
    check_frame(tag + " _packets_dev", sub, wsub[0], st2, wsub[1], tr2[0], wsub[2])
    check_frame(tag + " _image", img.reshape(resy, resx, 3), want, st3, wst, tr3[0], wtrunc)
    assert wtrunc == 0 and d.deepest >= 3 and want.any()


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("resx,resy", TK.PANES_FRAMES)
def test_panes_cut_at_depth_2(torch_mod, resx, resy, arith, mode):
    """max_depth = 2: the frame (the lanes level 2 still selects keep their diffuse), TreeStats and the truncated count are the restatement's;
    the counter is added to, and a second frame on the same set at depth 8 is the uncut one"""
    c, sc, ms = panes_set()
    want, wst, wtrunc, d, _ = TK.panes_frame(resx, resy, mode, 2)
    full = TK.panes_frame(resx, resy, mode, 8)
    sc.set_arith(arith)
    try:
        st = sc.new_stats()
        frame, tr = ms.render_transparent(c["cam"], resx, resy, c["lights"], stats=st, max_depth=2)
        frame2, tr = ms.render_transparent(c["cam"], resx, resy, c["lights"], max_depth=2, truncated=tr)
        st8 = sc.new_stats()
        frame8, tr8 = ms.render_transparent(c["cam"], resx, resy, c["lights"], stats=st8, max_depth=8)
        frame, frame2, frame8, st, st8, tr, tr8 = (a.cpu().numpy() for a in (frame, frame2, frame8, st, st8, tr, tr8))
    finally:
        sc.set_arith("ieee")
    check_frame("panes %dx%d depth 2 %s" % (resx, resy, arith), frame, want, st, wst, tr[0], 2 * wtrunc)
    check_frame("panes %dx%d depth 8 after depth 2 %s" % (resx, resy, arith), frame8, full[0], st8, full[1], tr8[0], 0)
    assert wtrunc > 0 and d.deepest == 2 and np.array_equal(frame2, frame) and (want != full[0]).any()


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("depth", [1, 8])
def test_a_set_without_capable_materials_renders_as_the_existing_frames(torch_mod, depth, arith, mode):
    """a new-creator set of `panes` with opaque stand-ins: byte-equal to snail_render_materials_packets_dev with equal stats, device against device"""
    torch = torch_mod
    c, sc, ms = panes_set(opaque=True)
    assert not ms.can_select_transparent
    resx, resy = 70, 50
    from tests import dbvh_shade_ref as S
    dxy = dev(torch, np.asarray(S.frame_packets(resx, resy), dtype=np.int32).reshape(-1, 2))
    sc.set_arith(arith)
    try:
        st, st0 = sc.new_stats(), sc.new_stats()
        got, tr = ms.render_transparent_packets(c["cam"], resx, resy, dxy, c["lights"], stats=st, max_depth=depth)
        want = ms.render_packets(c["cam"], resx, resy, dxy, c["lights"], stats=st0)
        got, want, st, st0, tr = (a.cpu().numpy() for a in (got, want, st, st0, tr))
    finally:
        sc.set_arith("ieee")
    check_frame("opaque panes depth %d %s" % (depth, arith), got, want, st, st0.astype(np.uint64), tr[0], 0)
    assert want.any() and st0[2] > 256 * 20


# ---- 6. a capable set and the older entry points ----
def test_every_older_entry_point_refuses_a_capable_set(torch_mod):
    torch = torch_mod
    sc, ms, _, _ = device_sets()
    assert ms.can_select_transparent
    rp, rg = records(False), records(True)
    xy = dev(torch, Y.synth().packet_xy())
    hits = (dev(torch, rp["t"]), dev(torch, rp["u"]), dev(torch, rp["v"]), dev(torch, rp["tri"]))
    smp = torch.zeros((Y.N_PACKETS, 9, 64, 4), dtype=torch.float32, device="cuda:0")
    tiles = np.array([[0, 0, 32, 32]], dtype=np.int32)
    calls = {
        "snail_materials_shade_packets_dev": lambda: ms.shade_packets(CAM, RESX, RESY, xy, hits),
        "snail_materials_mirror_packets_dev": lambda: ms.mirror_packets(CAM, RESX, RESY, xy, hits[0], smp),
        "snail_materials_shade_rays_dev": lambda: ms.shade_rays(dev(torch, rg["dirs"]), None, dev(torch, rg["t"]), dev(torch, rg["u"]), dev(torch, rg["v"]), dev(torch, rg["tri"])),
        "snail_render_materials_dev": lambda: ms.render(CAM, RESX, RESY),
        "snail_render_materials_packets_dev": lambda: ms.render_packets(CAM, RESX, RESY, xy),
        "snail_render_materials_image": lambda: ms.render_image_host(CAM, RESX, RESY),
        "snail_materials_bounce_dev": lambda: ms.render(CAM, RESX, RESY, reflections=True),
        "snail_materials_bounce_packets_dev": lambda: ms.render_packets(CAM, RESX, RESY, xy, reflections=True),
        "snail_materials_bounce_image": lambda: ms.render_image_host(CAM, RESX, RESY, reflections=True),
        "snail_materials_frame_packets_dev": lambda: ms.frame_packets(CAM, RESX, RESY, xy, flags=P.RENDER_AA4),
        "snail_materials_render_tiles": lambda: ms.render_tiles_host(CAM, RESX, RESY, tiles),
        "snail_materials_render_frame": lambda: ms.render_frame_host(CAM, RESX, RESY, flags=P.RENDER_AA4),
    }
    from snail_amd._lib import MATERIALS_BOUNCE_SIGNATURES, MATERIALS_SIGNATURES, MATERIALS_TILES_SIGNATURES
    takes_a_set = {k for t in (MATERIALS_SIGNATURES, MATERIALS_BOUNCE_SIGNATURES, MATERIALS_TILES_SIGNATURES) for k in t} - {
        "snail_shtris_pack", "snail_texture_size", "snail_texture_build", "snail_materials_create", "snail_materials_destroy"}
    assert set(calls) == takes_a_set
    for name, call in calls.items():
        with pytest.raises(_lib.SnailError) as e:
            call()
        assert name in str(e.value) and "transparent" in str(e.value), (name, str(e.value))
