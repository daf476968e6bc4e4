"""The transparency continuation under full shading of instanced scenes on the MI355X
(include/snail_instances_materials_transparency.h; InstancedMaterialSet(..., transparent=True), .shade_packets_transp / .shade_rays_transp /
.continue_packets / .render_transparent*): the sample stages with opacity and selector -- k_imat_sample_transp / _rays --, the generator, the
levels' walk under the order list -- k_imat_trace_level --, the levels' lights -- k_imat_light_transp -- and the frames, bit for bit, byte for
byte and TreeStats and counters for equality against the test-side restatement tests/instances_materials_transparency_ref.py, in both
arithmetics; and, independent of that restatement, invisible panes against the existing frames of the scene without them, a set without
capable materials against the existing stages and frames, and the sample stages against themselves on synthetic records.  The cases
(tests/instances_materials_transparency_cases.py) were chosen with the restatement alone; what they must exercise is asserted on its counters
without a GPU by tests/test_instances_materials_transparency_host.py.  Nothing here reads outside the repository."""
import functools

import numpy as np
import pytest

from snail_amd import HostBVH, _lib
from snail_amd import instances_materials as IP
from snail_amd import materials as P
from snail_amd.instances import InstancedScene
from snail_amd.scene import Context, Scene
from tests import instances_materials_synth as Z
from tests import instances_materials_transparency_cases as C
from tests import instances_materials_transparency_ref as IT
from tests import materials_ref as M
from tests import materials_synth as Y
from tests import materials_transparency_cases as TK
from tests import materials_transparency_ref as T
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu
ARITH = [("ieee", O.MODE_IEEE), ("host_sse", O.MODE_SSE)]
INF = np.float32(np.inf)
STAGE = ("glasshouse", 96, 64)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_blas, _sets = {}, {}


def blas_scene(key, tv, osc):
    """the device Scene of a BLAS, built once; the product builder's tree is the oracle's"""
    if key not in _blas:
        hb = HostBVH.build(tv)
        assert np.array_equal(hb.perm, osc.perm) and hb.nodes.tobytes() == osc.nodes.tobytes()
        _blas[key] = Scene(hb, 0)
    return _blas[key]


def product_materials(descs, textures):
    mats = [P.Material.simple(d[1], d[2]) if d[0] == "simple" else P.Material.textured(d[1], d[2]) if d[0] == "tex" else
            P.Material.transparent(d[1], d[2], d[3]) if d[0] == "transp" else P.Material.uber(d[1], d[2], d[3]) for d in descs]
    return mats, [P.Texture(t) for t in textures]


def check_tree(isc, ref):
    xs, bs = isc.slot_transforms()
    assert isc.nodes().tobytes() == ref.nodes.tobytes() and np.array_equal(xs, ref.xf) and np.array_equal(bs, ref.bi)


def new_set(name, panes=True, opaque=False, transparent=True):
    c = C.case(name, panes)
    keys = ["chain", "pane"] if name == "deep" else ["sheet", "box", "pane", "pane2"]
    scs = [blas_scene(k, tv, osc) for k, tv, osc in zip(keys, c["tvs"], c["oscs"])]
    isc = InstancedScene(scs, c["rot"], c["tr"], c["bi"])
    check_tree(isc, c["ref"])
    mats, texs = product_materials(C.opaque_descs(c["descs"]) if opaque else c["descs"], C.textures())
    return isc, IP.InstancedMaterialSet(isc, c["per_blas"], mats, texs, transparent=transparent)


def device_set(name, panes=True, opaque=False, transparent=True):
    """(InstancedScene, InstancedMaterialSet) of a case, built once; the handle's tree and records are the case's own (built without a GPU)"""
    key = (name, panes, opaque, transparent)
    if key not in _sets:
        _sets[key] = new_set(*key)
    return _sets[key]


def set_arith(isc, arith):
    for s in isc.blas:
        s.set_arith(arith)


def dev(torch, a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")      # (a copy: the shared inputs are read-only)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def assert_bits(what, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    ne = bits(got) != bits(want)
    print("%s: %d differing words of %d" % (what, int(ne.sum()), ne.size))
    if ne.any():
        at = tuple(np.argwhere(ne)[0])
        raise AssertionError("%s: %d words differ; first at %s: %r / %r" % (what, int(ne.sum()), at, got[at], want[at]))


def assert_frame(frame, want, st, wst, what):
    bad = np.argwhere((frame != want).any(axis=2))
    print("%s: %d differing pixels; stats %s / %s" % (what, len(bad), np.asarray(st).tolist(), np.asarray(wst).tolist()))
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), frame[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())
    assert np.array_equal(np.asarray(st).astype(np.uint64), np.asarray(wst).astype(np.uint64)), (what, st, wst)


def assert_samples(what, got, want):
    """(samples, opacity, sel) of the device against a level's records"""
    smp, op, sel = (g.cpu().numpy() for g in got)
    n = len(want["t"])
    assert_bits(what + ": nine planes", smp, want["samples"])
    assert_bits(what + ": opacity", op, want["opacity"].reshape(n, 256))
    assert_bits(what + ": selector", sel, want["sel"])


def hits_of(torch, r):
    n = len(r["t"])
    return (dev(torch, r["t"].reshape(n, 256)), dev(torch, r["bary"][:, :, 0:4].reshape(n, 256)), dev(torch, r["bary"][:, :, 4:8].reshape(n, 256)),
            dev(torch, r["inst"].reshape(n, 256)), dev(torch, r["tri_id"].reshape(n, 256)))


def rays_args(torch, r, mask=True):
    """a generic level's records as the arguments of shade_rays_transp"""
    n = len(r["t"])
    return [dev(torch, r["dir"]), dev(torch, r["mask"]) if mask else None, dev(torch, r["t"].reshape(n, 256)), dev(torch, r["bary"].reshape(n, 64, 2, 4)),
            dev(torch, r["inst"].reshape(n, 256)), dev(torch, r["tri_id"].reshape(n, 256))]


def walk(torch, isc, m, stats=None):
    """the device's walk of generic packets given as device tensors (origin, dir, idir, mask, distance, object, element, bary): in place"""
    org, d, idir, mask, dist, obj, elem, bary = m
    n = d.shape[0]
    ctx = Context(origin=org.view(n * 64, 12), dir=d.view(n * 64, 12), idir=idir.view(n * 64, 12), distance=dist.view(n * 64, 4), object=obj.view(n * 64, 4),
                  barycentric=bary.view(n * 64, 8), size=64, shared_origin=False, mask=mask.view(n * 64))
    isc.traverse_primary(ctx, elem, stats=stats)
    return dist, obj, elem, bary


# ---- 1. primary and generic sample stages on the restatement's level records ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_sample_stages_equal_the_restatement_on_its_level_records(torch_mod, arith, mode):
    torch = torch_mod
    name, resx, resy = STAGE
    isc, ms = device_set(name)
    cam = C.case(name)["cams"][resx]
    _, _, _, d, xy, rec = C.reference(name, resx, resy, mode)
    set_arith(isc, arith)
    try:
        _, l0 = C.level_records(rec, 0)
        assert_samples("primary, %s" % arith, ms.shade_packets_transp(cam, resx, resy, dev(torch, xy), hits_of(torch, l0)), l0)
        assert l0["sel"].any() and (l0["opacity"] > 0).any()
        for level in (1, 2, 3):
            idx, r = C.level_records(rec, level)
            assert len(idx) >= 1
            assert_samples("level %d (%d packets), %s" % (level, len(idx), arith), ms.shade_rays_transp(*rays_args(torch, r)), r)
    finally:
        set_arith(isc, "ieee")
    assert d.deepest >= 3


# ---- 2. both stages on synthetic records, under the capable material list ----
@functools.lru_cache(maxsize=None)
def synth_set():
    scs = []
    for b in Z.blases():
        hb = HostBVH.build(b.tv)
        assert np.array_equal(hb.perm, b.osc.perm) and hb.nodes.tobytes() == b.osc.nodes.tobytes()
        scs.append(Scene(hb, 0))
    a = Z.arrangement()
    isc = InstancedScene(scs, a.rot, a.tr, a.bi_input)
    check_tree(isc, a.ref)
    mats, texs = product_materials(TK.descs(), TK.textures())
    return isc, IP.InstancedMaterialSet(isc, [b.per_blas for b in Z.blases()], mats, texs, transparent=True)


@functools.lru_cache(maxsize=None)
def synth_ref():
    tx = Y.ref_textures() + [M.RefTexture(t) for t in TK.textures()[TK.N_TEX:]]
    return IT.InstTranspRef(Z.SynthRef(Z.arrangement().ref, [b.per_blas for b in Z.blases()], TK.ref_materials(TK.descs()), tx))


@functools.lru_cache(maxsize=None)
def synth_generic():
    """directions and selectors for the synthetic list as generic packets: materials_synth's, packet by packet"""
    s = Y.synth()
    pk = [s.packet(p % Y.N_PACKETS, generic=True) for p in range(Z.N_PACKETS)]
    return np.stack([p["dirs"] for p in pk]).astype(np.float32), np.stack([p["bits"] for p in pk])


@functools.lru_cache(maxsize=None)
def synth_expected(mode, generic):
    """the restatement over the synthetic records through the generator's clamp rule (tests/instances_materials_synth.py, clamp_records)"""
    r, ref, diag = Z.records(), synth_ref(), IT.SampleDiag()
    xy = Z.packet_xy()
    dirs, sel = synth_generic()
    outs = []
    for p in range(Z.N_PACKETS):
        s, key_tri, _ = Z.clamp_records(r["slot"][p], r["tri"][p])
        d = dirs[p] if generic else Y.primary_dirs(int(xy[p, 0]), int(xy[p, 1]), mode)
        outs.append(ref.samples(d, r["t"][p], s, key_tri, r["bary"][p], sel[p] if generic else None, diag))
    return TK.stack(outs), diag


def synth_hits(torch, r):
    n = len(r["t"])
    return (dev(torch, r["t"].reshape(n, 256)), dev(torch, r["bary"][:, :, 0:4].reshape(n, 256)), dev(torch, r["bary"][:, :, 4:8].reshape(n, 256)),
            dev(torch, r["slot"].reshape(n, 256)), dev(torch, r["tri"].reshape(n, 256)))


@pytest.mark.parametrize("arith,mode", ARITH)
def test_synthetic_records_under_the_capable_list(torch_mod, arith, mode):
    torch = torch_mod
    isc, ms = synth_set()
    r = Z.records()
    n = Z.N_PACKETS
    dirs, sel = synth_generic()
    mask = T.sel_bytes(sel)
    wp, dp = synth_expected(mode, False)
    wg, dg = synth_expected(mode, True)
    h = synth_hits(torch, r)
    gen = [dev(torch, dirs), dev(torch, mask), h[0], dev(torch, r["bary"].reshape(n, 64, 2, 4)), h[3], h[4]]
    set_arith(isc, arith)
    try:
        gp = [g.cpu().numpy() for g in ms.shade_packets_transp(Y.Cam(), Y.FRAME[0], Y.FRAME[1], dev(torch, Z.packet_xy()), h)]
        gg = [g.cpu().numpy() for g in ms.shade_rays_transp(*gen)]
        # device against device: an all-15 mask equals NULL
        full = [g.cpu().numpy() for g in ms.shade_rays_transp(gen[0], dev(torch, np.full((n, 64), 15, np.uint8)), *gen[2:])]
        null = [g.cpu().numpy() for g in ms.shade_rays_transp(gen[0], None, *gen[2:])]
        # ... and overwriting the masked lanes' records changes no output bit
        lanes = ~sel.reshape(n, 256)
        rng = np.random.RandomState(4)
        t2 = r["t"].reshape(n, 256).copy(); t2[lanes] = rng.uniform(0.5, 9.0, size=int(lanes.sum())).astype(np.float32)
        s2 = r["slot"].reshape(n, 256).copy(); s2[lanes] = rng.randint(-3, 40, size=int(lanes.sum()))
        i2 = r["tri"].reshape(n, 256).copy(); i2[lanes] = rng.randint(-3, 400, size=int(lanes.sum()))
        over = [g.cpu().numpy() for g in ms.shade_rays_transp(gen[0], gen[1], dev(torch, t2), gen[3], dev(torch, s2), dev(torch, i2))]
    finally:
        set_arith(isc, "ieee")
    for what, got, want in (("primary", gp, wp), ("generic", gg, wg)):
        assert_bits("synthetic %s planes, %s" % (what, arith), got[0], want["samples"])
        assert_bits("synthetic %s opacity, %s" % (what, arith), got[1], want["opacity"])
        assert_bits("synthetic %s selector, %s" % (what, arith), got[2], want["sel"])
    for k, what in enumerate(("planes", "opacity", "selector")):
        assert_bits("all-15 mask against NULL, " + what, full[k], null[k])
        assert_bits("masked lanes overwritten, " + what, over[k], gg[k])
    assert lanes.sum() >= 256 and (mask != 15).any()
    for d in (dp, dg):
        print(TK.describe(d))
        assert d.blocks_a_flag >= 8 and d.blocks_c_flag >= 8 and d.c_overwritten >= 1 and d.selected_lanes >= 256 and d.flagged_opaque_lanes >= 16


# ---- 3. the two stages agree on the primary list ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_the_two_stages_agree_on_the_primary_list(torch_mod, arith, mode):
    """the primary packets given to the generic stage with their camera directions and no mask: RayGroup<0, 0>, the same samples"""
    torch = torch_mod
    name, resx, resy = STAGE
    isc, ms = device_set(name)
    cam = C.case(name)["cams"][resx]
    xy = C.reference(name, resx, resy, mode)[4]
    dirs = np.stack([O.gen_packet(np.asarray(cam.as_array13(), dtype=np.float32), resx, resy, int(x), int(y), mode)[0].reshape(64, 3, 4) for x, y in xy.tolist()])
    set_arith(isc, arith)
    try:
        dxy = dev(torch, xy)
        hits = isc.trace_packets(cam, resx, resy, dxy)
        a = ms.shade_packets_transp(cam, resx, resy, dxy, hits)
        bary = torch.stack([hits[1].view(-1, 64, 4), hits[2].view(-1, 64, 4)], dim=2).contiguous()
        b = ms.shade_rays_transp(dev(torch, dirs), None, hits[0], bary, hits[3], hits[4])
        a, b = [x.cpu().numpy() for x in a], [x.cpu().numpy() for x in b]
    finally:
        set_arith(isc, "ieee")
    for k, what in enumerate(("planes", "opacity", "selector")):
        assert_bits("primary stage against generic stage, %s, %s" % (what, arith), a[k], b[k])
    assert a[2].any()


# ---- 4. a set without capable materials samples as the existing stages ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_a_set_without_capable_materials_samples_as_the_existing_stages(torch_mod, arith, mode):
    torch = torch_mod
    name, resx, resy = STAGE
    isc, ms = device_set(name, True, True, False)
    cam = C.case(name)["cams"][resx]
    _, _, _, _, xy, rec = C.reference(name, resx, resy, mode)
    _, r1 = C.level_records(rec, 1)
    assert ms.can_select_transparent is False
    set_arith(isc, arith)
    try:
        dxy = dev(torch, xy)
        hits = isc.trace_packets(cam, resx, resy, dxy)
        a = [x.cpu().numpy() for x in ms.shade_packets_transp(cam, resx, resy, dxy, hits)]
        old = ms.shade_packets(cam, resx, resy, dxy, hits).cpu().numpy()
        args = rays_args(torch, r1)
        b = [x.cpu().numpy() for x in ms.shade_rays_transp(*args)]
        old_rays = ms.shade_rays(*args).cpu().numpy()
    finally:
        set_arith(isc, "ieee")
    assert_bits("primary planes against shade_packets, %s" % arith, a[0], old)
    assert_bits("generic planes against shade_rays, %s" % arith, b[0], old_rays)
    # (UBER dissolve 1.0 writes opacity 1 and is flagged: it never selects)
    assert not a[2].any() and not b[2].any() and set(np.unique(a[1]).tolist()) <= {0.0, 1.0} and old.any() and old_rays.any()


# ---- 5. the generator ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_the_generator_for_primary_and_generic_input(torch_mod, arith, mode):
    torch = torch_mod
    name, resx, resy = STAGE
    isc, ms = device_set(name)
    cam = C.case(name)["cams"][resx]
    cam13 = np.asarray(cam.as_array13(), dtype=np.float32)
    _, _, _, _, xy, rec = C.reference(name, resx, resy, mode)
    _, l0 = C.level_records(rec, 0)
    _, l1 = C.level_records(rec, 1)
    keys = ("origin", "dir", "idir", "mask", "distance", "object", "element", "bary")
    org = np.repeat(cam13[:3].reshape(1, 3, 1), 4, axis=2).astype(np.float32)

    def sel_bits(b):
        return ((b.reshape(64, 1).astype(np.int32) >> np.arange(4).reshape(1, 4)) & 1).astype(bool)

    wp = [IT.InstTranspRef.continue_packets(O.gen_packet(cam13, resx, resy, int(x), int(y), mode)[0].reshape(64, 3, 4), org, None, l0["t"][p], sel_bits(l0["sel"][p]), mode)
          for p, (x, y) in enumerate(xy.tolist())]
    wg = [IT.InstTranspRef.continue_packets(l1["dir"][p], l1["origin"][p], l1["idir"][p], l1["t"][p], sel_bits(l1["sel"][p]), mode) for p in range(len(l1["t"]))]
    set_arith(isc, arith)
    try:
        n0, n1 = len(l0["t"]), len(l1["t"])
        st0, st1 = isc.new_stats(), isc.new_stats()
        gp = [g.cpu().numpy() for g in ms.continue_packets(dev(torch, l0["t"].reshape(n0, 256)), dev(torch, l0["sel"]), cam=cam, resx=resx, resy=resy,
                                                           packet_xy=dev(torch, xy), stats=st0)]
        gg = [g.cpu().numpy() for g in ms.continue_packets(dev(torch, l1["t"].reshape(n1, 256)), dev(torch, l1["sel"]),
                                                           rays=(dev(torch, l1["origin"]), dev(torch, l1["dir"]), dev(torch, l1["idir"])), stats=st1)]
    finally:
        set_arith(isc, "ieee")
    for what, got, want, st in (("primary", gp, wp, st0), ("generic", gg, wg, st1)):
        n = len(want)
        for k, g in zip(keys, got):
            w = np.stack([x[k] for x in want])
            assert_bits("generator, %s input, %s, %s" % (what, k, arith), g.reshape(w.shape), w)
        assert not got[5].any() and not got[6].any() and not got[7].view(np.uint32).any()
        order = np.array([p if want[p]["order_on"] else -1 for p in range(n)], dtype=np.int32)
        assert np.array_equal(got[8], order) and (order >= 0).any() and (order < 0).any(), (got[8], order)
        selected = sum(int((x["distance"] == INF).sum()) for x in want)
        assert st.cpu().numpy().tolist() == [0, 0, selected, 0] and selected >= 64


# ---- 6. two levels down by stages ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_two_levels_down_by_stages(torch_mod, arith, mode):
    """trace -> sample -> generator -> walk -> sample -> generator -> walk with the device's own outputs all the way: the restatement's level-1
    and level-2 hit records on the packets that reach those levels"""
    torch = torch_mod
    name, resx, resy = STAGE
    isc, ms = device_set(name)
    cam = C.case(name)["cams"][resx]
    _, _, _, _, xy, rec = C.reference(name, resx, resy, mode)
    i1, l1 = C.level_records(rec, 1)
    i2, l2 = C.level_records(rec, 2)
    set_arith(isc, arith)
    try:
        dxy = dev(torch, xy)
        hits = isc.trace_packets(cam, resx, resy, dxy)
        _, _, sel0 = ms.shade_packets_transp(cam, resx, resy, dxy, hits)
        c1 = ms.continue_packets(hits[0], sel0, cam=cam, resx=resx, resy=resy, packet_xy=dxy)
        d1, o1, e1, b1 = walk(torch, isc, c1[:8])
        _, _, sel1 = ms.shade_rays_transp(c1[1], c1[3], d1, b1, o1, e1)
        c2 = ms.continue_packets(d1, sel1, rays=(c1[0], c1[1], c1[2]))
        d2, o2, e2, b2 = walk(torch, isc, c2[:8])
        got1 = [x.cpu().numpy() for x in (d1, o1, e1, b1)]
        got2 = [x.cpu().numpy() for x in (d2, o2, e2, b2)]
        order1, order2 = c1[8].cpu().numpy(), c2[8].cpu().numpy()
    finally:
        set_arith(isc, "ieee")
    assert np.array_equal(np.flatnonzero(order1 >= 0), i1) and np.array_equal(np.flatnonzero(order2 >= 0), i2)
    for level, idx, got, want in ((1, i1, got1, l1), (2, i2, got2, l2)):
        n = len(idx)
        for g, k in zip(got, ("t", "inst", "tri_id", "bary")):
            assert_bits("level %d %s, %s" % (level, k, arith), g[idx].reshape(n, -1), want[k].reshape(n, -1))
    assert len({int(s) for s in np.unique(got2[1][i2][np.isfinite(got2[0][i2])])}) >= 2


# ---- 7. frames ----
FRAME_RUNS = [(96, 64, "case"), (70, 50, "case"), (64, 48, "case"), (64, 48, "none"), (64, 48, "eight")]


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("resx,resy,lights_key", FRAME_RUNS)
def test_frames_equal_the_restatement(torch_mod, resx, resy, lights_key, arith, mode):
    torch = torch_mod
    isc, ms = device_set("glasshouse")
    cam = C.case("glasshouse")["cams"][resx]
    lights = C.lights_of("glasshouse", lights_key)
    want, wst, wtr, d, xy, rec = C.reference("glasshouse", resx, resy, mode, lights_key)
    pbgr, pst, ptr = C.packet_results(rec)
    rng = np.random.RandomState(resx + len(lights_key))
    pick = rng.permutation(len(xy))[:(2 * len(xy)) // 3]
    set_arith(isc, arith)
    try:
        st = isc.new_stats()
        frame, trunc = ms.render_transparent(cam, resx, resy, lights, stats=st, max_depth=8)
        st2 = isc.new_stats()
        pk, trunc2 = ms.render_transparent_packets(cam, resx, resy, dev(torch, xy[pick]), lights, stats=st2, max_depth=8)
        pitch = resx * 3 + 20
        img, ist, itr = ms.render_transparent_image_host(cam, resx, resy, lights, pitch=pitch, fill=0x5a, max_depth=8)
        frame, pk = frame.cpu().numpy(), pk.cpu().numpy()
    finally:
        set_arith(isc, "ieee")
    what = "glasshouse %dx%d %s lights, %s" % (resx, resy, lights_key, arith)
    assert_frame(frame, want, st.cpu().numpy(), wst, what + ", _dev")
    assert int(trunc.cpu().numpy()[0]) == 0 == wtr
    assert_frame(img[:, :resx * 3].reshape(resy, resx, 3), want, ist, wst, what + ", _image")
    assert (img[:, resx * 3:] == 0x5a).all() and int(itr[0]) == 0
    # the packet list: a packet depends on no other (the rays of a partial packet that lie outside the frame are traced and shaded as the others)
    bad = (pk != pbgr[pick]).any(axis=2)
    print("%s, _packets_dev on %d of %d packets: %d differing pixels" % (what, len(pick), len(xy), int(bad.sum())))
    assert not bad.any()
    assert np.array_equal(st2.cpu().numpy().astype(np.uint64), pst[pick].sum(axis=0).astype(np.uint64)) and int(trunc2.cpu().numpy()[0]) == 0


@pytest.mark.parametrize("arith,mode", ARITH)
def test_the_truncated_counter_at_depth_2(torch_mod, arith, mode):
    isc, ms = device_set("glasshouse")
    name, resx, resy = STAGE
    cam = C.case(name)["cams"][resx]
    want, wst, wtr, d, xy, rec = C.reference(name, resx, resy, mode, "case", 2)
    set_arith(isc, arith)
    try:
        st = isc.new_stats()
        frame, trunc = ms.render_transparent(cam, resx, resy, C.lights_of(name, "case"), stats=st, max_depth=2)
        trunc = ms.render_transparent(cam, resx, resy, C.lights_of(name, "case"), max_depth=2, truncated=trunc)[1]      # (+=: twice the lanes)
        img, ist, itr = ms.render_transparent_image_host(cam, resx, resy, C.lights_of(name, "case"), max_depth=2, truncated=np.full(1, 7, np.uint64))
        frame = frame.cpu().numpy()
    finally:
        set_arith(isc, "ieee")
    assert_frame(frame, want, st.cpu().numpy(), wst, "depth 2, %s" % arith)
    assert int(trunc.cpu().numpy()[0]) == 2 * wtr and int(itr[0]) == 7 + wtr and wtr >= 16
    assert_frame(img.reshape(resy, resx, 3), want, ist, wst, "depth 2 _image, %s" % arith)


# ---- 8. invisible panes: independent of the restatement ----
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("resx,resy", C.FRAMES)
def test_invisible_panes_equal_the_existing_frame_without_them(torch_mod, resx, resy, arith, mode):
    isc, ms = device_set("invisible")
    isc0, ms0 = device_set("invisible", False, True, False)
    cam = C.case("invisible")["cams"][resx]
    assert ms.can_select_transparent is True and ms0.can_select_transparent is False
    set_arith(isc, arith)
    try:
        st, st0 = isc.new_stats(), isc0.new_stats()
        frame, trunc = ms.render_transparent(cam, resx, resy, None, stats=st, max_depth=8)
        plain = ms0.render(cam, resx, resy, None, stats=st0)
        frame, plain, st, st0 = frame.cpu().numpy(), plain.cpu().numpy(), st.cpu().numpy(), st0.cpu().numpy()
    finally:
        set_arith(isc, "ieee")
    bad = int((frame != plain).any(axis=2).sum())
    print("invisible %dx%d %s: %d differing pixels; stats %s / %s" % (resx, resy, arith, bad, st.tolist(), st0.tolist()))
    assert bad == 0 and int(trunc.cpu().numpy()[0]) == 0 and plain.any()
    assert (st[:3] > st0[:3]).all()      # (the panes were walked and continued through: the frames are equal because they do not show)


# ---- 9. a set without capable materials through the new frame functions ----
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("depth", [1, 8])
def test_a_set_without_capable_materials_renders_the_existing_frames(torch_mod, depth, arith, mode):
    torch = torch_mod
    name, resx, resy = "glasshouse", 70, 50
    isc, ms = device_set(name, True, True, False)
    cam = C.case(name)["cams"][resx]
    lights = C.lights_of(name, "case")
    xy = C.reference(name, resx, resy, mode)[4]
    set_arith(isc, arith)
    try:
        sa, sb, sc, sd = (isc.new_stats() for _ in range(4))
        new, trunc = ms.render_transparent(cam, resx, resy, lights, stats=sa, max_depth=depth)
        old = ms.render(cam, resx, resy, lights, stats=sb)
        dxy = dev(torch, xy[::2])
        newp, trunc = ms.render_transparent_packets(cam, resx, resy, dxy, lights, stats=sc, max_depth=depth, truncated=trunc)
        oldp = ms.render_packets(cam, resx, resy, dxy, lights, stats=sd)
        img, ist, itr = ms.render_transparent_image_host(cam, resx, resy, lights, max_depth=depth)
        oimg, oist = ms.render_image_host(cam, resx, resy, lights)
        new, old, newp, oldp = (x.cpu().numpy() for x in (new, old, newp, oldp))
    finally:
        set_arith(isc, "ieee")
    assert_frame(new, old, sa.cpu().numpy(), sb.cpu().numpy(), "no capable material, depth %d, %s, _dev" % (depth, arith))
    assert np.array_equal(newp, oldp) and np.array_equal(sc.cpu().numpy(), sd.cpu().numpy())
    assert np.array_equal(img, oimg) and np.array_equal(ist, oist) and int(itr[0]) == 0 and int(trunc.cpu().numpy()[0]) == 0 and old.any()


# ---- 10. the older entry points refuse a capable set ----
def test_older_entry_points_refuse_a_capable_set(torch_mod):
    torch = torch_mod
    name, resx, resy = STAGE
    isc, ms = device_set(name)
    cam = C.case(name)["cams"][resx]
    assert ms.can_select_transparent is True
    xy = dev(torch, C.reference(name, resx, resy)[4][:2])
    f = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda:0")        # noqa: E731
    i = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda:0")          # noqa: E731
    hits = (f(2, 256), f(2, 256), f(2, 256), i(2, 256), i(2, 256))
    calls = {
        "shade_packets": lambda: ms.shade_packets(cam, resx, resy, xy, hits),
        "mirror_packets": lambda: ms.mirror_packets(cam, resx, resy, xy, hits[0], f(2, 9, 64, 4)),
        "shade_rays": lambda: ms.shade_rays(f(2, 64, 3, 4), None, hits[0], f(2, 64, 2, 4), hits[3], hits[4]),
        "render": lambda: ms.render(cam, resx, resy),
        "render_packets": lambda: ms.render_packets(cam, resx, resy, xy),
        "render_image_host": lambda: ms.render_image_host(cam, resx, resy),
        "render reflections": lambda: ms.render(cam, resx, resy, reflections=True),
        "render_packets reflections": lambda: ms.render_packets(cam, resx, resy, xy, reflections=True),
        "render_image_host reflections": lambda: ms.render_image_host(cam, resx, resy, reflections=True),
    }
    for what, call in calls.items():
        with pytest.raises(_lib.SnailError) as e:
            call()
        assert "transparent" in str(e.value), (what, str(e.value))
    # ... and nothing was enqueued that breaks the set: it still renders
    frame, _ = ms.render_transparent(cam, resx, resy, C.lights_of(name, "case"))
    assert np.array_equal(frame.cpu().numpy(), C.reference(name, resx, resy)[0])


# ---- 11. the same set follows update and update_dev ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_the_same_set_follows_updates(torch_mod, arith, mode):
    torch = torch_mod
    resx, resy = 64, 48
    a, u = C.case("glasshouse"), C.case("moved")
    old = C.reference("glasshouse", resx, resy, mode)
    new = C.reference("moved", resx, resy, mode)
    assert (old[0] != new[0]).any(axis=2).sum() >= 100
    isc, ms = new_set("glasshouse")                                   # (a handle of this test's own: the cached one keeps its transforms)
    cam = a["cams"][resx]
    set_arith(isc, arith)
    try:
        def run(what, want):
            st = isc.new_stats()
            frame, trunc = ms.render_transparent(cam, resx, resy, a["lights"], stats=st)
            assert_frame(frame.cpu().numpy(), want[0], st.cpu().numpy(), want[1], "%s, %s" % (what, arith))
            assert int(trunc.cpu().numpy()[0]) == 0
        run("before the update", old)
        isc.update(u["rot"], u["tr"], u["bi"])
        check_tree(isc, u["ref"])
        run("after update", new)
        xf = np.concatenate([a["rot"].reshape(-1, 9), a["tr"].reshape(-1, 3)], axis=1).astype(np.float32)
        isc.update_dev(dev(torch, xf), dev(torch, a["bi"]))
        run("after update_dev", old)
        check_tree(isc, a["ref"])
    finally:
        set_arith(isc, "ieee")
        ms.close()
        isc.close()


# ---- 12. the DEEP instantiations ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_the_deep_case(torch_mod, arith, mode):
    isc, ms = device_set("deep")
    c = C.case("deep")
    want, wst, wtr, d, xy, rec = C.reference("deep", 64, 64, mode)
    set_arith(isc, arith)
    try:
        st = isc.new_stats()
        frame, trunc = ms.render_transparent(c["cams"][64], 64, 64, c["lights"], stats=st)
        frame = frame.cpu().numpy()
    finally:
        set_arith(isc, "ieee")
    assert_frame(frame, want, st.cpu().numpy(), wst, "deep, %s" % arith)
    assert int(trunc.cpu().numpy()[0]) == wtr == 0 and d.level_selected[1] >= 256 and d.lights[1].not_culled


# ---- 13. launches in flight: the groups are reused behind their events and grow ----
def test_nine_launches_on_two_streams_then_a_smaller_frame_then_a_deeper_one(torch_mod):
    torch = torch_mod
    isc, ms = new_set("glasshouse")
    c = C.case("glasshouse")
    lights = c["lights"]
    try:
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        outs = []
        for k in range(9):                                            # one more than the set has groups, depth 2 first: the levels' part is small
            s = streams[k % 2]
            st = isc.new_stats()
            with torch.cuda.stream(s):
                outs.append((ms.render_transparent(c["cams"][70], 70, 50, lights, stats=st, stream=s, max_depth=2), st))
        small = ms.render_transparent(c["cams"][64], 64, 48, lights, max_depth=2)
        deeper = ms.render_transparent(c["cams"][96], 96, 64, lights, max_depth=8)      # more packets AND more levels: every part grows
        again = ms.render_transparent(c["cams"][70], 70, 50, lights, max_depth=2)
        torch.cuda.synchronize()
        w2 = C.reference("glasshouse", 70, 50, max_depth=2)
        for k, ((frame, trunc), st) in enumerate(outs):
            assert_frame(frame.cpu().numpy(), w2[0], st.cpu().numpy(), w2[1], "launch %d of nine" % k)
            assert int(trunc.cpu().numpy()[0]) == w2[2]
        assert np.array_equal(small[0].cpu().numpy(), C.reference("glasshouse", 64, 48, max_depth=2)[0])
        assert np.array_equal(deeper[0].cpu().numpy(), C.reference("glasshouse", 96, 64)[0]) and int(deeper[1].cpu().numpy()[0]) == 0
        assert np.array_equal(again[0].cpu().numpy(), w2[0])
    finally:
        ms.close()
        isc.close()
