"""The one mirrored bounce under full shading of instanced scenes on the MI355X (include/snail_instances_materials_bounce.h;
InstancedMaterialSet.mirror_packets / .shade_rays and reflections=True): the mirror stage, the mirrored packets' walk, the sample stage on
generic packets -- k_imat_sample_rays -- and the frames, bit for bit, byte for byte and TreeStats for equality against the test-side
restatement tests/instances_materials_bounce_ref.py, in both arithmetics; and, independent of that restatement, the degenerate set against
the simple-shading bounce of InstancedScene.render_whitted, and k_imat_sample_rays against itself on synthetic records.  The cases
(tests/instances_materials_bounce_cases.py) were chosen with the restatement alone; what they must exercise is asserted on its counters
without a GPU by tests/test_instances_materials_bounce_host.py.  Nothing here reads outside the repository."""
import functools

import numpy as np
import pytest

from snail_amd import HostBVH, _lib
from snail_amd import instances_materials as IP
from snail_amd import materials as P
from snail_amd.instances import InstancedScene
from snail_amd.scene import Context, Scene, _stream_ptr
from tests import instances_materials_bounce_cases as BK
from tests import instances_materials_bounce_ref as IB
from tests import instances_materials_cases as K
from tests import instances_materials_synth as Z
from tests import materials_synth as Y
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu
ARITH = [("ieee", O.MODE_IEEE), ("host_sse", O.MODE_SSE)]
INF = np.float32(np.inf)
PLANES = ["normal x", "normal y", "normal z", "diffuse r", "diffuse g", "diffuse b", "specular r", "specular g", "specular b"]


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


def product_materials(descs=None, textures=None):
    mats = [P.Material.simple(d[1], d[2]) if d[0] == "simple" else P.Material.textured(d[1], d[2]) if d[0] == "tex" else P.Material.uber(d[1], d[2], d[3])
            for d in (descs if descs is not None else K.DESCS)]
    return mats, [P.Texture(t) for t in (textures if textures is not None else K.TEXTURES())]


def check_tree(isc, ref):
    xs, bs = isc.slot_transforms()
    assert isc.nodes().tobytes() == ref.nodes.tobytes() and np.array_equal(xs, ref.xf) and np.array_equal(bs, ref.bi)


def new_set(name):
    c = BK.case(name)
    keys = ["chain"] if name == "deep" else ["sheet", "box"][:len(c["tvs"])]
    scs = [blas_scene(k, tv, osc) for k, tv, osc in zip(keys, c["tvs"], c["oscs"])]
    isc = InstancedScene(scs, c["rot"], c["tr"], c["bi"])
    check_tree(isc, c["ref"])
    mats, texs = product_materials()
    return isc, IP.InstancedMaterialSet(isc, c["per_blas"], mats, texs)


def device_set(name):
    """(InstancedScene, InstancedMaterialSet) of a case, built once; the handle's tree and records are the case's own (built without a GPU)"""
    if name not in _sets:
        _sets[name] = new_set(name)
    return _sets[name]


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


def mirrored_of(inter):
    """the restatement's mirrored packets of a frame as arrays in the device's layouts"""
    n = len(inter)
    g = lambda k, shape: IB.stack(inter, "mirrored", k).reshape(shape)      # noqa: E731
    return dict(origin=g("origin", (n, 64, 3, 4)), dir=g("dir", (n, 64, 3, 4)), idir=g("idir", (n, 64, 3, 4)), mask=g("mask", (n, 64)),
                distance=g("distance", (n, 256)), object=g("object", (n, 256)), element=g("element", (n, 256)), bary=g("bary", (n, 64, 2, 4)))


def nested_of(inter):
    n = len(inter)
    g = lambda k, shape: IB.stack(inter, "nested", k).reshape(shape)        # noqa: E731
    return dict(t=g("t", (n, 256)), inst=g("inst", (n, 256)), tri_id=g("tri_id", (n, 256)), bary=g("bary", (n, 64, 2, 4)), samples=g("samples", (n, 9, 64, 4)))


def walk(torch, isc, m, stats=None):
    """the device's walk of mirrored packets given as device tensors (origin, dir, idir, mask, distance, object, element, bary): in place"""
    org, d, idir, mask, dist, obj, elem, bary = m
    n = d.shape[0]
    ctx = Context(origin=org.view(n * 64, 12), dir=d.view(n * 64, 12), idir=idir.view(n * 64, 12), distance=dist.view(n * 64, 4), object=obj.view(n * 64, 4),
                  barycentric=bary.view(n * 64, 8), size=64, shared_origin=False, mask=mask.view(n * 64))
    isc.traverse_primary(ctx, elem, stats=stats)
    return dist, obj, elem, bary


STAGE_CASES = [("main", 96, 64), ("mirror", 70, 50)]


# ---- 1. the mirror stage ----
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("name,resx,resy", STAGE_CASES)
def test_mirror_stage_equals_the_restatement(torch_mod, name, resx, resy, arith, mode):
    torch = torch_mod
    isc, ms = device_set(name)
    cam = BK.case(name)["cams"][resx]
    _, _, inter, xy, d = BK.reference(name, resx, resy, mode)
    want = mirrored_of(inter)
    set_arith(isc, arith)
    try:
        dxy = dev(torch, xy)
        hits = isc.trace_packets(cam, resx, resy, dxy)
        smp = ms.shade_packets(cam, resx, resy, dxy, hits)
        st = isc.new_stats()
        got = ms.mirror_packets(cam, resx, resy, dxy, hits[0], smp, stats=st)
        got = [g.cpu().numpy() for g in got]
    finally:
        set_arith(isc, "ieee")
    assert_bits("primary samples", smp.cpu().numpy(), IB.stack(inter, "samples"))
    for g, k in zip(got, ("origin", "dir", "idir", "mask", "distance", "object", "element", "bary")):
        assert_bits("mirrored %s, %s %dx%d %s" % (k, name, resx, resy, arith), g, want[k])
    assert not got[5].any() and not got[6].any() and not got[7].view(np.uint32).any()
    assert st.cpu().numpy().tolist() == [0, 0, d.mirrored_lanes, 0] and d.mirrored_lanes >= 256
    # masked lanes carry zeros everywhere and -inf; selected lanes inf
    sel = ((got[3].reshape(-1, 64, 1) >> np.arange(4).reshape(1, 1, 4)) & 1).astype(bool)
    assert (got[4].reshape(-1, 64, 4)[sel] == INF).all() and (got[4].reshape(-1, 64, 4)[~sel] == -INF).all() and sel.any() and (~sel).any()
    for k in range(2):
        assert not got[k].transpose(0, 1, 3, 2)[~sel].view(np.uint32).any()


# ---- 2. the device's own mirrored packets through the walk ----
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("name,resx,resy", STAGE_CASES)
def test_the_devices_mirrored_packets_walk_to_the_restatements_nested_hits(torch_mod, name, resx, resy, arith, mode):
    torch = torch_mod
    isc, ms = device_set(name)
    cam = BK.case(name)["cams"][resx]
    _, _, inter, xy, d = BK.reference(name, resx, resy, mode)
    want = nested_of(inter)
    set_arith(isc, arith)
    try:
        dxy = dev(torch, xy)
        hits = isc.trace_packets(cam, resx, resy, dxy)
        m = ms.mirror_packets(cam, resx, resy, dxy, hits[0], ms.shade_packets(cam, resx, resy, dxy, hits))
        dist, obj, elem, bary = (x.cpu().numpy() for x in walk(torch, isc, m))
    finally:
        set_arith(isc, "ieee")
    for g, k in ((dist, "t"), (obj, "inst"), (elem, "tri_id"), (bary, "bary")):
        assert_bits("nested %s, %s %dx%d %s" % (k, name, resx, resy, arith), g, want[k])
    assert d.mirrored_hits >= 256 and len({int(s) for s in np.unique(obj[np.isfinite(dist)])}) >= 2


# ---- 3. the sample stage on generic packets ----
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("name,resx,resy", STAGE_CASES + [("quirk", 48, 32)])
def test_shade_rays_equals_the_restatements_nested_samples(torch_mod, name, resx, resy, arith, mode):
    torch = torch_mod
    isc, ms = device_set(name)
    _, _, inter, _, d = BK.reference(name, resx, resy, mode)
    mp, nst = mirrored_of(inter), nested_of(inter)
    args = [dev(torch, a) for a in (mp["dir"], mp["mask"], nst["t"], nst["bary"], nst["inst"], nst["tri_id"])]
    unmasked = np.flatnonzero((mp["mask"] == 15).all(axis=1))
    set_arith(isc, arith)
    try:
        got = ms.shade_rays(*args).cpu().numpy()
        again = None
        if len(unmasked):      # the unmasked packets once more with d_mask = NULL
            sub = [a[torch.from_numpy(unmasked).to("cuda:0")].contiguous() for a in args]
            again = ms.shade_rays(sub[0], None, *sub[2:]).cpu().numpy()
    finally:
        set_arith(isc, "ieee")
    ne = bits(got) != bits(nst["samples"])
    print("%s %dx%d %s: nested samples differing per plane %s" % (name, resx, resy, arith, {PLANES[c]: int(ne[:, c].sum()) for c in range(9) if ne[:, c].any()}))
    assert_bits("nested samples, %s %dx%d %s" % (name, resx, resy, arith), got, nst["samples"])
    if name != "quirk":
        assert len(unmasked) >= 4 and d.packets_masked >= 8
        assert_bits("unmasked packets with a NULL mask", again, nst["samples"][unmasked])
    if name == "mirror":
        assert d.nested.quirk_lanes >= 1 and d.a_uber_unmasked >= 8


# ---- 4. frames ----
def raw_bounce_dev(ms, cam, resx, resy, lights7, flags, out, stats):
    """snail_instances_materials_bounce_dev with the flags given (InstancedMaterialSet.render never passes 0 to it)"""
    lights, cam13, amb = ms._frame_args(cam, lights7, (0.1, 0.1, 0.1))
    rc = _lib.lib().snail_instances_materials_bounce_dev(ms._h, _lib.ptr(cam13), resx, resy, _lib.ptr(lights) if len(lights) else None, len(lights), _lib.ptr(amb), flags,
                                                         _lib.ptr(out), int(out.stride(0)), _lib.ptr(stats), _stream_ptr(None))
    _lib.check(rc, "snail_instances_materials_bounce_dev")
    return out


def sublist_reference(name, resx, resy, mode, lights_key):
    """a shuffled two thirds of the frame's packets -> (list, bytes, TreeStats): every packet's own bytes and counters, as the restatement
    booked them while it rendered the frame (a packet depends on no other)"""
    inter, xy = BK.reference(name, resx, resy, mode, lights_key)[2:4]
    pick = np.random.RandomState(len(xy)).permutation(len(xy))[:(2 * len(xy)) // 3]
    return np.ascontiguousarray(np.array(xy)[pick]), np.stack([inter[p]["bgr"] for p in pick]), np.sum([inter[p]["stats"] for p in pick], axis=0).astype(np.uint64)


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("name,resx,resy,lights_key", [("main", 96, 64, "case"), ("main", 70, 50, "case"), ("main", 70, 50, "none"), ("main", 64, 48, "eight"),
                                                       ("mirror", 96, 64, "case")])
def test_frames_equal_the_restatement(torch_mod, name, resx, resy, lights_key, arith, mode):
    torch = torch_mod
    isc, ms = device_set(name)
    cam, lights = BK.case(name)["cams"][resx], BK.lights_of(name, lights_key)
    want, wst, _, _, d = BK.reference(name, resx, resy, mode, lights_key)
    sub, pw, pst = sublist_reference(name, resx, resy, mode, lights_key)
    what = "%s %dx%d %s lights %s" % (name, resx, resy, lights_key, arith)
    set_arith(isc, arith)
    try:
        st = isc.new_stats()
        frame = ms.render(cam, resx, resy, lights, stats=st, reflections=True).cpu().numpy()
        assert_frame(frame, want, st.cpu().numpy(), wst, "_dev " + what)
        st = isc.new_stats()
        got = ms.render_packets(cam, resx, resy, dev(torch, sub), lights, stats=st, reflections=True).cpu().numpy()
        assert np.array_equal(got, pw) and np.array_equal(st.cpu().numpy().astype(np.uint64), pst), ("_packets_dev " + what, st, pst)
        # the host image, with a pitch of its own: the bytes past a row's pixels stay
        img, ist = ms.render_image_host(cam, resx, resy, lights, pitch=resx * 3 + 5, fill=0xCD, reflections=True)
        assert_frame(img[:, :resx * 3].reshape(resy, resx, 3), want, ist, wst, "_image " + what)
        assert (img[:, resx * 3:] == 0xCD).all()
        # flags = 0 through the new function: the existing function's frame and TreeStats
        s0, s1 = isc.new_stats(), isc.new_stats()
        old = ms.render(cam, resx, resy, lights, stats=s0).cpu().numpy()
        new = raw_bounce_dev(ms, cam, resx, resy, lights, 0, torch.zeros((resy, resx, 3), dtype=torch.uint8, device="cuda:0"), s1).cpu().numpy()
        assert_frame(new, old, s1.cpu().numpy(), s0.cpu().numpy(), "flags 0 " + what)
        assert (old != frame).any()
    finally:
        set_arith(isc, "ieee")
    if lights_key == "none":
        assert d.nested.lit_pixels == 0 and d.primary.lit_pixels == 0 and d.mirrored_hits >= 256
    elif lights_key == "eight":
        assert len({n for _, n in d.nested.not_culled}) == 8 and d.nested.lit_pixels >= 100
    elif name == "main":
        assert d.nested.culled and d.nested.not_culled and d.nested.occluded_pixels >= 64


# ---- 5. independent of the restatement: the degenerate set ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_degenerate_set_equals_the_simple_shading_bounce(torch_mod, arith, mode):
    isc, ms = device_set("degenerate")
    c = BK.case("degenerate")
    set_arith(isc, arith)
    try:
        for resx, resy in BK.FRAMES:
            st0, st1, st2 = isc.new_stats(), isc.new_stats(), isc.new_stats()
            want = isc.render_whitted(c["cams"][resx], resx, resy, c["lights"], color=(1.0, 1.0, 1.0), stats=st0, reflections=True).cpu().numpy()
            plain = isc.render_whitted(c["cams"][resx], resx, resy, c["lights"], color=(1.0, 1.0, 1.0), stats=st2).cpu().numpy()
            got = ms.render(c["cams"][resx], resx, resy, c["lights"], stats=st1, reflections=True).cpu().numpy()
            assert (want != plain).any() and len(np.unique(want.reshape(-1, 3), axis=0)) > 16
            assert_frame(got, want, st1.cpu().numpy(), st0.cpu().numpy(), "degenerate %dx%d %s" % (resx, resy, arith))
    finally:
        set_arith(isc, "ieee")


# ---- 6. updates: the kernels read the instance records at launch ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_the_same_set_follows_updates(torch_mod, arith, mode):
    torch = torch_mod
    c, u = BK.case("main"), BK.case("updated")
    isc, ms = new_set("main")          # (a scene of this test's own: the cached one keeps its transforms)
    resx, resy = 96, 64
    cam = c["cams"][resx]
    old, ost = BK.reference("main", resx, resy, mode)[:2]
    new, nst = BK.reference("updated", resx, resy, mode)[:2]
    assert int((old != new).any(axis=2).sum()) >= 500
    render = lambda st: ms.render(cam, resx, resy, c["lights"], stats=st, reflections=True).cpu().numpy()      # noqa: E731
    set_arith(isc, arith)
    try:
        st = isc.new_stats()
        assert_frame(render(st), old, st.cpu().numpy(), ost, "before the update")
        isc.update(u["rot"], u["tr"], u["bi"])
        check_tree(isc, u["ref"])
        st = isc.new_stats()
        assert_frame(render(st), new, st.cpu().numpy(), nst, "after update")
        xf = np.concatenate([c["rot"].reshape(-1, 9), c["tr"]], axis=1).astype(np.float32)
        isc.update_dev(torch.from_numpy(xf).to("cuda:0"), torch.from_numpy(np.ascontiguousarray(c["bi"], dtype=np.int32)).to("cuda:0"))
        st = isc.new_stats()
        frame = render(st)
        check_tree(isc, c["ref"])
        assert_frame(frame, old, st.cpu().numpy(), ost, "after update_dev")
    finally:
        set_arith(isc, "ieee")
        ms.close()
        isc.close()


# ---- 7. a DEEP BLAS: the DEEP instantiations of the mirrored walk and of k_imat_light_rays ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_deep_blas_under_one_light(torch_mod, arith, mode):
    isc, ms = device_set("deep")
    c = BK.case("deep")
    assert c["oscs"][0].depth > 62 and len(c["lights"]) == 1
    resx, resy = 64, 64
    want, wst, _, _, d = BK.reference("deep", resx, resy, mode)
    set_arith(isc, arith)
    try:
        st = isc.new_stats()
        frame = ms.render(c["cams"][64], resx, resy, c["lights"], stats=st, reflections=True).cpu().numpy()
    finally:
        set_arith(isc, "ieee")
    assert_frame(frame, want, st.cpu().numpy(), wst, "deep %s" % arith)
    assert d.mirrored_hits >= 16 and d.nested.lit_pixels >= 8 and d.nested.not_culled


# ---- 8. launches in flight, and set growth ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_nine_launches_on_two_streams_then_a_smaller_and_a_larger_frame(torch_mod, arith, mode):
    """nine launches without a host wait between them (more than the set's 8 groups of intermediates: the ninth reuses the first's, behind
    its event), alternating between two streams; then a smaller frame (the groups are large enough), then a larger one (they grow)"""
    torch = torch_mod
    isc, ms = new_set("main")          # (a set of this test's own: its groups start empty)
    c = BK.case("main")
    want70, st70 = BK.reference("main", 70, 50, mode)[:2]
    want96, st96 = BK.reference("main", 96, 64, mode)[:2]
    want64, st64 = BK.reference("main", 64, 48, mode)[:2]
    streams = [torch.cuda.Stream(device="cuda:0") for _ in range(2)]
    set_arith(isc, arith)
    try:
        frames, stats = [], []
        for k in range(9):
            s = streams[k & 1]
            with torch.cuda.stream(s):
                stats.append(isc.new_stats())
                frames.append(ms.render(c["cams"][70], 70, 50, c["lights"], stats=stats[-1], stream=s, reflections=True))
        for s in streams:
            s.synchronize()
        for k in range(9):
            assert_frame(frames[k].cpu().numpy(), want70, stats[k].cpu().numpy(), st70, "launch %d of nine, %s" % (k, arith))
        st = isc.new_stats()
        small = ms.render(c["cams"][64], 64, 48, c["lights"], stats=st, reflections=True).cpu().numpy()      # 12 packets: the group is large enough
        assert_frame(small, want64, st.cpu().numpy(), st64, "the smaller frame, %s" % arith)
        st = isc.new_stats()
        large = ms.render(c["cams"][96], 96, 64, c["lights"], stats=st, reflections=True).cpu().numpy()      # 24 packets: the group grows
        assert_frame(large, want96, st.cpu().numpy(), st96, "the larger frame, %s" % arith)
        st = isc.new_stats()
        again = ms.render(c["cams"][70], 70, 50, c["lights"], stats=st, reflections=True).cpu().numpy()
        assert_frame(again, want70, st.cpu().numpy(), st70, "after the growth, %s" % arith)
    finally:
        set_arith(isc, "ieee")
        ms.close()
        isc.close()


# ---- 9. k_imat_sample_rays on synthetic records ----
@functools.lru_cache(maxsize=None)
def synth_blas_scenes():
    out = []
    for b in Z.blases():
        hb = HostBVH.build(b.tv)
        assert np.array_equal(hb.perm, b.osc.perm) and hb.nodes.tobytes() == b.osc.nodes.tobytes()
        out.append(Scene(hb, 0))
    return out


@functools.lru_cache(maxsize=None)
def synth_set():
    a = Z.arrangement()
    isc = InstancedScene(synth_blas_scenes(), a.rot, a.tr, a.bi_input)
    check_tree(isc, a.ref)
    mats, texs = product_materials(Y.material_descs(), Y.synth().textures)
    return isc, IP.InstancedMaterialSet(isc, [b.per_blas for b in Z.blases()], mats, texs)


@functools.lru_cache(maxsize=None)
def synth_inputs():
    """the generator's 48-packet list as NESTED hit records: seeded finite directions, and a seeded mask -- a third of the packets all
    selected, the rest with quads of every lane pattern, whole blocks among them selected so that branch (a) meets masked packets"""
    r = Z.records()
    n = len(r["t"])
    rng = np.random.RandomState(77)
    dirs = (rng.rand(n, 64, 3, 4).astype(np.float32) * np.float32(2.0) - np.float32(1.0))
    dirs = (dirs / np.sqrt((dirs.astype(np.float64) ** 2).sum(axis=2, keepdims=True))).astype(np.float32)
    mask = rng.randint(0, 16, size=(n, 64)).astype(np.uint8)
    full_blocks = rng.rand(n, 16) < 0.6
    mask = np.where(np.repeat(full_blocks, 4, axis=1), np.uint8(15), mask).astype(np.uint8)
    mask[::3] = 15
    mask[1::3, 0] &= 14          # (a packet of the masked kind stays masked whatever the draw)
    for a in (dirs, mask):
        a.setflags(write=False)
    return dirs, mask


def synth_expected(recs, dirs, mask):
    """the restatement's nested samples of a record list (the records through the generator's clamp rule first) -> ([n,9,64,4], counters)"""
    ref = IB.InstBounceRef(Z.reference())
    d = IB.BounceDiag()
    n = len(recs["t"])
    out = np.zeros((n, 9, 64, 4), dtype=np.float32)
    for p in range(n):
        s, key_tri, _ = Z.clamp_records(recs["slot"][p], recs["tri"][p])
        sel = ((mask[p].reshape(64, 1).astype(np.int32) >> np.arange(4).reshape(1, 4)) & 1).astype(bool)
        _, nrm, diff, spec = ref.samples_rays(dirs[p], recs["t"][p], s, key_tri, recs["bary"][p], sel, d)
        out[p] = Y.to_planes(nrm, diff, spec)
    return out, d


def synth_shade(torch, ms, recs, dirs, mask):
    n = len(recs["t"])
    return ms.shade_rays(dev(torch, dirs), None if mask is None else dev(torch, mask), dev(torch, recs["t"].reshape(n, 256)), dev(torch, recs["bary"].reshape(n, 64, 2, 4)),
                         dev(torch, recs["slot"].reshape(n, 256)), dev(torch, recs["tri"].reshape(n, 256))).cpu().numpy()


@pytest.mark.parametrize("arith,mode", ARITH)
def test_synthetic_records_equal_the_restatement(torch_mod, arith, mode):
    isc, ms = synth_set()
    r = Z.records()
    dirs, mask = synth_inputs()
    want, d = synth_expected(r, dirs, mask)
    set_arith(isc, arith)
    try:
        got = synth_shade(torch_mod, ms, r, dirs, mask)
    finally:
        set_arith(isc, "ieee")
    ne = bits(got) != bits(want)
    print("synthetic records %s: differing per plane %s; a masked/unmasked %d/%d, uber %d/%d, b %d, c %d, quirk %d" % (
        arith, {PLANES[c]: int(ne[:, c].sum()) for c in range(9) if ne[:, c].any()}, d.a_masked, d.a_unmasked, d.a_uber_masked, d.a_uber_unmasked, d.nested.blocks_b,
        d.nested.blocks_c, d.nested.quirk_lanes))
    assert_bits("synthetic records, %s" % arith, got, want)
    assert min(d.a_masked, d.a_unmasked, d.a_uber_masked, d.a_uber_unmasked, d.nested.blocks_b, d.nested.blocks_c, d.nested.quirk_lanes, d.multi_slot_blocks) >= 1, vars(d)
    assert ((mask != 15).any(axis=1)).sum() >= 16 and ((mask == 15).all(axis=1)).sum() >= 16 and got.any()


@pytest.mark.parametrize("arith,mode", ARITH)
def test_synthetic_records_device_against_device(torch_mod, arith, mode):
    """no restatement: an all-15 mask equals NULL; the t, slot, triId and bary of MASKED lanes overwritten with other finite values inside
    the scene change no output bit"""
    torch = torch_mod
    isc, ms = synth_set()
    r = Z.records()
    dirs, mask = synth_inputs()
    n = len(r["t"])
    a = Z.arrangement()
    sel = ((mask.reshape(n, 64, 1).astype(np.int32) >> np.arange(4).reshape(1, 1, 4)) & 1).astype(bool)
    rng = np.random.RandomState(5)
    slot2 = rng.randint(0, a.n, size=(n, 64, 4)).astype(np.int32)
    other = dict(t=np.where(sel, r["t"], (rng.rand(n, 64, 4) * 9.0 + 0.5).astype(np.float32)).astype(np.float32),
                 slot=np.where(sel, r["slot"], slot2).astype(np.int32),
                 tri=np.where(sel, r["tri"], (rng.randint(0, 1 << 20, size=(n, 64, 4)) % a.n_tris[slot2]).astype(np.int32)).astype(np.int32),
                 bary=np.where(np.concatenate([sel, sel], axis=2), r["bary"], (rng.rand(n, 64, 8) * 0.5).astype(np.float32)).astype(np.float32))
    changed = (bits(other["t"]) != bits(r["t"])) | (other["slot"] != r["slot"]) | (other["tri"] != r["tri"])
    assert changed[~sel].mean() > 0.9 and not changed[sel].any() and (~sel).sum() >= 1000
    ones = np.full((n, 64), 15, dtype=np.uint8)
    set_arith(isc, arith)
    try:
        all15, null = synth_shade(torch, ms, r, dirs, ones), synth_shade(torch, ms, r, dirs, None)
        base, over = synth_shade(torch, ms, r, dirs, mask), synth_shade(torch, ms, other, dirs, mask)
    finally:
        set_arith(isc, "ieee")
    assert_bits("an all-15 mask against NULL, %s" % arith, all15, null)
    assert_bits("masked lanes overwritten, %s" % arith, over, base)
    assert base.any() and not np.array_equal(bits(base), bits(all15))
    # a masked lane's nine planes are zero
    assert not base.transpose(0, 2, 3, 1)[~sel].view(np.uint32).any()
