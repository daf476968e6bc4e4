"""The sample and mirror stages of full shading on the MI355X -- k_mat_sample, its twin k_mat_sample_rays and k_mat_mirror
(snail_amd/csrc/materials.inc) -- on the SYNTHETIC hit records of tests/materials_synth.py, bit for bit against the restatements
(MaterialsRef.samples, BounceRef.samples_rays, BounceRef.mirror) in both arithmetics.  Every other GPU test of these kernels feeds them what a
traversal of four procedural scenes produced, with two textures and texture coordinates in [-3, 3]; here they meet textures with a side of 1,
taller than wide, 8192 wide and 8192 tall (TexRec::lvl[13]), ten textures in one set, coordinates on integers, a few ulps beside them and next
to +-2^20, every mip level up to the clamp, blocks of every branch built on purpose, ids outside the scene, and normals of length 0, 1e-20 and
1e3.  Independent of the restatements: the twins against each other, a constant-grey set whose samples are known in closed form, and
dyadic triangles against their integer-shifted partners.  What the lists must exercise is asserted on the restatements' diagnostics here and,
without a GPU, by tests/test_materials_synth_host.py.  Nothing here reads outside the repository.

Left out: a texDiff product at or above 2^32 (the low-word truncation of uint(float)): it needs a texture of 4096 x 4096 or more, 50 MB or more."""
import functools

import numpy as np
import pytest

from snail_amd import HostBVH
from snail_amd import materials as P
from snail_amd.scene import Scene
from tests import materials_bounce_ref as B
from tests import materials_ref as M
from tests import materials_synth as Y
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu
ARITH = [("ieee", O.MODE_IEEE), ("host_sse", O.MODE_SSE)]
INF = np.float32(np.inf)
RESX, RESY = Y.FRAME
CAM = Y.Cam()
PLANES = ["normal x", "normal y", "normal z", "diffuse r", "diffuse g", "diffuse b", "specular r", "specular g", "specular b"]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def product_materials(descs):
    return [P.Material.simple(d[1], d[2]) if d[0] == "simple" else P.Material.textured(d[1], d[2]) if d[0] == "tex" else P.Material.uber(d[1], d[2], d[3]) for d in descs]


@functools.lru_cache(maxsize=None)
def device_sets():
    """(Scene, the noise set, the grey set) over the synthetic triangles, built once; the product builder's tree is the oracle's, so the
    generator's triIds are the product's"""
    s = Y.synth()
    hb = HostBVH.build(s.tv)
    assert np.array_equal(hb.perm, s.osc.perm) and hb.nodes.tobytes() == s.osc.nodes.tobytes()
    sc = Scene(hb, 0)
    noise = P.MaterialSet(sc, s.uv, s.nrm, s.mat_index, s.flat, s.material_map, product_materials(s.descs), [P.Texture(t) for t in s.textures])
    grey = P.MaterialSet(sc, s.uv, s.nrm, s.mat_index, s.flat, s.material_map, product_materials(s.descs_grey), [P.Texture(t) for t in s.textures_grey])
    return sc, noise, grey


@functools.lru_cache(maxsize=None)
def records(generic):
    """the list's packets as the arrays the calls take: t, u, v, tri [n,256]; dirs [n,64,3,4], mask bytes [n,64], bits [n,64,4] (generic)"""
    s = Y.synth()
    pk = [s.packet(p, generic) for p in range(Y.N_PACKETS)]
    return stack_packets(pk, generic)


def stack_packets(pk, generic):
    n = len(pk)
    out = dict(t=np.stack([p["t"] for p in pk]).reshape(n, 256), tri=np.stack([p["tri"] for p in pk]).reshape(n, 256),
               u=np.stack([p["bary"][:, 0:4] for p in pk]).reshape(n, 256), v=np.stack([p["bary"][:, 4:8] for p in pk]).reshape(n, 256))
    if generic:
        out["dirs"] = np.stack([p["dirs"] for p in pk])
        out["bits"] = np.stack([p["bits"] for p in pk])
        out["mask"] = (out["bits"].astype(np.uint8) << np.arange(4, dtype=np.uint8).reshape(1, 1, 4)).sum(axis=2).astype(np.uint8)
    return {k: np.ascontiguousarray(a) for k, a in out.items()}


def dev(torch, a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")      # (a copy: the shared inputs are read-only)


def shade_packets(torch, ms, r, xy):
    return ms.shade_packets(CAM, RESX, RESY, dev(torch, xy), (dev(torch, r["t"]), dev(torch, r["u"]), dev(torch, r["v"]), dev(torch, r["tri"]))).cpu().numpy()


def shade_rays(torch, ms, r, dirs, mask, pick=None):
    sel = (lambda a: a) if pick is None else (lambda a: a[pick])
    return ms.shade_rays(dev(torch, sel(dirs)), None if mask is None else dev(torch, sel(mask)), dev(torch, sel(r["t"])), dev(torch, sel(r["u"])), dev(torch, sel(r["v"])),
                         dev(torch, sel(r["tri"]))).cpu().numpy()


def compare_planes(what, got, want):
    """all nine planes by bit pattern; prints the number of differing words per plane before it asserts"""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (got.shape, want.shape)
    ne = np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)
    print("%s: %d differing words of %d; per plane %s" % (what, int(ne.sum()), ne.size, {PLANES[c]: int(ne[:, c].sum()) for c in range(9) if ne[:, c].any()}))
    if ne.any():
        at = tuple(np.argwhere(ne)[0])
        raise AssertionError("%s: %d words differ; first at (packet, plane, quad, lane) %s: %r / %r; packets %s" % (
            what, int(ne.sum()), at, got[at], want[at], sorted(set(np.argwhere(ne)[:, 0].tolist()))[:16]))


def primary_dirs(mode):
    xy = Y.synth().packet_xy()
    return np.ascontiguousarray(np.stack([Y.primary_dirs(int(x), int(y), mode) for x, y in xy.tolist()]))


# ---- 1. the primary sample stage ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_primary_sample_stage_on_synthetic_records(torch_mod, arith, mode):
    sc, ms, _ = device_sets()
    want, d = Y.expected_primary(mode)
    sc.set_arith(arith)
    try:
        got = shade_packets(torch_mod, ms, records(False), Y.synth().packet_xy())
    finally:
        sc.set_arith("ieee")
    print(Y.describe(d))
    compare_planes("primary list, %s" % arith, got, want)
    Y.check_conditions(d)


# ---- 2. the sample stage on generic packets ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_generic_sample_stage_on_synthetic_records(torch_mod, arith, mode):
    """the caller's directions and masks; the packets whose lanes are all selected once more without a mask array"""
    sc, ms, _ = device_sets()
    want, bd = Y.expected_generic()
    r = records(True)
    full = np.flatnonzero((r["mask"] == 15).all(axis=1))
    sc.set_arith(arith)
    try:
        got = shade_rays(torch_mod, ms, r, r["dirs"], r["mask"])
        got_full = shade_rays(torch_mod, ms, r, r["dirs"], None, full)
    finally:
        sc.set_arith("ieee")
    print(Y.describe(bd.nested, bd))
    compare_planes("generic list, %s" % arith, got, want)
    compare_planes("generic list, the %d all-selected packets without a mask array, %s" % (len(full), arith), got_full, want[full])
    Y.check_conditions(bd.nested, bd)
    assert 8 <= len(full) <= Y.N_PACKETS - 8                         # hasMask takes both values


# ---- 3. the twins, directly ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_the_twin_kernels_agree_on_the_primary_list(torch_mod, arith, mode):
    """k_mat_sample_rays on the primary list's records with the directions the generator produces for them and no mask is k_mat_sample:
    device against device, no restatement involved"""
    sc, ms, _ = device_sets()
    r = records(False)
    sc.set_arith(arith)
    try:
        a = shade_packets(torch_mod, ms, r, Y.synth().packet_xy())
        b = shade_rays(torch_mod, ms, r, primary_dirs(mode), None)
    finally:
        sc.set_arith("ieee")
    compare_planes("twins, %s" % arith, b, a)
    assert a[:, 3:].any() and a[:, 0:3].any()


# ---- 4. independent of the restatement ----
def lane_materials(r, bits=None):
    """the material of every hit lane, from the records alone: the map entry of the (clamped) triangle -- except a lane that hit triangle 0
    beside a lane 0 that missed, which keeps the default (-1).  -> (material int64 [n,64,4], -2 where the lane did not hit)"""
    s = Y.synth()
    n = len(r["t"])
    t = r["t"].reshape(n, 64, 4)
    hit = (t < INF) if bits is None else ((t < INF) & bits)
    tri = Y.clamp_ids(r["tri"], s.n).reshape(n, 64, 4)
    mat = np.asarray(Y.MAP, dtype=np.int64)[s.mat_index[s.input_of[tri]]]
    mat = np.where(~hit[:, :, 0:1] & (tri == 0), -1, mat)
    return np.where(hit, mat, -2)


@pytest.mark.parametrize("arith,mode", ARITH)
def test_grey_textures_sample_to_their_grey(torch_mod, arith, mode):
    """the constant-grey set, every TEX material without N.R: a hit lane of TEX material k has diffuse = specular = float32(g_k) * (1 / 255)
    exactly, whatever its coordinates, level and taps -- g_k names the texture, so a tap that strays into a neighbour's bytes, into the
    padding or past the chain shows"""
    sc, _, grey = device_sets()
    s = Y.synth()
    rp, rg = records(False), records(True)
    sc.set_arith(arith)
    try:
        got = [("primary", shade_packets(torch_mod, grey, rp, s.packet_xy()), lane_materials(rp)),
               ("generic", shade_rays(torch_mod, grey, rg, rg["dirs"], rg["mask"]), lane_materials(rg, rg["bits"]))]
    finally:
        sc.set_arith("ieee")
    for what, smp, mat in got:
        for k, g in enumerate(Y.GREYS):
            want = np.float32(g) * (np.float32(1.0) / np.float32(255.0))
            lanes = mat == k
            bad = sum(int((smp[:, c][lanes] != want).sum()) for c in range(3, 9))
            print("grey set, %s list, %s: texture %d (%d x %d, g = %d): %d lanes, %d values off" % (what, arith, k, Y.SHAPES[k][0], Y.SHAPES[k][1], g, int(lanes.sum()), bad))
            assert lanes.sum() >= 256 and bad == 0, (what, k, bad)           # (16 triangles of every TEX material at the least, a full block each)
        assert (smp[:, 3:][np.broadcast_to((mat == -2)[:, None], smp[:, 3:].shape)] == 0).all()      # nothing for a lane that did not hit


@pytest.mark.parametrize("arith,mode", ARITH)
def test_a_dyadic_triangle_and_its_integer_shifted_partner_sample_identically(torch_mod, arith, mode):
    """single-triangle blocks, tight clusters of identical barycentrics, the same rays: the noise set's samples of a triangle whose coordinates
    are multiples of 1/64 and of its partner, shifted by exact integers up to +-8000, are the same bits (every step of the interpolation is
    exact for both, tests/materials_synth.py)"""
    sc, ms, _ = device_sets()
    s = Y.synth()
    pairs = [s.pair_packets(k) for k in range(4)]
    a, b = stack_packets([p[0] for p in pairs], True), stack_packets([p[1] for p in pairs], True)
    xy = s.packet_xy(4)
    sc.set_arith(arith)
    try:
        pa, pb = shade_packets(torch_mod, ms, a, xy), shade_packets(torch_mod, ms, b, xy)
        ra, rb = shade_rays(torch_mod, ms, a, a["dirs"], None), shade_rays(torch_mod, ms, b, b["dirs"], None)
    finally:
        sc.set_arith("ieee")
    assert (a["tri"] != b["tri"]).all() and np.array_equal(a["u"], b["u"]) and np.array_equal(a["dirs"], b["dirs"])
    compare_planes("pairs through k_mat_sample, %s" % arith, pb, pa)
    compare_planes("pairs through k_mat_sample_rays, %s" % arith, rb, ra)
    tex = np.isin(lane_materials(a), np.arange(len(Y.SHAPES)))
    assert tex.sum() >= 16 * 16 and pa[:, 3:6].transpose(0, 2, 3, 1)[tex].any() and len(np.unique(pa[:, 3][tex])) >= 64      # textured lanes, and the taps differ


# ---- 5. the mirror stage ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_mirror_stage_on_synthetic_samples(torch_mod, arith, mode):
    """synthetic distances and a synthetic sample buffer: normals of length 0 (exact zeros on hit lanes), 1e-20, ~1 and 1e3, axis-aligned unit
    normals; all six outputs by bytes, and the nested call's TracingRays"""
    torch = torch_mod
    sc, ms, _ = device_sets()
    xy, t, smp = Y.mirror_inputs()
    want, selected = Y.expected_mirror(mode)
    n = len(xy)
    sc.set_arith(arith)
    try:
        st = sc.new_stats()
        got = [a.cpu().numpy() for a in ms.mirror_packets(CAM, RESX, RESY, dev(torch, xy), dev(torch, t.reshape(n, 256)), dev(torch, smp), stats=st)]
        st = st.cpu().numpy()
    finally:
        sc.set_arith("ieee")
    nrm, hit = smp[:, 0:3].transpose(0, 2, 1, 3), t < INF
    assert ((nrm == 0).all(axis=2) & hit).sum() >= 64 and (hit.all(axis=(1, 2))).any() and (~hit.any(axis=(1, 2))).any()
    failed = []
    for k, g in zip(("origin", "dir", "idir", "mask", "distance", "object"), got):
        w = want[k]
        g = np.ascontiguousarray(g.reshape(w.shape))
        assert g.dtype == w.dtype, (k, g.dtype, w.dtype)
        ne = g.view(np.uint8) != w.view(np.uint8)
        print("mirror %s %s: %d differing bytes of %d" % (arith, k, int(ne.sum()), ne.size))
        if ne.any():
            failed.append((k, int(ne.sum()), np.argwhere(ne)[:4].tolist()))
    assert not failed, failed
    assert np.isfinite(want["origin"]).all() and np.isfinite(want["dir"]).all()
    assert st.tolist() == [0, 0, selected, 0] and selected >= 1024


# ---- 6. one frame through the staged launches ----
@functools.lru_cache(maxsize=None)
def frame_case():
    """materials_synth.frame_case() on the device"""
    s = Y.synth()
    c, mat_index, ref = Y.frame_case()
    hb = HostBVH.build(c["tv"])
    assert np.array_equal(hb.perm, c["osc"].perm) and hb.nodes.tobytes() == c["osc"].nodes.tobytes()
    sc = Scene(hb, 0)
    ms = P.MaterialSet(sc, c["uv"], c["nrm"], mat_index, c["flat"], s.material_map, product_materials(s.descs), [P.Texture(t) for t in s.textures])
    return c, sc, ms, ref


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("reflections", [False, True])
def test_one_frame_with_the_ten_texture_set(torch_mod, reflections, arith, mode):
    c, sc, ms, ref = frame_case()
    cam = c["cam70"]
    if reflections:
        bd = B.BounceDiag()
        want, wst, _, _ = B.BounceRef(ref).render(cam.as_array13(), RESX, RESY, c["lights"], mode=mode, diag=bd)
        d = bd.primary
    else:
        d = M.Diag()
        want, wst, _, _ = ref.render(cam.as_array13(), RESX, RESY, c["lights"], mode=mode, diag=d)
    sc.set_arith(arith)
    try:
        st = sc.new_stats()
        frame = ms.render(cam, RESX, RESY, c["lights"], stats=st, reflections=reflections).cpu().numpy()
        st = st.cpu().numpy().astype(np.uint64)
    finally:
        sc.set_arith("ieee")
    bad = np.argwhere((frame != want).any(axis=2))
    sampled = sorted({t for (t, _) in d.mips})
    print("frame %s reflections=%s: %d differing pixels; stats %s / %s; textures sampled %s" % (arith, reflections, len(bad), st.tolist(), wst.tolist(), sampled))
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), frame[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())
    assert np.array_equal(st, wst), (st, wst)
    assert sampled == list(range(len(Y.SHAPES))) and d.hit_pixels >= 1000      # every texture of the set is sampled by the frame
