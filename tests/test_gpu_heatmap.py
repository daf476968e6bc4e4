"""Per-packet TreeStats and the gVals[5] heat-map of plain scenes (include/snail_heatmap.h) on the GPU, in both arithmetics.

Expected counters come from the CPU oracle wherever it can give them per packet -- primary packets one at a time (orc_gen_packet + orc_trace_rays,
plus the 256 rays of TracingRays), one-packet lit frames (orc_render_whitted's stats ARE the packet's) -- and, for the packets of a lit multi-packet
frame, from the already shipped snail_render_whitted_packets_dev run on the one-packet list [that packet], whose d_stats is that packet's RayTrace
call; their sum is held against the oracle's frame stats.  Bytes are tests/heat_ref.py applied to those counters.

Shapes are the smallest at which the booking can go wrong: 48x32 (six packets: the dispatch interleave maps block -> packet), 40x24 (cut edge
packets), a shuffled list with a packet listed twice, the depth-63 chain (the DEEP instantiations), packets the main kernel defers to the exact pass,
lights that are culled for some packets and traced for others."""
import numpy as np
import pytest

from snail_amd import HostBVH
from snail_amd.camera import Camera
from tests import extremes as X
from tests import heat_ref as H
from tests import oracle_lib as O
from tests import util as U

pytestmark = pytest.mark.gpu

F = np.float32
ARITHS = [("ieee", O.MODE_IEEE), ("host_sse", O.MODE_SSE)]
REFL, AA4 = 1, 4


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _scene(hb, arith):
    from snail_amd.scene import Scene
    sc = Scene(hb, 0)
    sc.set_arith(arith)
    return sc


def frame_xy(resx, resy):
    return np.array([(x, y) for y in range(0, resy, 16) for x in range(0, resx, 16)], dtype=np.int32)


def oracle_primary_packet(osc, cam13, resx, resy, x, y, mode):
    """-> (TreeStats of the primary packet at (x, y): TraversePrimary + 256 rays, whether the main kernel has to defer it: a non-finite value)"""
    d, di = O.gen_packet(cam13, resx, resy, int(x), int(y), mode)
    org = np.repeat(np.asarray(cam13[:3], dtype=F), 4)[None, :].copy()
    dist = np.full((64, 4), np.inf, dtype=F)
    st = osc.trace_rays(org, d.reshape(64, 12).copy(), di.reshape(64, 12).copy(), None, dist, np.zeros((64, 4), np.int32), np.zeros((64, 8), F), 1, 64, True, mode=mode)
    st = st.astype(np.uint64)
    st[2] += 256
    return st, not (np.isfinite(d).all() and np.isfinite(di).all())


def oracle_primary_packets(osc, cam13, resx, resy, xy, mode):
    got = [oracle_primary_packet(osc, cam13, resx, resy, x, y, mode) for x, y in np.asarray(xy).tolist()]
    return np.array([g[0] for g in got], dtype=np.uint64), np.array([g[1] for g in got])


def dev_packet_stats(torch_mod, sc, cam, resx, resy, xy=None, **kw):
    """-> (uint64 [n, 4] per packet, uint64 [4] the call's d_stats)"""
    stats = sc.new_stats()
    dxy = None if xy is None else torch_mod.from_numpy(np.ascontiguousarray(xy, dtype=np.int32)).cuda()
    out = sc.packet_stats(cam, resx, resy, dxy, stats=stats, **kw)
    torch_mod.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32).astype(np.uint64), stats.cpu().numpy().astype(np.uint64)


def shipped_packet_stats(torch_mod, sc, cam, resx, resy, xy, lights, refl):
    """per packet: d_stats of snail_render_whitted_packets_dev on the one-packet list [that packet]"""
    rows = []
    for x, y in np.asarray(xy).tolist():
        st = sc.new_stats()
        one = torch_mod.tensor([[x, y]], dtype=torch_mod.int32, device="cuda")
        sc.render_whitted_packets(cam, resx, resy, one, lights, stats=st, reflections=refl)
        torch_mod.cuda.synchronize()
        rows.append(st.cpu().numpy().astype(np.uint64))
    return np.array(rows, dtype=np.uint64)


# ---- the scene of the lit cases: chosen on the CPU so that lights are culled for some packets, shadow packets are skipped whole for others --------

def heat_scene():
    """A 4x4 grid of floor quads at y = 0 with a dozen small raised patches (varied cost), and ONE big triangle at y = 8, above the camera and out of
    its view, whose shadow from light A ends on the line x = 0 of the floor: the shadow packets of the view's left third are occluded whole by that
    one triangle (TraverseShadow's early out: skips), the middle third's in part, the right third's not at all."""
    tris = []
    g = np.linspace(-12, 12, 5)
    for i in range(4):
        for j in range(4):
            x0, x1, z0, z1 = g[i], g[i + 1], g[j], g[j + 1]
            tris += [[[x1, 0, z1], [x0, 0, z1], [x0, 0, z0]], [[x1, 0, z0], [x1, 0, z1], [x0, 0, z0]]]
    rng = np.random.RandomState(3)
    for _ in range(12):
        cx, cz = rng.uniform(-5, 5, 2)
        s = rng.uniform(0.2, 0.6)
        h = rng.uniform(0.1, 0.5)
        tris += [[[cx + s, h, cz + s], [cx - s, h, cz + s], [cx - s, h, cz - s]], [[cx + s, h, cz - s], [cx + s, h, cz + s], [cx - s, h, cz - s]]]
    tris.append([[-3.43, 8, 40], [-60, 8, 0], [-3.43, 8, -40]])
    return np.array(tris, dtype=F).reshape(-1, 9)


LIGHT_A = [-6, 14, 0.5, 1, 0.9, 0.8, 60]            # high above the occluder: reaches every packet, shadowed on the left
LIGHT_B = [-4.5, 0.8, -2.0, 0.7, 0.8, 1, 1.5]       # low, small radius: culled at packet level for most packets, traced for the nearest
LIGHT_FAR = [300, 300, 300, 1, 1, 1, 1.0]           # culled for every packet
_pair = {}


def heat_pair():
    if "p" not in _pair:
        tv = heat_scene()
        _pair["p"] = (HostBVH.build(tv), O.OracleScene(tv))
    return _pair["p"]


def down_camera(dx=0.3, dz=0.2, h=5.0):
    return Camera(np.array([dx, h, dz], F), np.array([1, 0, 0], F), np.array([0, 0, 1], F), np.array([0, -1, 0], F), F(1.0))


def lights_arr(ls):
    return np.array(ls, dtype=F).reshape(-1, 7)


# ---- A: primary only, against the oracle per packet ------------------------------------------------------------------------------------------

def _case(name):
    """-> (HostBVH, OracleScene, camera, every packet deferred by rule)"""
    if name == "extremes-scaled":          # beyond the fastOK bound: the main kernel defers EVERY packet to the exact pass
        tv, hb, osc = X.scaled_pair("box", 31)
        assert not X.fast_ok(osc.tris, osc.nodes)
        return hb, osc, X.scaled_camera("box", 31), True
    if name == "extremes-centre":          # a view plane at distance 2^-80: the ray through the frame's centre has p = (0, 0, 2^-80), p.p underflows to 0,
        tv, hb, osc = U.scene_pair("box")  # RSqrt gives inf and the direction NaN -- that ONE packet is deferred, the others are not
        c = U.camera_for("box", tv)
        return hb, osc, Camera(c.pos, c.right, c.up, c.front, F(2.0 ** -80)), False
    tv, hb, osc = U.scene_pair(name)
    return hb, osc, U.camera_for(name, tv), False


@pytest.mark.parametrize("arith,mode", ARITHS)
@pytest.mark.parametrize("name", ["atrium:0.02", "chain", "extremes-scaled", "extremes-centre"])
def test_primary_counters_match_the_oracle(torch_mod, name, arith, mode):
    hb, osc, cam, all_deferred = _case(name)
    sc = _scene(hb, arith)
    assert (osc.depth > 62) == (name == "chain")
    cam13 = cam.as_array13()
    for resx, resy in ((48, 32), (40, 24)):
        xy = frame_xy(resx, resy)
        want, deferred = oracle_primary_packets(osc, cam13, resx, resy, xy, mode)
        if name == "extremes-centre" and (resx, resy) == (48, 32):
            assert deferred.any() and not deferred.all()                         # some packets take the exact pass, some the main kernel
        elif name != "extremes-centre":
            assert not deferred.any() and len(np.unique(want, axis=0)) >= 3      # (all_deferred: by the scene's magnitudes, not by a value of the packet)
        got, tot = dev_packet_stats(torch_mod, sc, cam, resx, resy)
        assert np.array_equal(got, want), (name, arith, resx, resy, got.tolist(), want.tolist())
        assert np.array_equal(tot, want.sum(axis=0))
        assert np.array_equal(tot, osc.render_primary(cam13, resx, resy, mode=mode, threads=2)[4])
        # an explicit list: shuffled, one packet twice -- counters by list position
        order = np.array([4, 1, 5, 0, 1, 3, 2])
        got, tot = dev_packet_stats(torch_mod, sc, cam, resx, resy, xy[order])
        assert np.array_equal(got, want[order]), (name, arith, resx, resy, "list")
        assert np.array_equal(tot, want[order].sum(axis=0))
    sc.close()


# ---- B: lit one-packet frames against the oracle -----------------------------------------------------------------------------------------------

LIGHT_SETS = {"one": [LIGHT_B], "two": [LIGHT_A, LIGHT_B], "culled": [LIGHT_FAR], "traced+culled": [LIGHT_A, LIGHT_FAR]}


@pytest.mark.parametrize("arith,mode", ARITHS)
def test_lit_one_packet_frames_match_the_oracle(torch_mod, arith, mode):
    hb, osc = heat_pair()
    sc = _scene(hb, arith)
    seen_skip = seen_cull = 0
    for resx, resy in ((16, 16), (13, 9)):
        for cam in (down_camera(-2.4, -1.2, 3.0), down_camera(0.3, 0.2, 5.0), down_camera(-4.0, -1.8, 2.0)):
            cam13 = cam.as_array13()
            for refl in (False, True):
                unlit = osc.render_whitted(cam13, resx, resy, lights_arr([]), mode=mode, reflections=refl, threads=1)[1]
                for key, ls in LIGHT_SETS.items():
                    want = osc.render_whitted(cam13, resx, resy, lights_arr(ls), mode=mode, reflections=refl, threads=1)[1]
                    got, tot = dev_packet_stats(torch_mod, sc, cam, resx, resy, lights7=lights_arr(ls), reflections=refl)
                    assert got.shape == (1, 4) and np.array_equal(got[0], want), (arith, resx, resy, cam.pos.tolist(), refl, key, got.tolist(), want.tolist())
                    assert np.array_equal(tot, want)
                    if key == "culled":
                        assert np.array_equal(want, unlit)                       # a culled light books nothing
                        seen_cull += 1
                    seen_skip += int(want[3] > 0)
    assert seen_skip > 0 and seen_cull > 0
    sc.close()


# ---- C, D: lit multi-packet frames; bytes -----------------------------------------------------------------------------------------------------

_expected = {}


def expected_lit(torch_mod, sc, arith, key, refl, resx=48, resy=32, cam=None):
    """per packet of the frame: the shipped one-packet-list launch's d_stats (computed once per configuration and shared)"""
    k = (arith, key, refl, resx, resy)
    if k not in _expected:
        _expected[k] = shipped_packet_stats(torch_mod, sc, cam or down_camera(), resx, resy, frame_xy(resx, resy), lights_arr(LIGHT_SETS[key]), refl)
    return _expected[k]


@pytest.mark.parametrize("arith,mode", ARITHS)
def test_lit_frame_counters_per_packet_and_in_sum(torch_mod, arith, mode):
    hb, osc = heat_pair()
    sc = _scene(hb, arith)
    cam = down_camera()
    cam13 = cam.as_array13()
    xy = frame_xy(48, 32)
    primary, _ = oracle_primary_packets(osc, cam13, 48, 32, xy, mode)
    for key in ("one", "two"):
        for refl in (False, True):
            want = expected_lit(torch_mod, sc, arith, key, refl)
            frame_stats = osc.render_whitted(cam13, 48, 32, lights_arr(LIGHT_SETS[key]), mode=mode, reflections=refl, threads=2)[1]
            assert np.array_equal(want.sum(axis=0), frame_stats)                 # the expected values themselves add up to the oracle's frame
            got, tot = dev_packet_stats(torch_mod, sc, cam, 48, 32, lights7=lights_arr(LIGHT_SETS[key]), reflections=refl)
            assert np.array_equal(got, want), (arith, key, refl, got.tolist(), want.tolist())
            assert np.array_equal(tot, frame_stats) and np.array_equal(got.sum(axis=0), tot)
            assert len({tuple(H.heat_bgr_bytes(p).tolist()) for p in want}) >= 3
            if key == "one" and not refl:      # light B alone: culled (packet, light) pairs book nothing, traced ones do
                culled = (want == primary).all(axis=1)
                assert culled.any() and not culled.all()
            if key == "two":
                assert (want[:, 3] > 0).any() and not (want[:, 3] > 0).all()     # shadow packets skipped whole on the left only
    sc.close()


@pytest.mark.parametrize("arith,mode", ARITHS)
def test_heat_bytes_in_every_store(torch_mod, arith, mode):
    """packet-major (grid and list), host image with a pitch (padding untouched), planar tiles: heat_ref of the expected counters"""
    hb, osc = heat_pair()
    sc = _scene(hb, arith)
    cam = down_camera()
    cam13 = cam.as_array13()
    from snail_amd.scene import Scene
    for resx, resy, key, refl in ((48, 32, "two", True), (40, 24, None, False), (48, 32, "one", False)):
        xy = frame_xy(resx, resy)
        if key is None:
            want, ls = oracle_primary_packets(osc, cam13, resx, resy, xy, mode)[0], lights_arr([])
        else:
            want, ls = expected_lit(torch_mod, sc, arith, key, refl), lights_arr(LIGHT_SETS[key])
        flags = Scene.RENDER_REFLECTIONS if refl else 0
        want_packets = H.heat_packets(want)
        want_frame = H.heat_frame(want, xy, resx, resy)
        assert len(np.unique(want_frame.reshape(-1, 3), axis=0)) >= 3
        # packet-major, the frame's grid; the counters come back with the bytes
        pst = torch_mod.zeros((len(xy), 4), dtype=torch_mod.int32, device="cuda")
        st = sc.new_stats()
        got = sc.render_heat_packets(cam, resx, resy, None, ls, reflections=refl, packet_stats=pst, stats=st)
        torch_mod.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), want_packets)                   # every ray of a packet, misses and rays outside the image included
        assert np.array_equal(pst.cpu().numpy().view(np.uint32).astype(np.uint64), want)
        assert np.array_equal(st.cpu().numpy().astype(np.uint64), want.sum(axis=0))
        # packet-major, a shuffled list with a packet listed twice, no counter output
        order = np.array([3, 5, 0, 3, 1, 2, 4])
        got = sc.render_heat_packets(cam, resx, resy, torch_mod.from_numpy(xy[order]).cuda(), ls, reflections=refl)
        torch_mod.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), want_packets[order])
        # host image with a pitch: the padding keeps its poison
        pitch = resx * 3 + 7
        img, stats = sc.render_heat_image_host(cam, resx, resy, ls, flags, pitch=pitch, fill=0xAB)
        assert np.array_equal(img[:, :resx * 3].reshape(resy, resx, 3), want_frame) and (img[:, resx * 3:] == 0xAB).all()
        assert np.array_equal(stats, want.sum(axis=0))
        img, _ = sc.render_heat_image_host(cam, resx, resy, ls, flags)
        assert np.array_equal(img, want_frame)
        # planar tiles (R, G-R, B-R), tiles cut at the image edge, one of them not packet-sized
        tiles = np.array([[0, 0, 32, 16], [32, 0, resx - 32, 16], [0, 16, 16, resy - 16], [16, 16, resx - 16, resy - 16]], dtype=np.int32)
        data, offsets, stats = sc.render_heat_tiles_host(cam, resx, resy, tiles, ls, flags)
        planes = O.planar_encode(want_frame, tiles)
        for k, o in enumerate(offsets.tolist()):
            assert np.array_equal(data[o:o + len(planes[k])], planes[k]), (arith, resx, resy, k)
        assert np.array_equal(stats, want.sum(axis=0))
    sc.close()


# ---- E: 4x antialiasing ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arith,mode", ARITHS)
def test_antialiased_heat(torch_mod, arith, mode):
    """40x24: quadrant (k & 1, k >> 1) of packet (x, y) carries the colour of packet (2x + 16 (k & 1), 2y + 16 (k >> 1)) of the 80x48 frame; the
    sub-packets at x = 80 lie outside that frame: traced and counted, their pixels dropped with the packet's right half"""
    hb, osc = heat_pair()
    sc = _scene(hb, arith)
    cam = down_camera()
    cam13 = cam.as_array13()
    from snail_amd.scene import Scene
    resx, resy = 40, 24
    xy = frame_xy(resx, resy)
    xy2 = np.array([(2 * x + 16 * (k & 1), 2 * y + 16 * (k >> 1)) for x, y in xy.tolist() for k in range(4)], dtype=np.int32)
    assert (xy2[:, 0] >= 2 * resx).any()
    for key, refl in ((None, False), ("two", False), ("one", True)):
        if key is None:
            want, ls = oracle_primary_packets(osc, cam13, 2 * resx, 2 * resy, xy2, mode)[0], lights_arr([])
        else:
            ls = lights_arr(LIGHT_SETS[key])
            want = shipped_packet_stats(torch_mod, sc, cam, 2 * resx, 2 * resy, xy2, ls, refl)
        flags = Scene.RENDER_AA4 | (Scene.RENDER_REFLECTIONS if refl else 0)
        frame_stats = osc.render_whitted(cam13, resx, resy, ls, mode=mode, reflections=refl, antialias=True, threads=2)[1]
        assert np.array_equal(want.sum(axis=0), frame_stats)
        want_packets = H.heat_aa_packets(want.reshape(-1, 4, 4))
        want_frame = H.packets_to_frame(want_packets, xy, resx, resy)
        assert len(np.unique(want_frame.reshape(-1, 3), axis=0)) >= 3
        pst = torch_mod.zeros((len(xy), 4, 4), dtype=torch_mod.int32, device="cuda")
        st = sc.new_stats()
        got = sc.render_heat_packets(cam, resx, resy, None, ls, reflections=refl, aa4=True, packet_stats=pst, stats=st)
        torch_mod.cuda.synchronize()
        assert np.array_equal(pst.cpu().numpy().view(np.uint32).astype(np.uint64).reshape(-1, 4), want), (arith, key, refl)
        assert np.array_equal(got.cpu().numpy(), want_packets)
        assert np.array_equal(st.cpu().numpy().astype(np.uint64), frame_stats)
        got = sc.render_heat_packets(cam, resx, resy, torch_mod.from_numpy(xy[::-1].copy()).cuda(), ls, reflections=refl, aa4=True)
        torch_mod.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), want_packets[::-1])
        img, stats = sc.render_heat_image_host(cam, resx, resy, ls, flags)
        assert np.array_equal(img, want_frame) and np.array_equal(stats, frame_stats)
        tiles = np.array([[0, 0, 32, 16], [32, 0, 8, 24], [0, 16, 32, 8]], dtype=np.int32)
        data, offsets, stats = sc.render_heat_tiles_host(cam, resx, resy, tiles, ls, flags)
        planes = O.planar_encode(want_frame, tiles)
        for k, o in enumerate(offsets.tolist()):
            assert np.array_equal(data[o:o + len(planes[k])], planes[k]), (arith, key, k)
        # tile (32, 0, 8, 24) holds the packets (32, 0) and (32, 16) once each: the tile list's counters are those of its own packets
        tile_xy = [(x, y) for tx, ty, tw, th in tiles.tolist() for y in range(ty, ty + th, 16) for x in range(tx, tx + tw, 16)]
        index = {tuple(p): i for i, p in enumerate(xy.tolist())}
        assert np.array_equal(stats, sum(want.reshape(-1, 4, 4)[index[p]].sum(axis=0) for p in tile_xy))
    sc.close()


# ---- F: two launches in flight ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arith,mode", ARITHS)
def test_two_launches_in_flight_share_nothing(torch_mod, arith, mode):
    hb, osc = heat_pair()
    sc = _scene(hb, arith)
    cams = (down_camera(), down_camera(-1.1, 0.7, 4.0))
    ls = lights_arr(LIGHT_SETS["two"])
    n = 6
    alone = []
    for cam in cams:
        pst = torch_mod.zeros((n, 4), dtype=torch_mod.int32, device="cuda")
        out = sc.render_heat_packets(cam, 48, 32, None, ls, reflections=True, packet_stats=pst)
        torch_mod.cuda.synchronize()
        alone.append((out.cpu().numpy(), pst.cpu().numpy()))
    assert not np.array_equal(alone[0][1], alone[1][1])
    streams = [torch_mod.cuda.Stream(), torch_mod.cuda.Stream()]
    outs = [torch_mod.zeros((n, 256, 3), dtype=torch_mod.uint8, device="cuda") for _ in cams]
    psts = [torch_mod.full((n, 4), -1, dtype=torch_mod.int32, device="cuda") for _ in cams]
    tots = [sc.new_stats() for _ in cams]
    torch_mod.cuda.synchronize()
    for rnd in range(3):                       # back to back, no synchronisation in between; more launches than one scratch set
        for k, cam in enumerate(cams):
            sc.render_heat_packets(cam, 48, 32, None, ls, reflections=True, out=outs[k], packet_stats=psts[k], stats=tots[k] if rnd == 0 else None, stream=streams[k])
    torch_mod.cuda.synchronize()
    for k in range(2):
        assert np.array_equal(outs[k].cpu().numpy(), alone[k][0]) and np.array_equal(psts[k].cpu().numpy(), alone[k][1]), (arith, k)
        assert np.array_equal(tots[k].cpu().numpy().astype(np.uint64), alone[k][1].view(np.uint32).astype(np.uint64).sum(axis=0))
    sc.close()
