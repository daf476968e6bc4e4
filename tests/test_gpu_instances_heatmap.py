"""Per-packet TreeStats and the gVals[5] heat-map of instanced scenes (include/snail_heatmap.h, snail_instances_*heat*) on the GPU, in both
arithmetics.  Expected counters: tests/dbvh_shade_ref.py's Scene<DBVH>::RayTrace called per packet with a fresh TreeStats (through
tests/dbvh_tiles_ref.py's packet set-up); bytes: tests/heat_ref.py on those counters, then the restated reduction, tint and ConvColor.  The cases
are those of tests/instances_shade_cases.py at their smallest frames."""
import os
import subprocess

import numpy as np
import pytest

from tests import dbvh_shade_ref as S
from tests import dbvh_tiles_ref as T
from tests import heat_ref as H
from tests import instances_shade_cases as K
from tests.test_gpu_instances import ARITH, blas, set_arith
from tests.test_gpu_instances_shade import device_scene, torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F = np.float32
AA, REFL = T.AA4, T.REFLECTIONS
_cases = {}
_want = {}


def case(name):
    if name not in _cases:
        names, rot, tr, bi, _, _, cam, lights, cref = K.case(name)
        isc, ref = device_scene(names, rot, tr, bi, cref)
        _cases[name] = (isc, T.TilesRef(ref), cam, lights)
    return _cases[name]


def ref_packet_stats(name, resx, resy, xy, refl, mode):
    """the restatement's RayTrace per packet, each with a TreeStats of its own (computed once per configuration and shared)"""
    xy = np.asarray(xy, dtype=np.int32).reshape(-1, 2)
    key = (name, resx, resy, xy.tobytes(), refl, mode)
    if key not in _want:
        _, tref, cam, lights = case(name)
        cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32)
        L = (lights, np.array([0.1, 0.1, 0.1], F), np.ones(3, F), bool(refl))
        rows = []
        for px, py in xy.tolist():
            st = np.zeros(4, dtype=np.uint64)
            tref._packet(cam13, resx, resy, px, py, L, False, mode, st, None, 0)
            rows.append(st)
        _want[key] = np.array(rows, dtype=np.uint64)
    return _want[key]


def u64(t):
    return t.cpu().numpy().view(np.uint32).astype(np.uint64)


def tinted_bytes(rgb, tint):
    return S.conv_color(rgb if tint is None else T.apply_tint(rgb, tint))


def want_packets(pstats, tint=None):
    return np.stack([np.tile(tinted_bytes(H.heat_rgb(p), tint), (256, 1)) for p in np.asarray(pstats).reshape(-1, 4)])


def want_aa_packets(pstats4, tint=None):
    ps = np.asarray(pstats4).reshape(-1, 4, 4)
    out = np.zeros((len(ps), 16, 16, 3), dtype=np.uint8)
    for i, four in enumerate(ps):
        for k in range(4):
            c = H.heat_rgb(four[k])
            out[i, 8 * (k >> 1):8 * (k >> 1) + 8, 8 * (k & 1):8 * (k & 1) + 8] = tinted_bytes((c + c) * F(0.25) + (c + c) * F(0.25), tint)
    return out.reshape(-1, 256, 3)


def check_tiles(got, off, want_bgr, tiles, resx, resy):
    k0 = 0
    for k, (x, y, w, h) in enumerate(np.asarray(tiles).reshape(-1, 4).tolist()):
        n = ((w + 15) // 16) * ((h + 15) // 16)
        want = T.planar_from_packets(want_bgr[k0:k0 + n], w, h, resx - x, resy - y)
        k0 += n
        assert np.array_equal(got[off[k]:off[k] + 3 * w * h], want), ("tile", k)


@pytest.mark.parametrize("arith,mode", ARITH)
def test_instanced_counters_and_bytes(torch_mod, arith, mode):
    torch = torch_mod
    isc, tref, cam, lights = case("field")
    set_arith(isc, arith)
    resx, resy = 48, 32
    xy = S.frame_packets(resx, resy)
    tint = T.rank_tint(3)
    for refl in (False, True):
        want = ref_packet_stats("field", resx, resy, xy, refl, mode)
        assert len({tuple(H.heat_bgr_bytes(p).tolist()) for p in want}) >= 3 and (want[:, 2] > 256).any()       # several colours; shadow rays were cast
        # the frame's grid; the sum is the shipped lit frame's d_stats
        st = isc.new_stats()
        got = isc.packet_stats(cam, resx, resy, None, lights, reflections=refl, stats=st)
        st2 = isc.new_stats()
        isc.render_whitted(cam, resx, resy, lights, stats=st2, reflections=refl)
        torch.cuda.synchronize()
        assert np.array_equal(u64(got), want), (arith, refl, u64(got).tolist(), want.tolist())
        assert np.array_equal(st.cpu().numpy().astype(np.uint64), want.sum(axis=0)) and np.array_equal(st.cpu().numpy(), st2.cpu().numpy())
        # a shuffled list with a packet twice: counters and bytes by list position, with and without the rank tint
        order = np.array([2, 5, 0, 2, 4, 1, 3])
        dxy = torch.from_numpy(np.ascontiguousarray(xy[order])).cuda()
        flags = REFL if refl else 0
        pst = torch.zeros((len(order), 4), dtype=torch.int32, device="cuda")
        a = isc.render_heat_packets(cam, resx, resy, dxy, lights, flags=flags, packet_stats=pst)
        b = isc.render_heat_packets(cam, resx, resy, dxy, lights, flags=flags, tint=tint)
        torch.cuda.synchronize()
        assert np.array_equal(u64(pst), want[order])
        assert np.array_equal(a.cpu().numpy(), want_packets(want[order])) and np.array_equal(a.cpu().numpy(), H.heat_packets(want[order]))
        assert np.array_equal(b.cpu().numpy(), want_packets(want[order], tint)) and not np.array_equal(a.cpu().numpy(), b.cpu().numpy())
        # the frame with a pitch (padding untouched) and the planar tile list with the tint
        pitch = resx * 3 + 5
        img, ist = isc.render_heat_frame_host(cam, resx, resy, lights, flags=flags, pitch=pitch, fill=0xAB)
        assert np.array_equal(img[:, :resx * 3].reshape(resy, resx, 3), H.heat_frame(want, xy, resx, resy)) and (img[:, resx * 3:] == 0xAB).all()
        assert np.array_equal(ist, want.sum(axis=0))
        tiles = np.array([[0, 0, 32, 16], [32, 0, 16, 32], [0, 16, 32, 16]], dtype=np.int32)
        index = {tuple(p): i for i, p in enumerate(xy.tolist())}
        sel = [index[tuple(p)] for p in T.tile_packets(tiles).tolist()]
        data, off, tst = isc.render_heat_tiles_host(cam, resx, resy, tiles, lights, flags=flags, tint=tint)
        check_tiles(data, off, want_packets(want[sel], tint), tiles, resx, resy)
        assert np.array_equal(tst, want[sel].sum(axis=0))
    set_arith(isc, "ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
def test_instanced_antialiased_heat_with_a_deep_blas(torch_mod, arith, mode):
    """chain + box (the DEEP inner walk), 24x24 with a bounce: four packets whose sixteen double-resolution packets partly lie outside the 48x48 frame"""
    torch = torch_mod
    assert blas("chain")[1].depth > 62
    isc, tref, cam, lights = case("deep")
    set_arith(isc, arith)
    resx, resy = 24, 24
    xy = S.frame_packets(resx, resy)
    xy2 = np.array([(2 * x + 16 * (k & 1), 2 * y + 16 * (k >> 1)) for x, y in xy.tolist() for k in range(4)], dtype=np.int32)
    assert (xy2[:, 0] >= 2 * resx).any() and (xy2[:, 1] >= 2 * resy).any()
    want = ref_packet_stats("deep", 2 * resx, 2 * resy, xy2, True, mode)
    assert len(np.unique(want, axis=0)) >= 3
    tint = T.rank_tint(15)
    pst = torch.zeros((len(xy), 4, 4), dtype=torch.int32, device="cuda")
    st = isc.new_stats()
    a = isc.render_heat_packets(cam, resx, resy, None, lights, flags=AA | REFL, packet_stats=pst, stats=st)
    b = isc.render_heat_packets(cam, resx, resy, None, lights, flags=AA | REFL, tint=tint)
    torch.cuda.synchronize()
    assert np.array_equal(u64(pst).reshape(-1, 4), want), (arith, u64(pst).reshape(-1, 4).tolist(), want.tolist())
    assert np.array_equal(st.cpu().numpy().astype(np.uint64), want.sum(axis=0))
    assert np.array_equal(a.cpu().numpy(), want_aa_packets(want)) and np.array_equal(a.cpu().numpy(), H.heat_aa_packets(want))
    assert np.array_equal(b.cpu().numpy(), want_aa_packets(want, tint))
    img, ist = isc.render_heat_frame_host(cam, resx, resy, lights, flags=AA | REFL)
    assert np.array_equal(img, H.packets_to_frame(want_aa_packets(want), xy, resx, resy)) and np.array_equal(ist, want.sum(axis=0))
    tiles = np.array([[0, 0, 24, 16], [0, 16, 24, 8]], dtype=np.int32)
    data, off, tst = isc.render_heat_tiles_host(cam, resx, resy, tiles, lights, flags=AA | REFL, tint=tint)
    check_tiles(data, off, want_aa_packets(want, tint), tiles, resx, resy)     # (the tiles' packets in order are the frame's)
    assert np.array_equal(tst, want.sum(axis=0))
    set_arith(isc, "ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
def test_cpp_adapter_routes_gvals5_to_the_device(torch_mod, tmp_path, arith, mode):
    """A C++ host in the reference's shape (tests/cpp/heatmap_mock.cpp, SNAIL_ADAPTER_DEVICE_HEATMAP): with gVals[5] the tile list and the image of a
    plain and of an instanced scene never reach the host renderer (a stub that exits) and carry the bytes and TreeStats of the C-ABI heat calls (the mock
    compares, with and without gVals[7], [9], [8]); gVals[5] + gVals[1] is the depth frame; gVals[6] with shading data still reaches the stub.  The
    gVals[5] tile buffers are held against the Python bindings here."""
    from snail_amd.render import divide_image
    from snail_amd.scene import Scene
    from tests import extremes as X
    from tests import util as U
    names, rot, tr, bi, _, _, _, _, _ = K.case("field")
    isc, tref, cam, lights = case("field")
    set_arith(isc, arith)
    resx, resy = 48, 32
    d = tmp_path
    for k, nm in enumerate(names):
        hb = blas(nm)[0].bvh
        hb.nodes.tofile(str(d / ("blas%d_nodes.bin" % k))); hb.tris.tofile(str(d / ("blas%d_tris.bin" % k)))
    xs, bs = isc.slot_transforms()
    isc.nodes().tofile(str(d / "top_nodes.bin")); xs.tofile(str(d / "xf12.bin")); bs.astype(np.int32).tofile(str(d / "blas_index.bin"))
    np.ascontiguousarray(cam.as_array13(), dtype=np.float32).tofile(str(d / "cam.bin"))
    np.ascontiguousarray(lights, dtype=np.float32).tofile(str(d / "lights7.bin"))
    ptv, phb, posc = U.scene_pair(names[0])
    pcam = U.camera_for(names[0], ptv)
    plights = X.lights_for(posc, pcam)
    np.ascontiguousarray(pcam.as_array13(), dtype=np.float32).tofile(str(d / "plain_cam.bin"))
    np.ascontiguousarray(plights, dtype=np.float32).tofile(str(d / "plain_lights7.bin"))
    tiles = divide_image(resx, resy)
    tiles.astype(np.int32).tofile(str(d / "tiles.bin"))
    np.array([resx, resy, int(arith == "host_sse"), len(names)] + [blas(nm)[0].bvh.depth for nm in names], dtype=np.int32).tofile(str(d / "meta.bin"))
    exe = str(tmp_path / "heatmap_mock")
    libdir = os.path.join(ROOT, "snail_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", os.path.join(ROOT, "tests", "cpp", "heatmap_mock.cpp"), "-o", exe, "-L" + libdir, "-lsnailhip",
                           "-Wl,-rpath," + libdir])
    r = subprocess.run([exe, str(d)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "heatmap adapter ok" in r.stdout, r.stdout + r.stderr
    assert "Render called" not in r.stdout
    want_i = isc.render_heat_tiles_host(cam, resx, resy, tiles, lights)[0]
    assert np.array_equal(np.fromfile(str(d / "out_inst_tiles.bin"), dtype=np.uint8), want_i) and len(np.unique(want_i)) >= 3
    sc = Scene(blas(names[0])[0].bvh, 0)
    sc.set_arith(arith)
    want_p = sc.render_heat_tiles_host(pcam, resx, resy, tiles, plights)[0]
    assert np.array_equal(np.fromfile(str(d / "out_plain_tiles.bin"), dtype=np.uint8), want_p) and len(np.unique(want_p)) >= 3
    sc.close()
    set_arith(isc, "ieee")
