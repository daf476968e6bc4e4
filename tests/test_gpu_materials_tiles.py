"""The tile renderer of full-shaded plain scenes on the MI355X (include/snail_materials_tiles.h; MaterialSet.frame_packets / .render_tiles_host /
.render_frame_host and the adapter's SNAIL_ADAPTER_DEVICE_MATERIALS routing): packets, planar tiles and frames byte for byte and TreeStats for
equality against the test-side restatement tests/materials_tiles_ref.py, in both arithmetics -- and, independent of that restatement, against
the entry points the header names as equivalent.  Frames, tile list and restatement objects are those of tests/materials_tiles_cases.py; what
they must exercise is asserted on the restatement's diagnostics without a GPU by tests/test_materials_tiles_host.py."""
import subprocess
import threading

import numpy as np
import pytest

from snail_amd import _lib
from snail_amd.scene import _stream_ptr
from tests import materials_bounce_cases as BK
from tests import materials_tiles_cases as C
from tests import materials_tiles_ref as MT
from tests import oracle_lib as O
from tests.test_gpu_materials_bounce import device_set, torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu
ARITH = [("ieee", O.MODE_IEEE), ("host_sse", O.MODE_SSE)]
REFL, DEPTH, AA = C.REFL, C.DEPTH, C.AA
FILL = 0xA5


def check_tiles(ms, name, res, tiles, offsets, total, inside, flags, tint, mode, lights_key="case"):
    """one snail_materials_render_tiles call into a prefilled buffer of the caller's against the restatement -> the buffer"""
    cam = C.camera(name, res)
    lights = BK.lights_of(name, lights_key)
    data = np.full(total, FILL, dtype=np.uint8)
    got, off, st = ms.render_tiles_host(cam, res[0], res[1], tiles, offsets, lights, flags=flags, tint=tint, data=data)
    want, wst = C.tref(name).tiles(cam.as_array13(), res[0], res[1], tiles, lights, flags, tint, mode=mode)
    assert got is data and np.array_equal(off, offsets)
    for k, (x, y, w, h) in enumerate(np.asarray(tiles).reshape(-1, 4).tolist()):
        g = data[off[k]:off[k] + 3 * w * h]
        bad = np.flatnonzero(g != want[k])
        assert len(bad) == 0, ("tile", k, (x, y, w, h), "flags", flags, len(bad), bad[:5].tolist(), g[bad[:5]].tolist(), want[k][bad[:5]].tolist())
    assert np.concatenate(want).any()
    assert (data[~inside] == FILL).all(), "bytes outside the tiles were written"
    assert np.array_equal(st, wst), (name, flags, st, wst)
    return data


# ---- 1. the packet form ----
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("lights_key", ["case", "none", "eight"])
def test_packet_form_every_flag_combination(torch_mod, lights_key, arith, mode):
    """`large`, 48 x 32 (6 packets): all eight flag combinations without tint and with rank_tint(15), whose green factor 1.7 drives channels past
    255; the case's two lights -- and flags 0 and AA4 | REFLECTIONS once without lights (colour = diffuse) and once with eight"""
    torch = torch_mod
    sc, ms = device_set("large")
    res = C.PACKET_RES
    cam = C.camera("large", res)
    lights = BK.lights_of("large", lights_key)
    xy = C.frame_xy(res)
    dxy = torch.from_numpy(np.ascontiguousarray(xy)).to("cuda:0")
    assert len(xy) == 6
    combos = range(8) if lights_key == "case" else (0, AA | REFL)
    clamped = 0
    sc.set_arith(arith)
    try:
        for flags in combos:
            for tint in (None, MT.rank_tint(15)):
                st = sc.new_stats()
                got = ms.frame_packets(cam, res[0], res[1], dxy, lights, flags=flags, tint=tint, stats=st).cpu().numpy()
                want, wst = C.tref("large").packets(cam.as_array13(), res[0], res[1], xy, lights, flags, tint, mode=mode)
                bad = np.argwhere(got != want)
                print("large %s lights=%s flags=%d tint=%s: %d differing bytes; stats %s / %s" % (arith, lights_key, flags, tint is not None, len(bad),
                                                                                                 st.cpu().numpy().tolist(), wst.tolist()))
                assert want.any() and len(bad) == 0, (flags, tint, len(bad), bad[:5].tolist())
                assert np.array_equal(st.cpu().numpy().astype(np.uint64), wst), (flags, st, wst)
                if tint is not None:
                    plain, _ = C.tref("large").packets(cam.as_array13(), res[0], res[1], xy, lights, flags, None, mode=mode)
                    clamped += int((plain[..., 1][want[..., 1] == 255] < 255).sum())
    finally:
        sc.set_arith("ieee")
    if lights_key == "case":
        assert clamped > 0                 # the tint drove green channels that were below 255 into the clamp
    if lights_key == "eight":
        assert len(lights) == 8


# ---- 2. the tile list ----
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("name", ["large", "small", "quirk"])
def test_tile_list(torch_mod, name, arith, mode):
    """44 x 70, six tiles (the reference's size, over the right edge, over the bottom edge, unaligned and no multiple of 16 or 4, narrower than a
    quad), offsets out of order with gaps and odd addresses, `data` prefilled; then another list, then the first again (the cache is rebuilt twice)"""
    sc, ms = device_set(name)
    other_off, other_total, other_inside = C.scattered_offsets(C.OTHER_TILES)
    assert len(MT.tile_packets(C.TILES)) == 21 and (C.OFFSETS % 2 == 1).any() and (np.diff(C.OFFSETS) < 0).any()
    sc.set_arith(arith)
    try:
        first = None
        for flags, tint in ((0, None), (AA, None), (AA | REFL, MT.rank_tint(3)), (DEPTH | AA, None)):
            data = check_tiles(ms, name, C.RES, C.TILES, C.OFFSETS, C.TOTAL, C.INSIDE, flags, tint, mode)
            if flags == AA:
                first = data
            # what a tile holds beyond the image is zero: the tile over the bottom edge below row 70, the one over the right edge past column 44
            t3 = data[C.OFFSETS[3]:C.OFFSETS[3] + 3 * 16 * 64].reshape(3, 64, 16)
            t2 = data[C.OFFSETS[2]:C.OFFSETS[2] + 3 * 16 * 64].reshape(3, 64, 16)
            assert not t3[:, 6:, :].any() and not t2[:, :, 12:].any()
        check_tiles(ms, name, C.RES, C.OTHER_TILES, other_off, other_total, other_inside, AA, None, mode)
        again = check_tiles(ms, name, C.RES, C.TILES, C.OFFSETS, C.TOTAL, C.INSIDE, AA, None, mode)
        assert np.array_equal(first, again)
        check_tiles(ms, name, C.RES, C.TILES, C.OFFSETS, C.TOTAL, C.INSIDE, AA, None, mode)       # (a cache hit)
    finally:
        sc.set_arith("ieee")


# ---- 3. the image form ----
@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("name", ["small", "mirror"])
def test_image_form(torch_mod, name, arith, mode):
    sc, ms = device_set(name)
    resx, resy = C.IMAGE_RES
    cam = C.camera(name, C.IMAGE_RES)
    lights = BK.case(name)["lights"]
    pitch = 3 * resx + 5
    sc.set_arith(arith)
    try:
        for flags in (AA, AA | REFL):
            img, st = ms.render_frame_host(cam, resx, resy, lights, flags=flags, pitch=pitch, fill=FILL)
            want, wst = C.tref(name).frame(cam.as_array13(), resx, resy, lights, flags, mode=mode)
            assert img.shape == (resy, pitch) and (img[:, 3 * resx:] == FILL).all()                 # the fill bytes are kept
            bad = np.argwhere((img[:, :3 * resx].reshape(resy, resx, 3) != want).any(axis=2))
            assert want.any() and len(bad) == 0, (flags, len(bad), bad[:5].tolist())
            assert np.array_equal(st, wst), (flags, st, wst)
        for refl in (False, True):                                                                  # without AA4: snail_materials_bounce_image
            a, sa = ms.render_frame_host(cam, resx, resy, lights, flags=REFL if refl else 0, pitch=pitch, fill=FILL)
            b, sb = ms.render_image_host(cam, resx, resy, lights, pitch=pitch, fill=FILL, reflections=refl)
            assert np.array_equal(a, b) and np.array_equal(sa, sb) and (a[:, :3 * resx] != FILL).any()
    finally:
        sc.set_arith("ieee")


# ---- 4. device against device: the header's equivalences ----
IN_IMAGE = np.array([(0, 0, 16, 64), (16, 0, 16, 64), (8, 8, 20, 24), (40, 3, 3, 5), (32, 64, 12, 6)], dtype=np.int32)      # (snail_render_tiles does not clip to the image)


@pytest.mark.parametrize("arith,mode", ARITH)
def test_plain_flags_are_the_bounce_packets(torch_mod, arith, mode):
    torch = torch_mod
    sc, ms = device_set("small")
    res = C.PACKET_RES
    cam = C.camera("small", res)
    lights = BK.case("small")["lights"]
    dxy = torch.from_numpy(np.ascontiguousarray(C.frame_xy(res)[::-1])).to("cuda:0")
    sc.set_arith(arith)
    try:
        for refl in (False, True):
            s1, s2 = sc.new_stats(), sc.new_stats()
            a = ms.frame_packets(cam, res[0], res[1], dxy, lights, flags=REFL if refl else 0, stats=s1).cpu().numpy()
            b = ms.render_packets(cam, res[0], res[1], dxy, lights, stats=s2, reflections=True, flags=0).cpu().numpy() if refl else None
            if not refl:      # snail_materials_bounce_packets_dev with flags 0
                out = torch.zeros((len(dxy), 256, 3), dtype=torch.uint8, device="cuda:0")
                cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32); amb = np.full(3, 0.1, np.float32)
                l7 = np.ascontiguousarray(lights, dtype=np.float32)
                _lib.check(_lib.lib().snail_materials_bounce_packets_dev(ms._h, _lib.ptr(cam13), res[0], res[1], _lib.ptr(dxy), len(dxy), _lib.ptr(l7), len(l7), _lib.ptr(amb), 0,
                                                                         _lib.ptr(out), _lib.ptr(s2), _stream_ptr(None)), "snail_materials_bounce_packets_dev")
                b = out.cpu().numpy()
            assert a.any() and np.array_equal(a, b) and np.array_equal(s1.cpu().numpy(), s2.cpu().numpy()), refl
    finally:
        sc.set_arith("ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("name,flags", [("small", DEPTH), ("small", DEPTH | AA), ("large", DEPTH | AA | REFL), ("degenerate_box", AA), ("degenerate_box", 0)])
def test_tiles_equal_snail_render_tiles(torch_mod, name, flags, arith, mode):
    """depth shading never reaches the full-shading branch, and a set of default materials with flat plane normals shades as simple shading
    does: both are the scene's own tile renderer, bytes and counters"""
    sc, ms = device_set(name)
    resx, resy = C.RES
    cam = C.camera(name, C.RES)
    lights = BK.case(name)["lights"]
    sc.set_arith(arith)
    try:
        got, off, st = ms.render_tiles_host(cam, resx, resy, IN_IMAGE, lights7=lights, flags=flags)
        want, woff, wst = sc.render_tiles_host(cam, resx, resy, IN_IMAGE, lights, flags=flags, color=(1.0, 1.0, 1.0))
    finally:
        sc.set_arith("ieee")
    assert np.array_equal(off, woff) and want.any()
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(st, wst), (st, wst)


# ---- 5. calls on one set take turns ----
@pytest.mark.parametrize("arith,mode", ARITH)
def test_two_threads_on_one_set(torch_mod, arith, mode):
    sc, ms = device_set("quirk")
    resx, resy = C.RES
    cam = C.camera("quirk", C.RES)
    lights = BK.case("quirk")["lights"]
    third = np.ascontiguousarray(C.TILES[::-1][:4])
    jobs = [[(C.TILES, AA, None), (C.OTHER_TILES, AA | REFL, MT.rank_tint(3)), (third, 0, None)],
            [(C.OTHER_TILES, DEPTH | AA, None), (third, AA, MT.rank_tint(15)), (C.TILES, REFL, None)]]
    sc.set_arith(arith)
    try:
        want = [[ms.render_tiles_host(cam, resx, resy, t, lights7=lights, flags=f, tint=tint) for t, f, tint in js] for js in jobs]
        errors = []

        def work(k):
            try:
                for j, (t, f, tint) in enumerate(jobs[k]):
                    got = ms.render_tiles_host(cam, resx, resy, t, lights7=lights, flags=f, tint=tint)
                    if not (np.array_equal(got[0], want[k][j][0]) and np.array_equal(got[2], want[k][j][2])):
                        errors.append((k, j))
            except Exception as e:   # pragma: no cover
                errors.append(repr(e))

        th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for x in th:
            x.start()
        for x in th:
            x.join()
    finally:
        sc.set_arith("ieee")
    assert not errors, errors
    assert all(w[0].any() for ws in want for w in ws)
    # ... and the single-threaded results are the restatement's (the first job of each thread)
    for k in range(2):
        t, f, tint = jobs[k][0]
        planes, wst = C.tref("quirk").tiles(cam.as_array13(), resx, resy, t, lights, f, tint, mode=mode)
        assert np.array_equal(want[k][0][0], np.concatenate(planes)) and np.array_equal(want[k][0][2], wst)


# ---- 6. the adapter ----
def write_mock_inputs(d, name, arith):
    from snail_amd import HostBVH
    from snail_amd import materials as P
    c = BK.case(name)
    _, ms = device_set(name)
    hb = HostBVH.build(c["tv"])
    hb.nodes.tofile(str(d / "nodes.bin")); hb.tris.tofile(str(d / "tris.bin"))
    ms.shtris.tofile(str(d / "shtris.bin"))
    np.asarray(c["material_map"], dtype=np.int32).tofile(str(d / "matmap.bin"))
    mats = [P.Material.simple(m[1], m[2]) if m[0] == "simple" else P.Material.textured(m[1], m[2]) if m[0] == "tex" else P.Material.uber(m[1], m[2], m[3]) for m in c["descs"]]
    P._material_records(mats).tofile(str(d / "mats.bin"))
    dims = []
    for k, t in enumerate(c["textures"]):
        tx = P.Texture(t)
        tx.levels.tofile(str(d / ("tex%d.bin" % k)))
        dims += [tx.width, tx.height]
    np.ascontiguousarray(C.camera(name, C.RES).as_array13(), dtype=np.float32).tofile(str(d / "cam.bin"))
    np.ascontiguousarray(C.camera(name, C.IMAGE_RES).as_array13(), dtype=np.float32).tofile(str(d / "cam_img.bin"))
    np.ascontiguousarray(c["lights"], dtype=np.float32).tofile(str(d / "lights7.bin"))
    C.TILES.astype(np.int32).tofile(str(d / "tiles.bin")); C.OFFSETS.astype(np.int32).tofile(str(d / "offsets.bin"))
    np.array([C.RES[0], C.RES[1], int(arith == "host_sse"), hb.depth, C.IMAGE_RES[0], C.IMAGE_RES[1], len(c["textures"])] + dims, dtype=np.int32).tofile(str(d / "meta.bin"))


@pytest.mark.parametrize("arith,mode", ARITH)
def test_cpp_adapter_routes_gvals6_to_the_device(torch_mod, tmp_path, arith, mode):
    """A C++ host in the reference's shape (tests/cpp/materials_mock.cpp built with SNAIL_ADAPTER_DEVICE_MATERIALS): with gVals[6] and an attached set
    the tile list with gVals[8] (rank 3) and gVals[9] and the image with gVals[7] equal the restatement, TreeStats too; without an attached set,
    with gVals[5] and no gVals[1], and for an image with gVals[8] the mock's host renderer is reached instead (the mock counts)."""
    from tests.test_materials_tiles_host import build_materials_mock
    name = "small"
    write_mock_inputs(tmp_path, name, arith)
    r = subprocess.run([build_materials_mock(tmp_path, True), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "materials adapter ok (with SNAIL_ADAPTER_DEVICE_MATERIALS), host renderer reached 5 times" in r.stdout, r.stdout + r.stderr
    stats = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in open(str(tmp_path / "stats.txt")).read().splitlines()}
    lights = BK.case(name)["lights"]
    want, wst = C.tref(name).tiles(C.camera(name, C.RES).as_array13(), C.RES[0], C.RES[1], C.TILES, lights, AA, MT.rank_tint(3), mode=mode)
    raw = np.fromfile(str(tmp_path / "out_tiles.bin"), dtype=np.uint8)
    inside = np.zeros(len(raw), dtype=bool)
    for k, w in enumerate(want):
        assert np.array_equal(raw[C.OFFSETS[k]:C.OFFSETS[k] + len(w)], w), k
        inside[C.OFFSETS[k]:C.OFFSETS[k] + len(w)] = True
    assert (raw[~inside] == FILL).all() and (~inside).sum() > 0
    assert stats["tiles"] == [int(x) for x in wst], (stats["tiles"], wst)
    resx, resy = C.IMAGE_RES
    wf, wfs = C.tref(name).frame(C.camera(name, C.IMAGE_RES).as_array13(), resx, resy, lights, REFL, mode=mode)
    img = np.fromfile(str(tmp_path / "out_img.bin"), dtype=np.uint8).reshape(resy, 3 * resx + 5)
    assert np.array_equal(img[:, :3 * resx].reshape(resy, resx, 3), wf) and (img[:, 3 * resx:] == FILL).all()
    assert stats["img"] == [int(x) for x in wfs], (stats["img"], wfs)


def test_cpp_adapter_without_the_macro_keeps_the_host_renderer(torch_mod, tmp_path):
    from tests.test_materials_tiles_host import build_materials_mock
    write_mock_inputs(tmp_path, "small", "ieee")
    r = subprocess.run([build_materials_mock(tmp_path, False), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "materials adapter ok (without SNAIL_ADAPTER_DEVICE_MATERIALS), host renderer reached 7 times" in r.stdout, r.stdout + r.stderr


# ---- 7. refusals with a live set ----
def test_refusals_leave_the_buffer_alone(torch_mod):
    sc, ms = device_set("small")
    cam = C.camera("small", C.RES)
    lights = BK.case("small")["lights"]
    nine = np.tile(lights[:1], (9, 1))
    bad_tile = C.TILES.copy(); bad_tile[2, 2] = 0
    for flags, ls, tl, tint, what in ((8, lights, C.TILES, None, "flags"), (AA, nine, C.TILES, None, "lights"), (AA, lights, bad_tile, None, "rect"),
                                      (AA, lights, C.TILES, [0.6, np.nan, 1.0], "tint")):
        data = np.full(C.TOTAL, FILL, dtype=np.uint8)
        with pytest.raises(_lib.SnailError, match=what):
            ms.render_tiles_host(cam, C.RES[0], C.RES[1], tl, C.OFFSETS, ls, flags=flags, tint=tint, data=data)
        assert (data == FILL).all(), what
    with pytest.raises(_lib.SnailError, match="flags"):
        ms.render_frame_host(cam, 35, 25, lights, flags=16 | AA)
    # the older frame functions keep refusing what they refused
    with pytest.raises(_lib.SnailError, match="flags"):
        ms.render(cam, 35, 25, lights, flags=AA)
    with pytest.raises(_lib.SnailError, match="flags"):
        ms.render(cam, 35, 25, lights, flags=DEPTH, reflections=True)
    # nTiles <= 0 and nPackets <= 0 return 0
    data, _, st = ms.render_tiles_host(cam, C.RES[0], C.RES[1], np.zeros((0, 4), np.int32), lights7=lights, flags=AA)
    assert len(data) == 0 and not st.any()
    # the set still renders
    check_tiles(ms, "small", C.RES, C.TILES, C.OFFSETS, C.TOTAL, C.INSIDE, AA, None, O.MODE_IEEE)
