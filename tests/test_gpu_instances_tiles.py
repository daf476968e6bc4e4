"""The tile renderer of instanced scenes on the MI355X (snail_instances_render_tiles / _render_frame / _shade_packets_dev): planar tiles and
frames byte for byte and TreeStats for equality against the test-side restatement tests/dbvh_tiles_ref.py, in both arithmetics, and -- without
the restatement -- against the merged lit-frame and depth paths.  The cases are those of tests/instances_shade_cases.py at small resolutions,
chosen with the restatement alone; what each must exercise is asserted on the restatement's own output."""
import os
import subprocess
import threading

import numpy as np
import pytest

from snail_amd import _lib
from snail_amd.instances import InstancedScene
from snail_amd.render import divide_image
from tests import dbvh_ref as R
from tests import dbvh_shade_ref as S
from tests import dbvh_tiles_ref as T
from tests import instances_shade_cases as K
from tests import oracle_lib as O
from tests.test_gpu_instances import ARITH, blas, set_arith
from tests.test_gpu_instances_shade import device_scene, torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu

AA, REFL, DEPTH = T.AA4, T.REFLECTIONS, T.DEPTH
RES = {"field": (64, 48), "deep": (64, 64), "inside": (64, 48)}
_cases = {}


def case(name):
    """the case, its InstancedScene and ONE restatement object per case (its memo is shared by the tests of this module)"""
    if name not in _cases:
        names, rot, tr, bi, _, _, cam, lights, cref = K.case(name)
        isc, ref = device_scene(names, rot, tr, bi, cref)
        _cases[name] = (isc, T.TilesRef(ref), cam, lights, names, rot, tr, bi)
    return _cases[name]


def conditions(tref, cam, resx, resy, lights, flags, mode):
    """the frame exercises what the comparison claims (counted over the samples the flags trace: 4 per pixel with AA)"""
    d = S.Diag()
    tref.colors(cam.as_array13(), resx, resy, S.frame_packets(resx, resy), lights, flags, mode=mode, diag=d)
    samples = resx * resy * (4 if flags & AA else 1)
    assert d.hit_pixels >= samples // 5, (d.hit_pixels, samples)
    if not flags & DEPTH:
        assert d.lit_pixels >= 100 and d.occluded_pixels >= 100, (d.lit_pixels, d.occluded_pixels)
    if flags & REFL and not flags & DEPTH:
        assert d.mirrored_hits >= 100, d.mirrored_hits


def check_tiles(isc, tref, cam, resx, resy, tiles, lights, flags, tint, mode, offsets=None, data=None):
    got, off, st = isc.render_tiles_host(cam, resx, resy, tiles, lights, flags=flags, tint=tint, offsets=offsets, data=data)
    want, wst = tref.tiles(cam.as_array13(), resx, resy, tiles, lights, flags, tint, mode=mode)
    t = np.asarray(tiles).reshape(-1, 4)
    for k, (x, y, w, h) in enumerate(t.tolist()):
        g = got[off[k]:off[k] + 3 * w * h]
        bad = np.flatnonzero(g != want[k])
        assert len(bad) == 0, ("tile", k, (x, y, w, h), "flags", flags, len(bad), bad[:5].tolist(), g[bad[:5]].tolist(), want[k][bad[:5]].tolist())
    assert np.array_equal(st, wst), (flags, st, wst)
    return got, off, st


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("flags,rank", [(AA, None), (AA | REFL, None), (AA | DEPTH, None), (AA, 3)], ids=["aa", "aa_reflections", "aa_depth", "aa_tint3"])
def test_field_tile_list_and_frame_equal_the_restatement(torch_mod, flags, rank, arith, mode):
    isc, tref, cam, lights = case("field")[:4]
    resx, resy = RES["field"]
    set_arith(isc, arith)
    conditions(tref, cam, resx, resy, lights, flags, mode)
    tint = None if rank is None else T.rank_tint(rank)
    got, off, st = check_tiles(isc, tref, cam, resx, resy, divide_image(resx, resy), lights, flags, tint, mode)
    plain = isc.render_tiles_host(cam, resx, resy, divide_image(resx, resy), lights, flags=flags & ~AA)[0]
    assert not np.array_equal(got, plain)                     # (the antialiased, or tinted, tiles are other tiles)
    if rank is not None:
        assert not np.array_equal(got, isc.render_tiles_host(cam, resx, resy, divide_image(resx, resy), lights, flags=flags)[0])
    else:
        img, ist = isc.render_frame_host(cam, resx, resy, lights, flags=flags)
        wf, wfs = tref.frame(cam.as_array13(), resx, resy, lights, flags, mode=mode)
        bad = np.argwhere((img != wf).any(axis=2))
        assert len(bad) == 0, (len(bad), bad[:5].tolist())
        assert np.array_equal(ist, wfs)
        assert ist[2] >= 4 * 256 * len(S.frame_packets(resx, resy))          # traced rays: four times the plain primary count, plus secondary rays
    set_arith(isc, "ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("name", ["deep", "inside"])
def test_deep_blas_and_a_camera_inside(torch_mod, name, arith, mode):
    """chain + box: the DEEP inner walk under the double-resolution packets; inside: the camera in the middle of an instance"""
    if name == "deep":
        assert blas("chain")[1].depth > 62
    isc, tref, cam, lights = case(name)[:4]
    resx, resy = RES[name]
    set_arith(isc, arith)
    conditions(tref, cam, resx, resy, lights, AA | REFL, mode)
    check_tiles(isc, tref, cam, resx, resy, divide_image(resx, resy), lights, AA | REFL, None, mode)
    set_arith(isc, "ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
def test_plain_tiles_equal_the_merged_paths(torch_mod, arith, mode):
    """Independent of the restatement: without antialiasing and tint the tile bytes are the planar encoding of the frames the merged entry
    points make, and the packet call is snail_instances_render_whitted_packets_dev."""
    torch = torch_mod
    isc, tref, cam, lights = case("field")[:4]
    resx, resy = RES["field"]
    set_arith(isc, arith)
    tiles = divide_image(resx, resy)
    for flags in (0, REFL, DEPTH):
        if flags == DEPTH:
            frame = isc.render_depth(cam, resx, resy).cpu().numpy()
        else:
            frame = isc.render_whitted(cam, resx, resy, lights, reflections=flags == REFL).cpu().numpy()
        assert (frame.reshape(-1, 3).max(axis=1) > 0).sum() >= resx * resy // 5
        got, off, _ = isc.render_tiles_host(cam, resx, resy, tiles, lights, flags=flags)
        for k, w in enumerate(O.planar_encode(frame, tiles)):
            assert np.array_equal(got[off[k]:off[k] + len(w)], w), (flags, k)
        img, _ = isc.render_frame_host(cam, resx, resy, lights, flags=flags)
        assert np.array_equal(img, frame), flags
    xy = S.frame_packets(resx, resy)
    sub = np.ascontiguousarray(xy[np.random.default_rng(7).permutation(len(xy))[: len(xy) // 2]])
    dxy = torch.from_numpy(sub).cuda()
    for refl in (False, True):
        s1, s2 = isc.new_stats(), isc.new_stats()
        a = isc.shade_packets(cam, resx, resy, dxy, lights, flags=REFL if refl else 0, stats=s1).cpu().numpy()
        b = isc.render_whitted_packets(cam, resx, resy, dxy, lights, stats=s2, reflections=refl).cpu().numpy()
        assert np.array_equal(a, b) and a.any() and np.array_equal(s1.cpu().numpy(), s2.cpu().numpy())
    # ... and with every switch on, the packet call is the restatement's
    st = isc.new_stats()
    a = isc.shade_packets(cam, resx, resy, dxy, lights, flags=AA | REFL, tint=T.rank_tint(15), stats=st).cpu().numpy()
    w, wst = tref.packets(cam.as_array13(), resx, resy, sub, lights, AA | REFL, T.rank_tint(15), mode=mode)
    assert np.array_equal(a, w) and np.array_equal(st.cpu().numpy().astype(np.uint64), wst)
    set_arith(isc, "ieee")


# 90 x 53: no dimension a multiple of 16 or 4.  A 16x64 tile (its last rows below the image), an 8-wide tile, a 24-high tile, a tile that the
# right and bottom edges clip, unaligned corners; out of raster order
AWKWARD = np.array([[64, 32, 40, 30], [0, 0, 16, 64], [37, 5, 8, 19], [16, 11, 21, 24], [48, 0, 16, 16]], dtype=np.int32)


@pytest.mark.parametrize("arith,mode", ARITH)
def test_awkward_tile_lists(torch_mod, arith, mode):
    isc, tref, cam, lights = case("field")[:4]
    resx, resy = 90, 53
    set_arith(isc, arith)
    size = 3 * AWKWARD[:, 2].astype(np.int64) * AWKWARD[:, 3]
    gaps = np.array([3, 1, 7, 2, 5], dtype=np.int64)
    offsets = (np.concatenate([[0], np.cumsum(size + gaps)[:-1]]) + 2).astype(np.int64)       # gaps of 2, 3, 1, 7, 2 and 5 bytes around the tiles
    total = int(offsets[-1] + size[-1] + gaps[-1])
    inside = np.zeros(total, dtype=bool)
    for o, n in zip(offsets.tolist(), size.tolist()):
        inside[o:o + n] = True
    for flags in (REFL, AA):
        conditions(tref, cam, resx, resy, lights, flags, mode)
        data = np.full(total, 0xAB, dtype=np.uint8)
        got, _, _ = check_tiles(isc, tref, cam, resx, resy, AWKWARD, lights, flags, T.rank_tint(5) if flags & AA else None, mode, offsets=offsets, data=data)
        assert got is data and (data[~inside] == 0xAB).all() and (~inside).sum() == 2 + gaps.sum()
        check_tiles(isc, tref, cam, resx, resy, divide_image(resx, resy), lights, flags, None, mode)
    set_arith(isc, "ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
def test_tile_list_cache(torch_mod, arith, mode):
    isc, tref, cam, lights = case("field")[:4]
    set_arith(isc, arith)
    a, b = divide_image(64, 48), np.ascontiguousarray(divide_image(64, 48)[::-1][:3])
    a1 = check_tiles(isc, tref, cam, 64, 48, a, lights, AA, None, mode)[0]
    check_tiles(isc, tref, cam, 64, 48, b, lights, AA, None, mode)
    check_tiles(isc, tref, cam, 90, 53, AWKWARD, lights, AA, None, mode)            # a second resolution in between
    a2 = check_tiles(isc, tref, cam, 64, 48, a, lights, AA, None, mode)[0]
    a3 = check_tiles(isc, tref, cam, 64, 48, a, lights, AA, None, mode)[0]          # (a cache hit)
    assert np.array_equal(a1, a2) and np.array_equal(a1, a3)
    set_arith(isc, "ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
def test_update_between_two_tile_list_frames(torch_mod, arith, mode):
    names, rot, tr, bi, _, _, cam, lights, cref = K.case("field")
    resx, resy = 64, 48
    isc, ref1 = device_scene(names, rot, tr, bi, cref)
    set_arith(isc, arith)
    tiles = divide_image(resx, resy)
    g1, off, st1 = isc.render_tiles_host(cam, resx, resy, tiles, lights, flags=AA)
    rot2, tr2, bi2 = K.layout(names, 40, 77, 0.1)          # instances moved, count grown past the handle's buffers
    isc.update(rot2, tr2, bi2)
    g2, _, st2 = isc.render_tiles_host(cam, resx, resy, tiles, lights, flags=AA)
    xs, bs = isc.slot_transforms()
    ref2 = R.Ref([blas(nm)[1] for nm in names], isc.nodes(), xs, bs)
    for g, st, ref in ((g1, st1, case("field")[1]), (g2, st2, T.TilesRef(ref2))):
        want, wst = ref.tiles(cam.as_array13(), resx, resy, tiles, lights, AA, mode=mode)
        assert np.array_equal(g, np.concatenate(want)) and np.array_equal(st, wst)
    assert not np.array_equal(g1, g2)
    set_arith(isc, "ieee")
    isc.close()


@pytest.mark.parametrize("arith,mode", ARITH)
def test_four_threads_render_tile_lists_on_one_handle(torch_mod, arith, mode):
    isc, tref, cam, lights = case("field")[:4]
    resx, resy = 64, 48
    set_arith(isc, arith)
    full = divide_image(resx, resy)
    jobs = [(full, AA, None), (np.ascontiguousarray(full[::-1]), REFL, None), (np.ascontiguousarray(full[1:]), AA | DEPTH, T.rank_tint(3)),
            (np.ascontiguousarray(full[:2]), AA, T.rank_tint(15))]
    want = [np.concatenate(tref.tiles(cam.as_array13(), resx, resy, t, lights, f, tint, mode=mode)[0]) for t, f, tint in jobs]
    errors = []

    def work(k):
        try:
            for j in (k, (k + 1) % 4):
                t, f, tint = jobs[j]
                got = isc.render_tiles_host(cam, resx, resy, t, lights, flags=f, tint=tint)[0]
                if not np.array_equal(got, want[j]):
                    errors.append((k, j))
        except Exception as e:   # pragma: no cover
            errors.append(repr(e))

    th = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    set_arith(isc, "ieee")
    assert not errors, errors


@pytest.mark.parametrize("arith,mode", ARITH)
def test_cpp_adapter_tile_list(torch_mod, tmp_path, arith, mode):
    """A C++ host in the reference's shape (tests/cpp/instances_tiles_mock.cpp, SNAIL_ADAPTER_INSTANCED_TILES): the tile-list Render with gVals[9],
    with gVals[9] + gVals[8] at rank 3, and with gVals[1], and the image Render with gVals[9], stay on the device -- bytes and TreeStats equal the
    restatement's; gVals[5] reaches the host renderer (a stub) over a prefetched frame (the mock checks that itself)."""
    from tests.test_instances_tiles_host import build_tiles_mock
    isc, tref, cam, lights, names = case("field")[:5]
    resx, resy = RES["field"]
    d = tmp_path
    for k, nm in enumerate(names):
        hb = blas(nm)[0].bvh
        hb.nodes.tofile(str(d / ("blas%d_nodes.bin" % k))); hb.tris.tofile(str(d / ("blas%d_tris.bin" % k)))
    xs, bs = isc.slot_transforms()
    isc.nodes().tofile(str(d / "top_nodes.bin")); xs.tofile(str(d / "xf12.bin")); bs.astype(np.int32).tofile(str(d / "blas_index.bin"))
    np.ascontiguousarray(cam.as_array13(), dtype=np.float32).tofile(str(d / "cam.bin"))
    np.ascontiguousarray(lights, dtype=np.float32).tofile(str(d / "lights7.bin"))
    tiles = divide_image(resx, resy)
    tiles.astype(np.int32).tofile(str(d / "tiles.bin"))
    depths = [blas(nm)[0].bvh.depth for nm in names]
    np.array([resx, resy, int(arith == "host_sse"), len(names)] + depths, dtype=np.int32).tofile(str(d / "meta.bin"))
    r = subprocess.run([build_tiles_mock(tmp_path), str(d)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "instances tiles adapter ok" in r.stdout, r.stdout + r.stderr
    assert "Render called" not in r.stdout
    stats = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in open(str(d / "stats.txt")).read().splitlines()}
    for key, fname, flags, tint in (("aa", "out_aa.bin", AA, None), ("tint", "out_tint.bin", AA, T.rank_tint(3)), ("depth", "out_depth.bin", DEPTH, None)):
        want, wst = tref.tiles(cam.as_array13(), resx, resy, tiles, lights, flags, tint, mode=mode)
        raw = np.fromfile(str(d / fname), dtype=np.uint8)
        pos = 0
        for k, w in enumerate(want):
            assert np.array_equal(raw[pos:pos + len(w)], w), (key, k)
            assert (raw[pos + len(w):pos + len(w) + 5] == 0xAB).all()           # the gap after every tile keeps its fill
            pos += len(w) + 5
        assert pos == len(raw) and stats[key] == [int(x) for x in wst], (key, stats[key], wst)
    wf, wfs = tref.frame(cam.as_array13(), resx, resy, lights, AA, mode=mode)
    raw = np.fromfile(str(d / "out_img_aa.bin"), dtype=np.uint8).reshape(resy, resx * 3 + 1)
    assert np.array_equal(raw[:, :resx * 3].reshape(resy, resx, 3), wf) and (raw[:, resx * 3:] == 0xAB).all()
    assert stats["img_aa"] == [int(x) for x in wfs]


def test_refusals_leave_the_buffer_alone(torch_mod):
    isc, tref, cam, lights = case("field")[:4]
    tiles = divide_image(64, 48)
    fill = lambda: np.full(3 * 64 * 48, 0xAB, dtype=np.uint8)
    nine = np.tile(lights[:1], (9, 1))
    bad_tile = tiles.copy(); bad_tile[2, 2] = 0
    for flags, ls, tl, tint, what in ((8, lights, tiles, None, "flags"), (AA, nine, tiles, None, "lights"), (AA, lights, bad_tile, None, "rect"),
                                      (AA, lights, tiles, [0.6, np.nan, 1.0], "tint")):
        data = fill()
        with pytest.raises(_lib.SnailError, match=what):
            isc.render_tiles_host(cam, 64, 48, tl, ls, flags=flags, tint=tint, data=data)
        assert (data == 0xAB).all(), what
    # a null `data`
    cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32); v3 = np.ones(3, np.float32)
    off = np.zeros(len(tiles), np.int64)
    rc = _lib.lib().snail_instances_render_tiles(isc._h, _lib.ptr(cam13), 64, 48, _lib.ptr(tiles), _lib.ptr(off), len(tiles), None, 0, _lib.ptr(v3), _lib.ptr(v3), 0, None,
                                                 None, None)
    assert rc != 0 and b"null buffer" in _lib.lib().snail_last_error()
    with pytest.raises(_lib.SnailError, match="flags"):
        isc.render_frame_host(cam, 64, 48, lights, flags=16 | AA)
    # the handle still renders
    check_tiles(isc, tref, cam, 64, 48, tiles, lights, AA, None, O.MODE_IEEE)
