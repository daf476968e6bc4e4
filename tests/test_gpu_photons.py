"""The photon pass of include/snail_wide.h (TracePhotons, src/photons.cpp:239-249): records and their stable compaction.  The expected
records are computed in NumPy (tests/wide_ref.py: photons) from the DEVICE's own distances, which tests/test_gpu_wide.py holds to the walk."""
import numpy as np
import pytest
import torch

from snail_amd import HostBVH, _lib, photons, scenes
from snail_amd.scene import Scene
from tests import wide_ref as WR

pytestmark = pytest.mark.gpu

FILL = 0xA5


@pytest.fixture(scope="module")
def box():
    """the box with its faces turned inwards: every ray from inside hits"""
    sc = Scene(HostBVH.build(scenes.box_scene(flip=False)), 0)
    yield sc
    sc.close()


def rays_of(lights7, count, seed, spread=0.2, aim=None):
    o, d = [], []
    for k, l in enumerate(np.asarray(lights7, dtype=np.float32).reshape(-1, 7)):
        oo, dd = photons.emit(l[:3], count, seed + k)
        oo = (l[:3] + (oo - l[:3]) * np.float32(spread)).astype(np.float32)
        if aim is not None:
            dd = aim(dd)
        o.append(oo); d.append(dd)
    return np.ascontiguousarray(np.concatenate(o)), np.ascontiguousarray(np.concatenate(d))


def trace(sc, o, d, lights7, count):
    """-> (records written, the whole output buffer as bytes, device distances, stats of the photon call)"""
    dev = sc._dev()
    do, dd = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    n = len(o)
    out = torch.full((max(n, 1), 32), FILL, dtype=torch.uint8, device=dev)
    npho = torch.full((1,), -3, dtype=torch.int32, device=dev)
    stats = torch.zeros(2, dtype=torch.int64, device=dev)
    sc.trace_photons(do, dd, lights7, count, out=out, n_photons=npho, stats=stats)
    dist = torch.full((n,), float("inf"), dtype=torch.float32, device=dev)
    st2 = torch.zeros(2, dtype=torch.int64, device=dev)
    if n:
        sc.wide_trace(do, dd, dist, stats=st2)
    torch.cuda.synchronize()
    assert stats.cpu().tolist() == st2.cpu().tolist()
    k = int(npho.cpu()[0])
    raw = out.cpu().numpy()
    return raw[:k].copy().view(photons.PHOTON).reshape(-1), raw, dist.cpu().numpy(), k


def check(sc, o, d, lights7, count):
    got, raw, dist, k = trace(sc, o, d, lights7, count)
    want = WR.photons(o, d, dist, lights7, count, photons.PHOTON)
    assert k == len(want), (k, len(want))
    assert got.tobytes() == want.tobytes()
    assert (raw[k:] == FILL).all()          # nothing past the records written is touched
    return got, dist


@pytest.mark.parametrize("count", [1, 63, 64, 65, 4097, 70001])
def test_every_ray_from_inside_leaves_a_photon(box, count):
    l7 = [[0.1, -0.2, 0.05, 0.5, 0.25, 1.0, 10.0]]
    o, d = rays_of(l7, count, seed=count)
    got, dist = check(box, o, d, l7, count)
    assert len(got) == count and np.isfinite(dist).all() and (dist > 0).all()
    assert (got["color"] == [127, 63, 255, 0]).all() and (got["temp"] == 1).all()


def test_a_light_outside_aimed_away_leaves_none(box):
    l7 = [[50.0, 0.0, 0.0, 1.0, 1.0, 1.0, 10.0]]

    def away(d):
        d = d.copy()
        d[:, 0] = np.abs(d[:, 0]) + np.float32(0.01)
        return d
    o, d = rays_of(l7, 300, seed=2, aim=away)
    got, raw, dist, k = trace(box, o, d, l7, 300)
    assert k == 0 and np.isinf(dist).all() and (raw == FILL).all()


def test_mixed_hits_keep_ray_order(box):
    l7 = [[2.5, 0.3, -0.2, 1.0, 1.0, 1.0, 10.0]]       # outside: some rays enter the box, most miss; offsets up to 2 units put some origins inside
    o, d = rays_of(l7, 5000, seed=9, spread=1.0)
    # rays are an input: the first 600 start inside (all hit), the next 600 point away from far outside (none hits)
    o[:600], d[:600] = rays_of([[0.0, 0.0, 0.0, 1, 1, 1, 1]], 600, seed=10)
    o[600:1200] = [50.0, 0.0, 0.0]
    d[600:1200, 0] = np.abs(d[600:1200, 0]) + np.float32(0.01)
    got, dist = check(box, o, d, l7, 5000)
    keep = np.flatnonzero(~np.isinf(dist))
    assert 700 < len(keep) < 4000
    assert np.array_equal(got["direction"], d[keep])     # stable: the survivors in ray order
    # blocks of 256 rays with no survivor, with some, and full ones all occur
    per_block = np.bincount(keep // 256, minlength=(5000 + 255) // 256)
    assert (per_block == 0).any() and (per_block == 256).any() and len(set(per_block.tolist())) >= 5


def test_two_lights_are_light_major_and_the_colour_rule(box):
    l7 = [[0.0, 0.0, 0.0, 2.0, -1.0, np.nan, 10.0], [0.3, 0.2, -0.1, 0.5, 0.999, 1.0, 10.0]]
    o, d = rays_of(l7, 333, seed=4)
    got, dist = check(box, o, d, l7, 333)
    assert len(got) == 666
    assert (got["color"][:333] == [255, 0, 0, 0]).all() and (got["color"][333:] == [127, 254, 255, 0]).all()


def test_the_host_form(box):
    l7 = [[2.5, 0.3, -0.2, 0.5, 0.5, 0.5, 10.0], [0.0, 0.0, 0.0, 1.0, 0.0, 0.25, 5.0]]
    o, d = rays_of(l7, 700, seed=12, spread=1.0)
    got, raw, dist, k = trace(box, o, d, l7, 700)
    rec, st = box.trace_photons_host(o, d, l7, 700)
    assert len(rec) == k and rec.tobytes() == got.tobytes() and st[0] > 0 and st[1] > 0
    rec0, st0 = box.trace_photons_host(o[:0], d[:0], l7[:0], 700)
    assert len(rec0) == 0
    with pytest.raises(_lib.SnailError, match="9 lights outside 0..8"):
        box.trace_photons_host(np.zeros((9, 3), np.float32), np.zeros((9, 3), np.float32), np.zeros((9, 7), np.float32), 1)
