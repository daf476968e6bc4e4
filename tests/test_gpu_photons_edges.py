"""The photon pass of include/snail_wide.h at its edges (cases: tests/wide_edge_cases.py; what they reach: tests/test_wide_edges_host.py):
more than 1024 blocks, so that the scan's carry is handed from round to round -- with the kept rays laid out by a pattern the test
knows, which pins the compaction independently of the walk --; distances that are NaN, -inf and negative, which all leave a record;
a preset d_stats; and the eight event-guarded scratch slots taken round by calls in flight on two streams."""
import numpy as np
import pytest
import torch

from snail_amd import HostBVH, photons, scenes
from snail_amd.scene import Scene
from tests import wide_edge_cases as EC
from tests import wide_ref as WR

pytestmark = pytest.mark.gpu

FILL = 0xA5
L7 = [[0.1, -0.2, 0.05, 0.5, 0.25, 1.0, 10.0], [0.3, 0.2, -0.1, 1.0, 0.5, 0.999, 10.0]]


def inward_box():
    """the box with its faces turned inwards: every ray from inside hits"""
    return Scene(HostBVH.build(scenes.box_scene(flip=False)), 0)


@pytest.fixture(scope="module")
def box():
    sc = inward_box()
    yield sc
    sc.close()


def buffers(dev, n, preset=(0, 0)):
    return (torch.full((max(n, 1), 32), FILL, dtype=torch.uint8, device=dev), torch.full((1,), -3, dtype=torch.int32, device=dev),
            torch.tensor(list(preset), dtype=torch.int64, device=dev))


def trace(sc, o, d, lights7, count, preset=(0, 0)):
    """-> (records written, the whole output buffer as bytes, the device's own distances, the photon call's stats minus `preset`)"""
    dev = sc._dev()
    do, dd = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    n = len(o)
    out, npho, stats = buffers(dev, n, preset)
    sc.trace_photons(do, dd, lights7, count, out=out, n_photons=npho, stats=stats)
    dist = torch.full((n,), float("inf"), dtype=torch.float32, device=dev)
    st2 = torch.zeros(2, dtype=torch.int64, device=dev)
    sc.wide_trace(do, dd, dist, stats=st2)
    torch.cuda.synchronize()
    assert stats.cpu().tolist() == [preset[0] + int(st2[0]), preset[1] + int(st2[1])]      # d_stats is ADDED to
    k = int(npho.cpu()[0])
    raw = out.cpu().numpy()
    assert 0 <= k <= n and (raw[k:] == FILL).all()          # nothing past the records written is touched
    return raw[:k].copy().view(photons.PHOTON).reshape(-1), raw, dist.cpu().numpy(), st2.cpu().numpy()


def check_pattern(sc, name, seed):
    lights, count = EC.PHOTON_SIZES[name]
    hit = EC.photon_pattern(name)
    o, d = EC.photon_rays(hit, seed)
    l7 = L7[:lights]
    got, raw, dist, _ = trace(sc, o, d, l7, count)
    kept = np.flatnonzero(hit)
    # the compaction, from the pattern alone: that many records, the kept rays' directions in ray order, each light's colour
    assert len(got) == len(kept), (name, len(got), len(kept))
    assert got["direction"].tobytes() == d[kept].tobytes()
    colours = np.stack([WR.photon_colour(l[3:6]) for l in l7])
    assert np.array_equal(got["color"], colours[kept // count]) and (got["temp"] == 1).all()
    # the walk kept what the pattern says, and the records are TracePhotons' over the device's own distances
    assert np.array_equal(np.flatnonzero(~(dist == np.inf)), kept)
    want = WR.photons(o, d, dist, l7, count, photons.PHOTON)
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("name", list(EC.PHOTON_SIZES))
def test_the_scan_hands_its_carry_on(box, name):
    check_pattern(box, name, seed=len(name))


def odd_case():
    o, d = EC.odd_photon_rays()
    b = EC.bvh("two")
    dist, visits = WR.wide_trace(b.nodes, b.tris, o, d, np.full(len(o), np.inf, dtype=np.float32))
    l7 = [[0.0, 0.0, 0.0, 1.0, 0.5, 0.25, 1.0]]
    return o, d, l7, dist, visits, WR.photons(o, d, dist, l7, len(o), photons.PHOTON)


def check_odd(sc):
    o, d, l7, wdist, wvisits, want = odd_case()
    preset = (2 ** 40 + 5, 7)
    got, raw, dist, st = trace(sc, o, d, l7, len(o), preset=preset)
    assert EC.same_floats(dist, wdist) and st.tolist() == wvisits.astype(np.int64).sum(axis=0).tolist()
    # NaN, -inf and negative distances leave a record; only +inf leaves none
    assert len(got) == len(want) == int((~(wdist == np.inf)).sum()) and len(want) > int(np.isfinite(wdist).sum())
    bad = EC.float_mismatches(got["position"], want["position"])
    assert len(bad) == 0, (bad[:8], got["position"].reshape(-1)[bad[:8]], want["position"].reshape(-1)[bad[:8]])
    assert np.isnan(got["position"]).any() and np.isfinite(got["position"]).all(axis=1).any()
    for field in ("direction", "color", "temp"):
        assert got[field].tobytes() == want[field].tobytes(), field
    # ... against the two mutations of the keep rule
    for m in WR.PHOTON_MUTATIONS:
        assert len(WR.photons(o, d, wdist, l7, len(o), photons.PHOTON, mutation=m)) < len(got)


def test_nan_minus_inf_and_negative_distances_leave_a_record():
    sc = Scene(EC.bvh("two"), 0)
    try:
        check_odd(sc)
    finally:
        sc.close()


@pytest.mark.parametrize("arith", ["ieee", "host_sse"])
def test_in_both_arithmetics(arith):
    """the pass is compiled once, outside the arithmetic namespaces: the scene's mode changes nothing"""
    sc, box = Scene(EC.bvh("two"), 0), inward_box()
    try:
        sc.set_arith(arith)
        box.set_arith(arith)
        check_odd(sc)
        check_pattern(box, "one_block_more", seed=3)
    finally:
        sc.close()
        box.close()


# ---- the scratch: eight event-guarded slots, SnailScene::wide[wideCount++ % 8], grown when a larger launch arrives ----
# (which call takes which slot, with how many rays, on which stream: wide_edge_cases.slot_plan)
def slot_rays(i):
    n = EC.slot_plan(i)[0]
    hit = np.random.RandomState(900 + i).randint(0, 3, size=n) > 0
    return EC.photon_rays(hit, 950 + i) + (int(hit.sum()),)


def probe_rays(i):
    """the rays of a wide_trace call between two photon calls: some start with a distance"""
    o, d = EC.photon_rays(np.random.RandomState(800 + i).randint(0, 2, size=1000).astype(bool), 850 + i)
    dist = np.full(1000, np.inf, dtype=np.float32)
    dist[::5] = np.float32(0.25)
    return o, d, dist


@pytest.mark.parametrize("interleave", [False, True], ids=["photons", "photons_and_walks"])
def test_twenty_calls_in_flight_on_two_streams(interleave):
    """20 calls, no host synchronisation between them, on two streams in turn; the counts cycle through 300, 70 001, 5 and 4 097.  slot_plan()
    shifts both cycles at every turn round the eight slots, so every slot's next user is on the other stream (the wait for the slot's
    event orders what stream order does not) and half the slots grow after they have been used (tests/test_wide_edges_host.py asserts both
    from i alone).  Every call's output, count and stats are those of the same rays alone on a fresh scene, the fill bytes past the count
    included.  With wide_trace calls in between (they share nothing with the scratch): the same, and their distances too."""
    sc = inward_box()
    dev = sc._dev()
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    l7 = L7[:1]
    calls, probes = [], []
    for i in range(EC.SLOT_CALLS):
        o, d, _ = slot_rays(i)
        calls.append((torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)) + buffers(dev, len(o), preset=(i, 2 * i)))
        if interleave:
            po, pd, pdist = probe_rays(i)
            probes.append(tuple(torch.from_numpy(a).to(dev) for a in (po, pd, pdist)))
    torch.cuda.synchronize()           # the inputs are there; from here on nothing waits for the device until all 20 are enqueued
    for i, (do, dd, out, npho, stats) in enumerate(calls):
        s = streams[EC.slot_plan(i)[1]]
        sc.trace_photons(do, dd, l7, len(do), out=out, n_photons=npho, stats=stats, stream=s)
        if interleave:
            po, pd, pdist = probes[i]
            sc.wide_trace(po, pd, pdist, stream=streams[1 - EC.slot_plan(i)[1]] if i % 3 else s)
    torch.cuda.synchronize()
    got = [(out.cpu().numpy(), int(npho.cpu()[0]), stats.cpu().tolist()) for (_, _, out, npho, stats) in calls]
    got_probes = [p[2].cpu().numpy() for p in probes]
    sc.close()
    for i, (do, dd, _, _, _) in enumerate(calls):
        fresh = inward_box()
        out, npho, stats = buffers(dev, len(do), preset=(i, 2 * i))
        fresh.trace_photons(do, dd, l7, len(do), out=out, n_photons=npho, stats=stats)
        if interleave:
            po, pd, _ = probes[i]
            pdist = torch.from_numpy(probe_rays(i)[2]).to(dev)
            fresh.wide_trace(po, pd, pdist)
        torch.cuda.synchronize()
        k = int(npho.cpu()[0])
        assert got[i][1] == k and got[i][2] == stats.cpu().tolist(), (i, got[i][1], k)
        assert got[i][0].tobytes() == out.cpu().numpy().tobytes(), i
        assert k == slot_rays(i)[2] and stats.cpu().tolist()[1] > 2 * i          # the "hit" rays, and only they, leave a record
        if interleave:
            assert got_probes[i].tobytes() == pdist.cpu().numpy().tobytes(), i
        fresh.close()
