"""Multi-frame primary launches against single-frame launches (run with -m gpu on an MI355X).

A launch of F frames maps its F x nSlots workgroups onto (frame, dispatch rank) pairs so that the F copies of a rank run on one XCD
(k_primary's XCD-major block -> (frame, rank) map).  Whatever the map, every frame must come out bit for bit as its own one-frame launch, the TreeStats
as their sum and d_slot_cost as the first frame's.  F = 3, 5 catch a non-power-of-two slip in the map; the rect's packet grid (21 x 13)
is not a multiple of the 4 x 4 regions, and the packet list (300 packets) is not a multiple of 128."""
from __future__ import annotations

import numpy as np
import pytest

from snail_amd import FPSCamera
from tests import util

pytestmark = pytest.mark.gpu

FRAMES = [2, 3, 4, 5, 8]
RES = (328, 200)        # 21 x 13 packets
LIST_RES = (640, 368)   # 40 x 23 packets, 300 of them in the list
N_LIST = 300


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module", params=["ieee", "host_sse"])
def scene(request):
    from snail_amd.scene import Scene
    tv, hbvh, osc = util.scene_pair("atrium:0.05")
    sc = Scene(hbvh, 0)
    sc.set_arith(request.param)
    assert sc.arith() == request.param
    yield tv, sc, osc
    sc.close()


def cameras(tv, osc, n, seed):
    base = util.camera_for("atrium:0.05", tv)
    rng = np.random.RandomState(seed)
    ext = osc.nodes[0]["bmax"] - osc.nodes[0]["bmin"]
    return [base] + [FPSCamera((base.pos + (rng.rand(3) - 0.5) * 0.05 * ext).astype(np.float32), float(rng.rand() * 6.28),
                               float(rng.rand() - 0.5) * 0.4).camera() for _ in range(n - 1)]


def same_frame(a, b, what):
    for name in ("t", "u", "v", "tri_id"):
        util.assert_bit_equal(getattr(a, name).cpu().numpy(), getattr(b, name).cpu().numpy(), "%s %s" % (what, name))


def singles(torch_mod, sc, cams, order):
    """Each camera in a one-frame launch: frames, summed TreeStats, the first frame's slot costs."""
    n = sc.primary_slots(*RES)
    frames, total, cost0 = [], np.zeros(4, dtype=np.int64), None
    for k, c in enumerate(cams):
        st = sc.new_stats()
        cost = torch_mod.zeros(n, dtype=torch_mod.int32, device="cuda")
        frames.append(sc.trace_primary(c, RES[0], RES[1], stats=st, order=order, slot_cost=cost))
        total += st.cpu().numpy()
        if k == 0:
            cost0 = cost.cpu().numpy()
    torch_mod.cuda.synchronize()
    return frames, total, cost0


@pytest.mark.parametrize("nf", FRAMES)
def test_rect_batch_equals_single_frames(torch_mod, scene, nf):
    """snail_trace_primary_batch_dev with the built-in order and with a fed-back (sorted: scattered ranks) order."""
    tv, sc, osc = scene
    cams = cameras(tv, osc, nf, 100 + nf)
    n = sc.primary_slots(*RES)
    ref, ref_stats, ref_cost = singles(torch_mod, sc, cams, None)
    sorted_order = sc.order_from_cost(torch_mod.from_numpy(ref_cost).cuda(), exact=True)
    assert sorted(sorted_order.cpu().numpy().tolist()) == list(range(n))
    for label, order in (("built-in order", None), ("fed-back order", sorted_order)):
        outs = [sc.alloc_frame(*RES) for _ in range(nf)]
        stats = sc.new_stats()
        cost = torch_mod.full((n,), -7, dtype=torch_mod.int32, device="cuda")
        sc.trace_primary_batch(cams, RES[0], RES[1], outs, stats=stats, order=order, slot_cost=cost)
        torch_mod.cuda.synchronize()
        for k in range(nf):
            same_frame(outs[k], ref[k], "%s, %d frames: frame %d" % (label, nf, k))
        assert np.array_equal(stats.cpu().numpy(), ref_stats), label
        assert np.array_equal(cost.cpu().numpy(), ref_cost), label


@pytest.mark.parametrize("nf", FRAMES)
def test_rect_batch_reorder_equals_single_frames(torch_mod, scene, nf):
    """snail_trace_primary_batch_reorder_dev: the frames of a launch that also derives the next order, fed that order again."""
    tv, sc, osc = scene
    cams = cameras(tv, osc, nf, 200 + nf)
    n = sc.primary_slots(*RES)
    ref, ref_stats, ref_cost = singles(torch_mod, sc, cams, None)
    order = torch_mod.arange(n, dtype=torch_mod.int32, device="cuda").flip(0).contiguous()   # a permutation that is not the built-in one
    for launch in range(2):
        outs = [sc.alloc_frame(*RES) for _ in range(nf)]
        stats = sc.new_stats()
        cost = torch_mod.zeros(n, dtype=torch_mod.int32, device="cuda")
        sc.trace_primary_batch(cams, RES[0], RES[1], outs, stats=stats, order=order, slot_cost=cost, next_order=order, order_exact=True)
        torch_mod.cuda.synchronize()
        for k in range(nf):
            same_frame(outs[k], ref[k], "reorder launch %d, %d frames: frame %d" % (launch, nf, k))
        assert np.array_equal(stats.cpu().numpy(), ref_stats)
        assert np.array_equal(cost.cpu().numpy(), ref_cost)
        assert sorted(order.cpu().numpy().tolist()) == list(range(n))


@pytest.mark.parametrize("nf", FRAMES)
def test_packet_list_batch_equals_single_frames(torch_mod, scene, nf):
    """snail_trace_packets_shaded_batch_dev over a shuffled list of 300 packets: shaded bytes and TreeStats."""
    tv, sc, osc = scene
    cams = cameras(tv, osc, nf, 300 + nf)
    pw, ph = (LIST_RES[0] + 15) // 16, (LIST_RES[1] + 15) // 16
    rng = np.random.RandomState(nf)
    pick = rng.permutation(pw * ph)[:N_LIST]
    xy = torch_mod.from_numpy(np.stack([pick % pw * 16, pick // pw * 16], axis=1).astype(np.int32)).cuda()
    ref, ref_stats = [], np.zeros(4, dtype=np.int64)
    for c in cams:
        st = sc.new_stats()
        ref.append(sc.trace_packets_shaded(c, LIST_RES[0], LIST_RES[1], xy, stats=st))
        ref_stats += st.cpu().numpy()
    bg = [torch_mod.zeros((N_LIST, 256, 3), dtype=torch_mod.uint8, device="cuda") for _ in range(nf)]
    stats = sc.new_stats()
    sc.trace_packets_shaded_batch(cams, LIST_RES[0], LIST_RES[1], xy, bg, stats=stats)
    torch_mod.cuda.synchronize()
    for k in range(nf):
        assert torch_mod.equal(bg[k], ref[k]), "%d frames: frame %d" % (nf, k)
    assert np.array_equal(stats.cpu().numpy(), ref_stats)
