"""The pool of intermediates and the frame-list cache of the two material handles on the MI355X (snail_amd/csrc/shading_sets_host.inc): ONE set
of a plain MaterialSet and of an InstancedMaterialSet is walked through its eight-slot rotation three laps and one call long, alternating over
two streams, so that consecutive uses of a slot take every growth path -- more packets, more lights, the bounce's part, the tile renderer's,
the levels', the per-packet counters' on a slot that has none yet, the same part grown, and a slot larger than its call.  Every call's bytes
(and its truncated count) equal, ==, those of the same call on a freshly created set: what a fresh set gives is tied to the oracle and the
restatements by the tests of each entry point.  The frame-list cache is taken past its cap of 16 packet-grid sizes and back to the first.
The tile renderer's part is reached by two routes: `frame_packets` with a tint books it together with the set (the plain opaque set alone has
that entry point: an instanced set has none, and it refuses a set that can select a transparent lane), `tree_frame_packets` with a tint grows it
beside the levels (every set).
Nothing here depends on how the pool is written: the file passes against any library whose sets behave as include/snail_materials*.h say."""
import numpy as np
import pytest

from snail_amd import instances_materials as IP
from snail_amd import materials as P
from snail_amd.instances import InstancedScene
from tests import instances_materials_cases as IK
from tests import instances_materials_transparency_cases as IC
from tests import materials_cases as K
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu
ARITH = [("ieee", O.MODE_IEEE), ("host_sse", O.MODE_SSE)]
REFL, AA = P.RENDER_REFLECTIONS, P.RENDER_AA4
TINT = (0.9, 0.55, 1.2)
SLOTS = 8
# one lap of the eight slots each: (resx, resy, lights, max_depth, shift of the call kinds against the slots).  Lap 2 grows what lap 1 allocated, in
# packets (2 x 2 -> 3 x 2), lights (0 -> 2) and depth (1 -> 4); lap 3 (5 x 3 packets) gives every slot the NEXT kind's parts beside its own.
LAPS = [(32, 32, 0, 1, 0), (48, 32, 2, 4, 0), (80, 48, 2, 4, 1)]
LAST = (32, 32, 0, 1)      # after the largest shape the smallest again: a slot larger than its call


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


# ---- the sets: (handle whose arithmetic is set, camera, lights, a function that creates a NEW set) ----
def plain(capable):
    """the smallest plain cases: materials_cases.small_scene with the materials of `quirk`, or `panes` with its transparent materials"""
    from tests.test_gpu_materials import device_set
    from tests.test_gpu_materials_transparency import panes_set, product_materials
    if capable:
        c, sc, _ = panes_set()
        cam = c["cam"]
    else:
        c, (sc, _) = K.case("quirk"), device_set("quirk")
        cam = K.case("degenerate_small")["cam"]      # (the same scene seen whole)
    tex = [P.Texture(t) for t in c["textures"]]
    new = lambda: P.MaterialSet(sc, c["uv"], c["nrm"], c["mat_index"], c["flat"], c["material_map"], product_materials(c["descs"]), tex, transparent=capable)      # noqa: E731
    return sc.set_arith, cam, c["lights"], new


def instanced(capable):
    """the smallest instanced cases: `main` of instances_materials_cases, or `glasshouse` with its panes"""
    from tests import test_gpu_instances_materials as TI
    from tests import test_gpu_instances_materials_transparency as TT
    if capable:
        c = IC.case("glasshouse")
        isc, _ = TT.device_set("glasshouse")
        mats, tex = TT.product_materials(c["descs"], IC.textures())
    else:
        c = IK.case("main")
        isc, _ = TI.device_set("main")
        mats, tex = TI.product_materials()
    new = lambda: IP.InstancedMaterialSet(isc, c["per_blas"], mats, tex, transparent=capable)      # noqa: E731
    return (lambda a: TI.set_arith(isc, a)), c["cams"][96], c["lights"], new


SETS = {"plain": plain, "instanced": instanced}


# ---- the calls: eight kinds per set, each a function of (set, camera, resx, resy, packet list, lights, depth) -> device tensors ----
def kinds(is_plain, capable):
    def tinted(ms, cam, rx, ry, xy, L, d):
        if is_plain and not capable:
            return (ms.frame_packets(cam, rx, ry, xy, L, tint=TINT),)      # (matShadeStore: the tile renderer's part beside the opaque stages)
        return ms.tree_frame_packets(cam, rx, ry, xy, L, tint=TINT, max_depth=d)
    levels = [
        ("transparent_packets", lambda ms, cam, rx, ry, xy, L, d: ms.render_transparent_packets(cam, rx, ry, xy, L, max_depth=d)),
        ("heat without a caller's array", lambda ms, cam, rx, ry, xy, L, d: ms.render_heat_packets(cam, rx, ry, xy, L, flags=REFL, max_depth=d)),
        ("packet_stats", lambda ms, cam, rx, ry, xy, L, d: ms.packet_stats(cam, rx, ry, None, L, reflections=True, max_depth=d)),
        ("tree bounce 4x", lambda ms, cam, rx, ry, xy, L, d: ms.tree_frame_packets(cam, rx, ry, xy, L, flags=REFL | AA, max_depth=d)),
        ("tinted", tinted),
    ]
    if capable:      # the entry points that take ANY set
        return levels + [
            ("transparent", lambda ms, cam, rx, ry, xy, L, d: ms.render_transparent(cam, rx, ry, L, max_depth=d)),
            ("tree bounce", lambda ms, cam, rx, ry, xy, L, d: ms.tree_frame_packets(cam, rx, ry, xy, L, flags=REFL, max_depth=d)),
            ("transparent_packets cut at 2", lambda ms, cam, rx, ry, xy, L, d: ms.render_transparent_packets(cam, rx, ry, xy, L, max_depth=min(d, 2))),
        ]
    return [
        ("frame", lambda ms, cam, rx, ry, xy, L, d: (ms.render(cam, rx, ry, L),)),
        ("frame with the bounce", lambda ms, cam, rx, ry, xy, L, d: (ms.render(cam, rx, ry, L, reflections=True),)),
        ("packets", lambda ms, cam, rx, ry, xy, L, d: (ms.render_packets(cam, rx, ry, xy, L),)),
    ] + levels[:1] + [
        ("packets with the bounce", lambda ms, cam, rx, ry, xy, L, d: (ms.render_packets(cam, rx, ry, xy, L, reflections=True),)),
    ] + levels[1:2] + levels[3:]


def shuffled_grid(resx, resy):
    pw, ph = (resx + 15) // 16, (resy + 15) // 16
    xy = np.array([(x * 16, y * 16) for y in range(ph) for x in range(pw)], dtype=np.int32)
    return xy[np.random.RandomState(7 + pw).permutation(len(xy))]


def host(outs):
    return [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("capable", [False, True], ids=["opaque", "transparent"])
@pytest.mark.parametrize("which", sorted(SETS))
def test_one_set_through_its_rotation_and_growth(torch_mod, which, capable, arith, mode):
    torch = torch_mod
    set_arith, cam, lights, new_set = SETS[which](capable)
    ks = kinds(which == "plain", capable)
    assert len(ks) == SLOTS
    steps = [(ks[(slot + shift) % SLOTS],) + (rx, ry, nl, d) for rx, ry, nl, d, shift in LAPS for slot in range(SLOTS)] + [(ks[0],) + LAST]
    assert len(steps) >= 2 * SLOTS + 1
    lists = {(rx, ry): torch.from_numpy(shuffled_grid(rx, ry)).to("cuda:0") for _, rx, ry, _, _ in steps}
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()

    def run(ms, step):
        (_, call), rx, ry, nl, d = step
        return call(ms, cam, rx, ry, lists[(rx, ry)], lights[:nl] if nl else None, d)

    set_arith(arith)
    try:
        ms = new_set()
        got = []
        for i, step in enumerate(steps):      # all enqueued before anything is waited for: a slot's next user meets its previous one's event
            with torch.cuda.stream(streams[i % 2]):
                got.append(run(ms, step))
        torch.cuda.synchronize()
        got = [host(g) for g in got]
        ms.close()
        distinct = 0
        for i, (step, g) in enumerate(zip(steps, got)):
            fresh = new_set()
            want = host(run(fresh, step))
            fresh.close()
            what = "%s %s %s call %d (slot %d) %s %dx%d lights %d depth %d" % ((which, "transparent" if capable else "opaque", arith, i, i % SLOTS, step[0][0]) + step[1:])
            bad = [int((a != b).sum()) for a, b in zip(g, want)]
            print("%s: differing %s of %s; distinct values %d%s" % (what, bad, [a.size for a in want], len(np.unique(want[0])),
                                                                    "; truncated %d" % int(want[1][0]) if len(want) > 1 else ""))
            assert len(g) == len(want) and all(a.shape == b.shape and a.dtype == b.dtype for a, b in zip(g, want)), what
            assert not any(bad), (what, bad)
            distinct += len(np.unique(want[0])) > 2
        assert distinct >= len(steps) - 2, distinct      # (no comparison of blank frames: at most the two smallest may show one surface alone)
    finally:
        set_arith("ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
@pytest.mark.parametrize("which", sorted(SETS))
def test_the_frame_list_cache_past_its_cap(torch_mod, which, arith, mode):
    """17 whole frames at 17 packet-grid sizes (k x 1 packets, k = 1..17) on one set, then the first size again: the 17th drops the 16 cached lists"""
    set_arith, cam, lights, new_set = SETS[which](False)
    sizes = [(16 * k, 16) for k in range(1, 18)] + [(16, 16)]
    set_arith(arith)
    try:
        ms = new_set()
        got = [ms.render(cam, rx, ry, lights) for rx, ry in sizes]
        got = host(got)
        ms.close()
        for (rx, ry), g in zip(sizes, got):
            fresh = new_set()
            want = fresh.render(cam, rx, ry, lights).cpu().numpy()
            fresh.close()
            print("%s %s frame list %dx%d: %d differing bytes of %d" % (which, arith, rx, ry, int((g != want).sum()), want.size))
            assert g.shape == want.shape == (ry, rx, 3) and np.array_equal(g, want), (which, arith, rx, ry)
        assert np.array_equal(got[0], got[-1]) and sum(len(np.unique(g)) > 2 for g in got) >= len(got) // 2
    finally:
        set_arith("ieee")


@pytest.mark.parametrize("arith,mode", ARITH)
def test_the_instances_handle_frame_list_cache_past_its_cap(torch_mod, arith, mode):
    """the same cache in the instances handle (render_whitted), against a handle created for each frame"""
    from tests import test_gpu_instances_materials as TI
    c = IK.case("main")
    isc, _ = TI.device_set("main")
    cam, lights = c["cams"][96], c["lights"]
    sizes = [(16 * k, 16) for k in range(1, 18)] + [(16, 16)]
    TI.set_arith(isc, arith)
    try:
        walked = InstancedScene(isc.blas, c["rot"], c["tr"], c["bi"])
        got = host([walked.render_whitted(cam, rx, ry, lights) for rx, ry in sizes])
        walked.close()
        for (rx, ry), g in zip(sizes, got):
            fresh = InstancedScene(isc.blas, c["rot"], c["tr"], c["bi"])
            want = fresh.render_whitted(cam, rx, ry, lights).cpu().numpy()
            fresh.close()
            assert g.shape == want.shape == (ry, rx, 3) and np.array_equal(g, want), (arith, rx, ry, int((g != want).sum()))
        assert np.array_equal(got[0], got[-1]) and sum(len(np.unique(g)) > 2 for g in got) >= len(got) // 2
    finally:
        TI.set_arith(isc, "ieee")
