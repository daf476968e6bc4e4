"""Host-only checks (no GPU) of the cases of tests/instances_materials_tree_cases.py against the conditions the GPU tests
(tests/test_gpu_instances_materials_tree.py) rest on, asserted on the restatement (tests/instances_materials_tree_ref.py) alone.  The counts
are lower bounds on coverage, not measurements: if a case misses one, the case changes, not the bound.

Truncated-lane counters of the unmutated restatement with reflections (96x64, whatever the lights):
  glasshouse   maxDepth 2: 842   3: 187   4: 3   5: 1   6: 0        (without the bounce at maxDepth 2: 286, the figure of
  moved        maxDepth 2: 321   3: 12    4: 0                        tests/instances_materials_transparency_cases.py's own reference)
  deep         maxDepth 1: 138   2: 0
So the frames of `glasshouse` and `moved` that the GPU test takes at maxDepth 2 are cut frames -- rays cross three panes and pane2 -- and
`deep`, ONE pane before the chain BLAS, is cut at maxDepth 1, not at 2: through the bounce its B chains reach level 2 and select nothing there.
The GPU test therefore compares `glasshouse` and `moved` at maxDepth 2 (counter equal to the restatement's, non-zero) AND at FULL_DEPTH, where the
counter is 0 and the frame is the reference's; and `deep` at maxDepth 2 and 8 (counter 0) AND at maxDepth 1 (non-zero, equal)."""
import numpy as np
import pytest

from tests import instances_materials_transparency_cases as C
from tests import instances_materials_tree_cases as K
from tests import instances_materials_tree_ref as R
from tests import oracle_lib as O


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutation_changes_bytes_or_treestats_of_a_case(mutation):
    changed = []
    for name in reversed(K.NAMES):       # (the quickest case first; one case that shows the rule is enough)
        base, mut = K.reference(name), K.reference(name, mutation=mutation)
        nb = int((base[0] != mut[0]).sum())
        print("%s / %s: %d differing bytes, stats %s / %s, truncated %d / %d" % (mutation, name, nb, base[1].tolist(), mut[1].tolist(), base[2], mut[2]))
        if nb or not np.array_equal(base[1], mut[1]):
            changed.append(name)
            break
    assert changed, mutation


def test_without_the_bounce_the_restatement_is_the_transparency_restatement():
    for name in ("glasshouse", "deep"):
        bgr, st, trunc, _, xy, _ = K.reference(name, bounce=False)
        resx, resy = K.FRAME
        fr, wst, wtrunc, _, wxy = C.IT.InstTranspFrames(K.transp_ref(name)).render(K.camera(name).as_array13(), resx, resy, K.lights_of(name, 2), mode=O.MODE_IEEE,
                                                                                     max_depth=K.GPU_DEPTH)
        assert np.array_equal(xy, wxy) and np.array_equal(C.IT.S.packets_to_frame(xy, bgr, resx, resy), fr) and np.array_equal(st, wst) and trunc == wtrunc


def test_truncated_lane_counters_of_the_cases():
    for name in ("glasshouse", "moved"):
        assert K.reference(name, max_depth=K.FULL_DEPTH)[2] == 0, name           # the frames compared at FULL_DEPTH are the reference's
        assert K.reference(name, max_depth=K.GPU_DEPTH)[2] > 0, name             # ... those at maxDepth 2 are cut, by the restatement's own count
    assert K.reference("deep", n_lights=1, max_depth=K.CUT_DEPTH)[2] > 0         # its purpose: a counter that moves
    assert K.reference("deep", n_lights=1, max_depth=K.GPU_DEPTH)[2] == 0
    assert K.reference("deep", n_lights=1, max_depth=8)[2] == 0


def test_all_miss_packets_of_a_nested_level_are_mirrored_and_b_lanes_continue():
    seen_miss = seen_cont = seen_trunc_b = 0
    for name in K.NAMES:
        d = K.reference(name)[3]
        seen_miss += sum(v for k, v in d.mirrored_all_miss.items() if k >= 1)
        seen_cont += sum(d.b_selected.values())
        seen_trunc_b += d.truncated_b
        print(name, "A calls", d.a_calls, "B calls", d.b_calls, "all-miss mirrored", d.mirrored_all_miss, "B lanes continued", d.b_selected, "truncated A / B", d.truncated_a, d.truncated_b)
        for k, n in d.a_calls.items():       # every call of chain A starts ONE mirrored call, hit or not
            assert d.b_calls.get((k, k), 0) == n
    assert seen_miss >= 1 and seen_cont >= 1 and seen_trunc_b >= 1
    d = K.reference("deep")[3]
    assert sum(v for k, v in d.mirrored_all_miss.items() if k >= 1) >= 1 and d.b_calls.get((1, 2), 0) >= 1


def test_slicing_the_packet_list_changes_nothing():
    name = "moved"
    bgr, st, trunc, _, xy, _ = K.reference(name)
    parts = [K.reference(name, xy=tuple(map(tuple, xy[a:b].tolist()))) for a, b in ((0, 7), (7, 8), (8, len(xy)))]
    assert np.array_equal(np.concatenate([p[0] for p in parts]), bgr)
    assert np.array_equal(sum(p[1] for p in parts), st) and sum(p[2] for p in parts) == trunc


def test_aa_tint_and_tiles_go_through_the_tile_restatement():
    tr = K.tiles_ref("moved")
    resx, resy = K.AA_FRAME
    cam = K.camera("moved").as_array13()
    xy = C.IT.S.frame_packets(resx, resy)
    plain, st0 = tr.packets(cam, resx, resy, xy, K.lights_of("moved", 2), R.REFLECTIONS | R.AA4)
    t0 = tr.truncated
    tinted, st1 = tr.packets(cam, resx, resy, xy, K.lights_of("moved", 2), R.REFLECTIONS | R.AA4, tint=K.TINT)
    assert np.array_equal(st0, st1) and tr.truncated == t0 and (plain != tinted).any()
    # four trees per output packet: the double-resolution frame's packets, each with its own counters
    sub = np.array([(2 * x + ox, 2 * y + oy) for x, y in xy.tolist() for ox, oy in ((0, 0), (16, 0), (0, 16), (16, 16))], dtype=np.int32)
    fr = R.InstTreeFrames(K.transp_ref("moved"))
    _, wst, wtrunc, _ = fr.render_packets(cam, resx * 2, resy * 2, sub, K.lights_of("moved", 2), max_depth=K.GPU_DEPTH)
    assert np.array_equal(st0, wst) and t0 == wtrunc
    # depth shading: no level runs, the counter does not move
    _, _ = tr.packets(cam, resx, resy, xy, None, R.DEPTH | R.REFLECTIONS)
    assert tr.truncated == 0
