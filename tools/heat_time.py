"""What a heat-map frame (gVals[5]: include/snail_heatmap.h) costs beside the lit frame of the same configuration on the same build: the atrium at
1920x1080 with the one point light of bench.py's config 3, bounce off and on, in the scene's default arithmetic (host_sse where available) --
device ms per frame between two events, medians of alternating runs:
  lit    Scene.render_whitted (snail_render_whitted_dev): the interleaved frame;
  heat   Scene.render_heat_packets (snail_render_heat_packets_dev) over the frame's grid + Scene.packets_bgr_to_frame: the same walks with the
         per-packet booking, no colour stage, the counters' colours and the scatter into the frame;
  stats  Scene.packet_stats (snail_packet_stats_dev): the counters alone.
Writes the table to profiles/heatmap.txt (or --out) and prints one JSON object.  No target: a measurement.

    python tools/heat_time.py [--res 1920x1080] [--reps 9] [--out profiles/heatmap.txt]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from snail_amd import FPSCamera, HostBVH, scenes  # noqa: E402
from snail_amd._lib import SnailError  # noqa: E402
from snail_amd.scene import Scene  # noqa: E402


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", default="1920x1080")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heatmap.txt"))
    a = ap.parse_args()
    resx, resy = (int(x) for x in a.res.split("x"))
    tv = scenes.scene_by_name("atrium")
    hb = HostBVH.build(tv)
    sc = Scene(hb, 0)
    try:
        sc.set_arith("host_sse")
    except SnailError:
        sc.set_arith("ieee")
    pos, ang, pitch = scenes.atrium_camera()
    cam = FPSCamera(pos, ang, pitch).camera()
    bmin, bmax = hb.bbox()
    c, e = (bmin + bmax) * 0.5, (bmax - bmin)
    lights = np.array([[c[0], c[1] + 0.35 * e[1], c[2], 1.0, 0.9, 0.8, 2.0 * float(e.max())]], dtype=np.float32)   # bench.py's config 3
    n = ((resx + 15) // 16) * ((resy + 15) // 16)
    frame = torch.zeros((resy, resx, 3), dtype=torch.uint8, device="cuda")
    bgr = torch.zeros((n, 256, 3), dtype=torch.uint8, device="cuda")
    pst = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    xy = torch.tensor([(x, y) for y in range(0, resy, 16) for x in range(0, resx, 16)], dtype=torch.int32, device="cuda")

    def heat(refl):
        sc.render_heat_packets(cam, resx, resy, None, lights, reflections=refl, out=bgr)
        Scene.packets_bgr_to_frame(xy, bgr, frame)

    runs = {
        "lit": lambda refl: sc.render_whitted(cam, resx, resy, lights, out=frame, reflections=refl),
        "heat": heat,
        "stats": lambda refl: sc.packet_stats(cam, resx, resy, None, lights, reflections=refl, out=pst),
    }
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    res = {"scene": "atrium", "res": [resx, resy], "arith": sc.arith(), "reps": a.reps}
    lines = ["heat-map frame against the lit frame: atrium %dx%d, one light (config 3), arithmetic %s; device ms per frame, median of %d alternating runs"
             % (resx, resy, sc.arith(), a.reps), ""]
    for refl in (False, True):
        ms = {k: [] for k in runs}
        for k in runs:          # warm-up: scratch growth, origin-relative node records
            runs[k](refl)
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for k, fn in runs.items():
                e0.record()
                fn(refl)
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        med = {k: statistics.median(v) for k, v in ms.items()}
        key = "bounce" if refl else "no_bounce"
        res[key] = {"ms": med, "heat_over_lit": med["heat"] / med["lit"], "stats_over_lit": med["stats"] / med["lit"],
                    "spread_ms": {k: [min(v), max(v)] for k, v in ms.items()}}
        lines.append("%-10s lit %.3f ms   heat %.3f ms (x %.3f)   stats only %.3f ms (x %.3f)"
                     % (key, med["lit"], med["heat"], med["heat"] / med["lit"], med["stats"], med["stats"] / med["lit"]))
        lines.append("           min..max: " + "   ".join("%s %.3f..%.3f" % (k, min(v), max(v)) for k, v in ms.items()))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), file=sys.stderr)
    print(json.dumps(res))
    sc.close()


if __name__ == "__main__":
    main()
