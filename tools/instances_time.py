"""What an instanced primary frame costs: Mrays/s of a 1920x1080 frame of snail_instances_trace_primary_dev for N = 1 (the identity
instance alone), 64 and 1024 instances (scenes.instance_field) of the atrium stand-in and of the lancia fixture, in both arithmetics,
beside the plain Scene.trace_primary rate of the same BLAS; and what a per-frame rebuild costs (the reference's -instances mode rebuilds the
top-level tree every frame): the host build (snail_instances_build) and a whole InstancedScene.update() -- build + upload, host wall time --
for --rebuild-counts instances (default 10 000).  Prints one JSON object.  No target: a measurement.

    python tools/instances_time.py [--res 1920x1080] [--reps 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from snail_amd import HostBVH, scenes, survey_camera  # noqa: E402
from snail_amd.instances import InstancedScene  # noqa: E402
from snail_amd.scene import Scene  # noqa: E402


def timed(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = None
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    return best


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", default="1920x1080")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--counts", default="1,64,1024")
    ap.add_argument("--rebuild-counts", default="10000")
    a = ap.parse_args()
    resx, resy = (int(x) for x in a.res.split("x"))
    rays = resx * resy
    out = {"res": a.res, "unit": "Mrays/s (best of %d launches)" % a.reps, "rows": []}
    meshes = {"atrium": lambda: scenes.atrium(),
              "lancia": lambda: np.load(os.path.join(ROOT, "tests", "golden", "lancia_tris.npz"))["tris"].reshape(-1, 9).astype(np.float32)}
    for name, load in meshes.items():
        tv = load()
        sc = Scene(HostBVH.build(tv), 0)
        lo, hi = sc.get_bbox()
        for arith in ("ieee", "host_sse"):
            sc.set_arith(arith)
            cam = survey_camera(tv)
            plain = timed(torch, lambda: sc.trace_primary(cam, resx, resy), a.reps)
            for n in (int(c) for c in a.counts.split(",")):
                rot, tr, bi = scenes.instance_field(lo, hi, n, seed=1)
                isc = InstancedScene([sc], rot, tr, bi)
                nd = isc.nodes()[0]
                fcam = cam if n == 1 else survey_camera(np.concatenate([nd["bmin"], nd["bmax"], nd["bmin"]]).reshape(1, 9))
                ms = timed(torch, lambda: isc.trace_primary(fcam, resx, resy), a.reps)
                plain_f = plain if n == 1 else timed(torch, lambda: sc.trace_primary(fcam, resx, resy), a.reps)
                out["rows"].append({"blas": name, "arith": arith, "instances": n, "instanced_mrays": round(rays / ms / 1e3, 1),
                                    "plain_mrays_same_camera": round(rays / plain_f / 1e3, 1), "instanced_ms": round(ms, 3)})
                isc.close()
        if name == "atrium":
            out["rebuild"] = rebuild(torch, sc, [int(c) for c in a.rebuild_counts.split(",")], a.reps)
        sc.close()
    print(json.dumps(out))


def rebuild(torch, sc, counts, reps):
    """best-of-`reps` host wall time of snail_instances_build and of InstancedScene.update (build + ordered upload, synchronised)"""
    import time
    from snail_amd.instances import build_instances, _xf12
    lo, hi = sc.get_bbox()
    bb = np.concatenate([lo, hi]).astype(np.float32).reshape(1, 6)
    rows = []
    for n in counts:
        rot, tr, bi = scenes.instance_field(lo, hi, n, seed=2)
        xf = _xf12(rot, tr)
        best_b = best_u = None
        isc = InstancedScene([sc], rot, tr, bi)
        for k in range(reps):
            t0 = time.perf_counter(); build_instances(xf, bi, bb); t1 = time.perf_counter()
            best_b = t1 - t0 if best_b is None else min(best_b, t1 - t0)
            rot2, tr2, _ = scenes.instance_field(lo, hi, n, seed=3 + k)
            torch.cuda.synchronize()
            t0 = time.perf_counter(); isc.update(rot2, tr2, bi); torch.cuda.synchronize(); t1 = time.perf_counter()
            best_u = t1 - t0 if best_u is None else min(best_u, t1 - t0)
        isc.close()
        rows.append({"instances": n, "build_ms": round(best_b * 1e3, 3), "update_ms": round(best_u * 1e3, 3)})
    return rows


if __name__ == "__main__":
    main()
