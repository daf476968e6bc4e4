"""Timing of BVH::WideTrace with one ray per lane (snail_wide_trace_dev) against the only way the packet walks can trace the same rays:
snail_trace_rays_dev with 64-quad groups of consecutive rays, per-ray origins (sharedOrigin = 0), no mask, on the same handle in the same
process.  (Its hit rule differs -- it culls t <= 0 and reports the triangle --, so only times are compared.)

Rays: 2^20 photons of snail_amd.photons.emit at the atrium camera position in the atrium scene, (a) in emission order -- consecutive
stratified photons form a thin fan -- and (b) under a seeded permutation, where a 256-ray group holds unrelated rays.
Per figure: 3 warm-up launches, 20 timed launches between HIP events (the distances are reset outside the events), the median; every
figure is taken 5 times and the spread of the 5 medians is reported.
Usage: python tools/wide_time.py [--rays N] [--scene NAME] [--out FILE]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from snail_amd import HostBVH, photons, scenes
from snail_amd.scene import Context, Scene

ap = argparse.ArgumentParser()
ap.add_argument("--rays", type=int, default=1 << 20)
ap.add_argument("--scene", default="atrium")
ap.add_argument("--out", default=None)
args = ap.parse_args()

WARM, TIMED, REPEATS = 3, 20, 5
n = (args.rays // 256) * 256
tv = scenes.scene_by_name(args.scene)
sc = Scene(HostBVH.build(tv), 0)
pos = scenes.stress_camera()[0] if args.scene.startswith("stress") else scenes.atrium_camera()[0]
origin, dirs = photons.emit(pos, n, seed=1)
perm = np.random.RandomState(2).permutation(n)
dev = sc._dev()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def median_ms(launch, reset):
    ms = []
    for k in range(WARM + TIMED):
        reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        if k >= WARM:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def figure(launch, reset):
    meds = [median_ms(launch, reset) for _ in range(REPEATS)]
    return float(np.median(meds)), max(meds) - min(meds)


def quads(a):   # [n, 3] -> Vec3q[]: per quad {x[4], y[4], z[4]}
    return np.ascontiguousarray(a.reshape(-1, 4, 3).transpose(0, 2, 1)).reshape(-1, 12)


say("%s: %d triangles, depth %d; %d rays from photons.emit at %s" % (args.scene, len(tv), sc.depth, n, np.asarray(pos).tolist()))
results = {}
for label, o, d in (("(a) emission order", origin, dirs), ("(b) seeded permutation", origin[perm], dirs[perm])):
    with np.errstate(all="ignore"):
        inv = (np.float32(1.0) / d).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    do, dd, di = t(o), t(d), t(inv)
    dist = torch.empty(n, dtype=torch.float32, device=dev)
    stats = torch.zeros(2, dtype=torch.int64, device=dev)
    sc.wide_trace(do, dd, dist.fill_(float("inf")), idir=di, stats=stats)
    torch.cuda.synchronize()
    hits = int(torch.isfinite(dist).sum().item())
    box_tests, tri_tests = stats.cpu().tolist()
    wide = figure(lambda: sc.wide_trace(do, dd, dist, idir=di), lambda: dist.fill_(float("inf")))
    ctx = Context(t(quads(o)), t(quads(d)), t(quads(inv)), torch.empty((n // 4, 4), dtype=torch.float32, device=dev),
                  torch.empty((n // 4, 4), dtype=torch.int32, device=dev), None, size=64, shared_origin=False)

    def reset_ctx():
        ctx.distance.fill_(float("inf"))
        ctx.object.fill_(0)
    packet = figure(lambda: sc.traverse_primary(ctx), reset_ctx)
    results[label[:3]] = (wide, packet)
    say("%s: %d rays hit; %.1f box tests and %.1f triangle tests per ray" % (label, hits, box_tests / n, tri_tests / n))
    say("    wide walk, one ray per lane : median %8.3f ms  spread %.3f ms  %8.1f Mrays/s" % (wide[0], wide[1], n / wide[0] / 1e3))
    say("    256-ray packets (comparator): median %8.3f ms  spread %.3f ms  %8.1f Mrays/s" % (packet[0], packet[1], n / packet[0] / 1e3))
(wide, packet) = results["(b)"]
margin = packet[0] - wide[0]
ok = margin > wide[1] + packet[1]
say("requirement on (b): the wide walk is faster than the comparator by more than the measured spread: %.3f ms against %.3f ms -> %s"
    % (margin, wide[1] + packet[1], "MET" if ok else "NOT MET"))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
sc.close()
sys.exit(0 if ok else 1)
