"""Build time of a plain scene's tree, four ways, and the primary-frame rate on each tree (include/snail_bvh_fast.h).
  (a) snail_bvh_build (host SAH sweep) + snail_scene_create            -- the parity tree
  (b) snail_scene_create_lbvh                                          -- NOT a parity tree
  (c) snail_bvh_build_fast (host, the reference's 16-bin builder) + snail_scene_create
  (d) snail_scene_create_fast_dev and snail_scene_rebuild_fast_dev     -- (c)'s bytes, built on the device; device time by events
Usage: python tools/build_time.py [atrium|stress-1M ...] [--no-sweep]   (the sweep over a million triangles takes minutes)"""
import os
import sys
import time
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from snail_amd import FPSCamera, HostBVH, scenes
from snail_amd.render import DistributedRenderer
from snail_amd.scene import Scene

names = [a for a in sys.argv[1:] if not a.startswith("--")] or ["atrium", "stress-1M"]
sweep = "--no-sweep" not in sys.argv
resx, resy = 1920, 1080
print("GPU_MAX_HW_QUEUES=%s (this tool's default is 8, as the project's other timing tools)" % os.environ["GPU_MAX_HW_QUEUES"])


def wall(fn):
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


def frame_ms(sc, cam):
    rnd = DistributedRenderer(sc, resx, resy, 0, 1, slots=4)
    ms = 0.0
    for rep in range(3):
        for _ in range(20): rnd.render(cam)
        rnd.flush(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(100): rnd.render(cam)
        rnd.flush(); torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / 100 * 1e3
    return ms


for name in names:
    tv = np.ascontiguousarray(scenes.scene_by_name(name).reshape(-1, 9), np.float32)
    pos, ang, pitch = scenes.atrium_camera() if name.startswith("atrium") else scenes.stress_camera()
    cam = FPSCamera(pos, ang, pitch).camera()
    print("%s: %d triangles" % (name, len(tv)))
    trees = []
    if sweep:
        hb, t_b = wall(lambda: HostBVH.build(tv))
        sc, t_c = wall(lambda: Scene(hb, 0))
        print("  (a) host sweep      %10.1f ms build + %7.1f ms create -> %d nodes, depth %d" % (t_b, t_c, hb.n_nodes, hb.depth))
        trees.append(("sweep", sc))
    Scene.from_lbvh(tv, 0, 4).close()
    lb, t_lb = wall(lambda: Scene.from_lbvh(tv, 0, 4))
    print("  (b) LBVH (device)   %10.2f ms of kernels, %7.1f ms the call" % (lb.build_ms, t_lb))
    trees.append(("lbvh", lb))
    hf, t_b = wall(lambda: HostBVH.build_fast(tv))
    sf, t_c = wall(lambda: Scene(hf, 0))
    print("  (c) host fast       %10.1f ms build + %7.1f ms create -> %d nodes, depth %d" % (t_b, t_c, hf.n_nodes, hf.depth))
    trees.append(("fast", sf))
    dv = torch.from_numpy(tv).cuda()
    Scene.from_fast_dev(dv, 0).close()
    sd, t_d = wall(lambda: Scene.from_fast_dev(dv, 0))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e30
    for rep in range(5):
        e0.record(); sd.rebuild_fast_dev(dv); e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    same = sd.bvh.nodes.tobytes() == hf.nodes.tobytes() and sd.bvh.tris.tobytes() == hf.tris.tobytes()
    print("  (d) device fast     %10.2f ms rebuild (events, best of 5), %7.1f ms create call; bytes equal to (c): %s" % (best, t_d, same))
    sd.close()      # (the device-built handle and its builder scratch are released before the frames are timed)
    del dv
    for label, sc in trees:
        print("  primary frame on the %-5s tree: %.4f ms at %dx%d" % (label, frame_ms(sc, cam), resx, resy))
    for label, sc in trees:
        sc.close()
