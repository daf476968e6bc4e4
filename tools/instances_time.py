"""What an instanced primary frame costs: Mrays/s of a 1920x1080 frame of snail_instances_trace_primary_dev for N = 1 (the identity
instance alone), 64 and 1024 instances (scenes.instance_field) of the atrium stand-in and of the lancia fixture, in both arithmetics,
beside the plain Scene.trace_primary rate of the same BLAS; and what a per-frame rebuild costs (the reference's -instances mode rebuilds the
top-level tree every frame): the host build (snail_instances_build) and a whole InstancedScene.update() -- build + upload, host wall time --
for --rebuild-counts instances (default 10 000).  Prints one JSON object.  No target: a measurement.

    python tools/instances_time.py [--res 1920x1080] [--reps 5]

--lit: what a LIT instanced frame costs instead (one light, atrium, both arithmetics): ms per frame and Mrays/s (primary rays per second) of
  device      snail_instances_render_whitted_dev, the whole frame in a handful of launches;
  per_packet  the path it replaces in a C++ host: snail_instances_trace_frame_packets for the primary frame, then ONE snail_instances_trace_shadow
              call per packet and light with that packet's shadow rays (prepared beforehand: the host's shading arithmetic between the calls is
              left out, which flatters this path);
  plain       Scene.render_whitted of the BLAS alone with the same camera and light, for scale.
Repeated alternating runs, medians.  --baseline-lib PATH loads another build of libsnailhip.so (e.g. the parent commit's, which has no device
path) and measures per_packet only.

    python tools/instances_time.py --lit [--baseline-lib PATH] [--reps 5]

--tiles: what a TILE-LIST frame costs (snail_instances_render_tiles over render.divide_image's 16x64 tiles; one light, atrium, IEEE): host wall ms
per frame, device-to-host copy and the scatter into the caller's buffer included, of
  tiles          no antialiasing;
  tiles_aa       SNAIL_RENDER_AA4;
  tiles_aa_tint  SNAIL_RENDER_AA4 and the tint of rank 3;
  image          InstancedScene.render_image_host of the same build (the interleaved frame, no tile list), for scale.
Repeated alternating runs, medians.

    python tools/instances_time.py --tiles [--reps 9]

--rebuild-dev: what the per-frame rebuild costs on the device (InstancedScene.update_dev = snail_instances_rebuild_dev, transforms already in
device memory) beside the host path (InstancedScene.update = snail_instances_build + upload, transforms in host memory), for --rebuild-counts
instances (default here 1024,10000): host wall ms per frame of each, synchronised, and the device time of update_dev alone between two events.
Alternating runs (each round: update(), one untimed update_dev, the timed update_dev -- the steady state of a loop that stays on the device),
medians.

    python tools/instances_time.py --rebuild-dev [--rebuild-counts 1024,10000] [--reps 15]

--materials: what FULL shading costs on an instanced frame (include/snail_instances_materials.h; one light, atrium with procedural uv,
normals and materials, both arithmetics): host wall ms per frame, synchronised, of
  full    InstancedMaterialSet.render (snail_instances_render_materials_dev): k_inst_frame, k_imat_sample, k_imat_light, k_mat_final;
  simple  InstancedScene.render_whitted of the same scene, camera and light (simple shading: one colour, plane normals).
Alternating runs, medians.  With --reflections both paths draw the one mirrored bounce of gVals[7]: InstancedMaterialSet.render(reflections=True)
(snail_instances_materials_bounce_dev: + k_mat_mirror, the mirrored packets' walk, k_imat_sample_rays, k_imat_light_rays, k_mat_colour_rays,
k_mat_final_blend) beside InstancedScene.render_whitted(reflections=True).  With --plane-normals every record is flat with its triangle's plane
normal and every material the default: the two paths then draw the same picture from the same rays (the degenerate set of the tests), and
the ratio is the cost of the full-shading stages alone.

    python tools/instances_time.py --materials [--reflections] [--plane-normals] [--reps 3]

--materials --transparency N: what the transparency continuation costs on an instanced full-shaded frame
(include/snail_instances_materials_transparency.h).  The scene of --materials with two of its material classes swapped for kinds that can
select a transparent lane (the second TEX material -> TRANSPARENT with the first texture's first channel as its opacity map, UBER dissolve 0
-> UBER dissolve 0.5); host wall ms per frame, synchronised, alternating runs, medians, of
  transp  InstancedMaterialSet.render_transparent(max_depth=N) (snail_instances_materials_transparent_dev): the way down level by level
          (k_imat_sample_transp, k_mat_continue[_rays], k_imat_trace_level, k_imat_sample_transp_rays), k_mat_truncated, the way back up
          (k_mat_blend_transp, k_imat_light_transp, k_mat_colour_transp), k_imat_light, k_mat_final
  flags0  InstancedMaterialSet.render of the same run: the same scene with the opaque stand-ins the swap replaced
and the lanes level N would still select (the truncated counter of one frame).  Nobody has measured this before: a record, not a gate.

    python tools/instances_time.py --materials --transparency 4 [--reps 5]

--materials --tree [--reflections] [--aa] [--tiles] [--transparency N]: the transparency continuation together with the bounce, 4x antialiasing
and tile lists on an instanced full-shaded frame (include/snail_instances_materials_tree.h), the scene and the capable set of --transparency;
host wall ms per frame, synchronised, median / min / max of the runs, the truncated-lane counter and the number of slices the packet list ran
in, at maxDepth N (default: 1, 4 and 8).  InstancedMaterialSet.tree_frame_packets, or with --tiles .render_tree_tiles_host over the frame cut
into 64x64 tiles (the device-to-host copy and the host's scatter included).  First measurements, not targets.
With --baseline-lib PATH (another build of the library, e.g. the parent commit's) the tool instead starts child processes that alternate between
this build and that one -- this, that, this, that --, each timing the two frames that had a device path before:
  transp   the capable set at maxDepth N (default 4), flags 0: tree_frame_packets here, render_transparent_packets (snail_instances_materials_
           transparent_packets_dev) in the other build -- the same kernels in the same order
  bounce   the opaque set with the one mirrored bounce: tree_frame_packets(RENDER_REFLECTIONS, maxDepth 1) here, render_packets(reflections=True)
           (snail_instances_materials_bounce_packets_dev) in the other build
and prints per row both processes' medians of either build, so that the other build's own run-to-run spread stands beside the difference.

    python tools/instances_time.py --materials --tree --reflections [--aa] [--tiles] [--reps 5]
    python tools/instances_time.py --materials --tree --baseline-lib parent/libsnailhip.so [--transparency 4] [--reps 7]

--materials --heat [--reflections] [--aa] [--tiles] [--transparency N]: the gVals[5] heat-map of an instanced full-shaded frame
(include/snail_instances_materials_heatmap.h) beside the lit frame it replaces, the same arguments, the scene, the capable set and the view of
--materials --tree, the first of --counts instances, maxDepth N (default 4).  ONE process, alternating rounds of --frames calls per variant:
  heat_packets    snail_instances_materials_heat_packets_dev              (with --tiles: heat_tiles, snail_instances_materials_render_heat_tiles)
  tree_packets    snail_instances_materials_tree_frame_packets_dev of this build: the yardstick, its kernels are the parent commit's
  parent_packets  with --baseline-lib PATH: the same call in that build of the library (e.g. the parent commit's), on handles of its own made
                  from the same arrays -- this build's lit call must lie within the run's own min .. max spread of it
Device events around a window enqueued back to back (--tiles: the host clock, call by call); ms per call: median (min .. max); the two launches'
TreeStats are compared first.  The heat launch runs fewer kernels (no blend, no colour stage) plus four atomics per booking wave.  No ratio is a
target: a measurement.  --out PATH appends the report (profiles/instances_materials_heat.txt).

    python tools/instances_time.py --materials --heat [--reflections] [--aa] [--tiles] [--counts 64] [--frames 20] [--reps 5] [--baseline-lib PATH] [--out PATH]

--materials --dynamic: what a frame of k DEFORMING BLASes costs under full shading (include/snail_instances_materials_dynamic.h): k bumpy
sheets of --dyn-tris triangles each (Scene.from_fast_dev), one instance per sheet, one InstancedMaterialSet.from_dev; per frame, ms, median
(min .. max) over --reps windows of --frames back-to-back steps between two device events:
  rebuild_batched   rebuild_blas_dev of all k (the k fast builds in ONE batched pass, include/snail_bvh_fast_batch.h, then ONE k_ishd_pack launch)
  rebuild_single    Scene.rebuild_fast_dev k times, then one update_blas_dev of all k: the builds one after the other with the single-tree
                    kernels, which are the parent commit's -- the yardstick of rebuild_batched, same results
  rebuild_all       rebuild_all_dev: rebuild_batched and top_level in one call (include/snail_instances_materials_rebuild_all.h)
                    (these three take turns window by window, so that what else the machine does falls on all of them alike)
  pack_batched      update_blas_dev of all k in one call: the pack alone (one k_ishd_pack + one k_ishd_info launch)
  pack_single       update_blas_dev k times with one entry each: the pack alone, k times two launches -- what batching is measured against
  top_level         isc.update_dev, which follows every BLAS rebuild
  frame             InstancedMaterialSet.render at --res with one light
  host_route        what a host had to do without the header, on the HOST clock per step: wait for the device, download the k perms,
                    pack_shtris on the CPU, create a set of host records (over a host-built twin of the same trees: the older creator
                    refuses a device-built BLAS) and destroy the previous one
No ratio is a target: a record.  The report says per row what the batched pass is worth against rebuild_single, and whether it is slower than it
by more than rebuild_single's own min .. max spread.  --commit names what was timed; --out PATH writes the report (profiles/bvh_fast_batch.txt;
profiles/instances_materials_dynamic.txt is the record of the commit before the batched pass).

    python tools/instances_time.py --materials --dynamic [--dyn-blas 4,16] [--dyn-tris 2048,20000] [--frames 20] [--reps 5] [--commit ID] [--out PATH]"""
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
    ap.add_argument("--rebuild-counts", default=None)
    ap.add_argument("--rebuild-dev", action="store_true")
    ap.add_argument("--lit", action="store_true")
    ap.add_argument("--tiles", action="store_true")
    ap.add_argument("--materials", action="store_true")
    ap.add_argument("--reflections", action="store_true")
    ap.add_argument("--plane-normals", action="store_true")
    ap.add_argument("--transparency", type=int, default=0, metavar="N")
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--tree", action="store_true")
    ap.add_argument("--aa", action="store_true")
    ap.add_argument("--heat", action="store_true")
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dynamic", action="store_true")
    ap.add_argument("--dyn-blas", default="4,16")
    ap.add_argument("--dyn-tris", default="2048,20000")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--tree-child", default=None, choices=["new", "old"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    resx, resy = (int(x) for x in a.res.split("x"))
    if a.rebuild_dev:
        return rebuild_dev(torch, [int(c) for c in (a.rebuild_counts or "1024,10000").split(",")], a.reps)
    a.rebuild_counts = a.rebuild_counts or "10000"
    if a.materials and a.dynamic:
        return materials_dynamic(torch, a, resx, resy)
    if a.materials and a.heat:
        return materials_heat(torch, a, resx, resy)
    if a.materials and a.tree:
        return materials_tree_compare(a) if a.baseline_lib and not a.tree_child else materials_tree(torch, a, resx, resy)
    if a.lit:
        return lit(torch, a, resx, resy)
    if a.tiles:
        return tiles(torch, a, resx, resy)
    if a.materials and a.transparency:
        return materials_transparency(torch, a, resx, resy)
    if a.materials:
        return materials(torch, a, resx, resy)
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


def shadow_packets_of(isc, cam13, resx, resy, light, t, inst, tri, tris_plane):
    """The shadow packets a host renderer would trace for one light (src/scene_trace.cpp:538-558), from the frame's packet-major hits:
    origin3 [1, 3], dir / idir [np*64, 3, 4], distance [np*64, 4] (-inf = masked).  Plain numpy; not timed."""
    pw, ph = (resx + 15) // 16, (resy + 15) // 16
    n = pw * ph
    q = np.arange(64)
    px = (np.arange(n) % pw * 16)[:, None, None] + (4 * (q & 3))[None, :, None] + np.arange(4)[None, None, :]
    py = (np.arange(n) // pw * 16)[:, None, None] + (q >> 2)[None, :, None] + np.zeros(4, dtype=np.int64)[None, None, :]
    pos, right, up, front, pd = cam13[0:3], cam13[3:6], cam13[6:9], cam13[9:12], cam13[12]
    sx = (px - resx * 0.5) / resy
    sy = (py - resy * 0.5) / resy
    d = right[None, None, None, :] * sx[..., None] + up[None, None, None, :] * sy[..., None] + (front * pd)[None, None, None, :]
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    t = t.reshape(n, 64, 4); inst = inst.reshape(n, 64, 4); tri = tri.reshape(n, 64, 4)
    hit = np.isfinite(t)
    p = pos + d * np.where(hit, t, 0.0)[..., None]
    xs, _ = isc.slot_transforms()
    rot = xs[inst][..., :9].reshape(n, 64, 4, 3, 3)
    nrm = np.einsum("...rc,...c->...r", rot, tris_plane[np.where(hit, tri, 0)])
    lv = p - light[None, None, None, :3]
    dist = np.linalg.norm(lv, axis=-1)
    fl = lv / np.maximum(dist, 1e-20)[..., None]
    cast = hit & ((nrm * fl).sum(-1) > 0)
    fl = np.where(hit[..., None], fl, 0.0)
    sdir = np.ascontiguousarray(np.transpose(fl, (0, 1, 3, 2)), dtype=np.float32).reshape(n * 64, 3, 4)
    with np.errstate(all="ignore"):
        sidir = np.where(sdir != 0, np.float32(1.0) / (sdir + np.float32(1e-8)), np.float32(0.0)).astype(np.float32)
    sdist = np.where(cast, dist * 0.9999, -np.inf).astype(np.float32).reshape(n * 64, 4)
    return np.ascontiguousarray(light[:3], dtype=np.float32).reshape(1, 3), sdir, sidir, sdist, int(cast.sum())


def lit(torch, a, resx, resy):
    import ctypes as C
    import statistics
    import time
    from snail_amd import _lib
    if a.baseline_lib:      # another build of the library for the whole process (it need not have the lit entry points)
        L = C.CDLL(os.path.abspath(a.baseline_lib))
        for table in (_lib.SIGNATURES, _lib.INSTANCES_SIGNATURES):
            for name, (res, args) in table.items():
                fn = getattr(L, name)
                fn.restype, fn.argtypes = res, args
        _lib._lib = L
    L = _lib.lib()
    rays = resx * resy
    pw, ph = (resx + 15) // 16, (resy + 15) // 16
    npk = pw * ph
    tv = scenes.atrium()
    hb = HostBVH.build(tv)
    sc = Scene(hb, 0)
    lo, hi = sc.get_bbox()
    plane = np.ascontiguousarray(hb.tris.view(np.float32).reshape(-1, 16)[:, 12:15])
    out = {"res": a.res, "lights": 1, "library": a.baseline_lib or "this build", "unit": "median of %d alternating runs" % a.reps, "rows": []}
    for arith in ("ieee", "host_sse"):
        sc.set_arith(arith)
        for n in (int(c) for c in a.counts.split(",")):
            rot, tr, bi = scenes.instance_field(lo, hi, n, seed=1)
            isc = InstancedScene([sc], rot, tr, bi)
            nd = isc.nodes()[0]
            cam = survey_camera(tv) if n == 1 else survey_camera(np.concatenate([nd["bmin"], nd["bmax"], nd["bmin"]]).reshape(1, 9))
            cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32)
            c, ext = (nd["bmin"] + nd["bmax"]) * 0.5, nd["bmax"] - nd["bmin"]
            light = np.array([[c[0], c[1] + 0.3 * ext[1], c[2], 1.0, 1.0, 1.0, float(np.linalg.norm(ext))]], dtype=np.float32)
            # the primary frame's hits, packet-major, and from them the shadow packets of the per-packet path
            t = np.zeros(npk * 256, np.float32); u = np.zeros_like(t); v = np.zeros_like(t)
            ins = np.zeros(npk * 256, np.int32); tri = np.zeros_like(ins)
            st = np.zeros(4, np.uint64)

            def frame_packets():
                _lib.check(L.snail_instances_trace_frame_packets(isc._h, _lib.ptr(cam13), resx, resy, _lib.ptr(t), _lib.ptr(u), _lib.ptr(v), _lib.ptr(ins), _lib.ptr(tri),
                                                                 _lib.ptr(st)), "snail_instances_trace_frame_packets")
            frame_packets()
            o3, sdir, sidir, sdist, cast = shadow_packets_of(isc, cam13.astype(np.float64), resx, resy, light[0].astype(np.float64), t, ins, tri, plane)
            work = sdist.copy()

            def per_packet():
                frame_packets()
                np.copyto(work, sdist)
                fn, h, po = L.snail_instances_trace_shadow, isc._h, _lib.ptr(o3)
                base_d, base_i, base_s = sdir.ctypes.data, sidir.ctypes.data, work.ctypes.data
                for p in range(npk):
                    rc = fn(h, 1, 64, po, C.c_void_p(base_d + p * 3072), C.c_void_p(base_i + p * 3072), C.c_void_p(base_s + p * 1024), None)
                    if rc:
                        _lib.check(rc, "snail_instances_trace_shadow")

            frame = torch.zeros((resy, resx, 3), dtype=torch.uint8, device="cuda")
            runs = {"per_packet": per_packet, "plain": lambda: sc.render_whitted(cam, resx, resy, light, out=frame)}
            if not a.baseline_lib:
                runs["device"] = lambda: isc.render_whitted(cam, resx, resy, light, out=frame)
            else:
                del runs["plain"]
            ms = {k: [] for k in runs}
            for k, fn in runs.items():      # warm-up
                fn(); torch.cuda.synchronize()
            for _ in range(a.reps):         # alternating
                for k, fn in runs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
                    ms[k].append((time.perf_counter() - t0) * 1e3)
            row = {"arith": arith, "instances": n, "packets": npk, "shadow_rays": cast}
            for k in ms:
                m = statistics.median(ms[k])
                row[k + "_ms"] = round(m, 3); row[k + "_mrays"] = round(rays / m / 1e3, 1)
            out["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            isc.close()
    sc.close()
    print(json.dumps(out))


def tiles(torch, a, resx, resy):
    import statistics
    import time
    from snail_amd.render import divide_image
    tv = scenes.atrium()
    sc = Scene(HostBVH.build(tv), 0)
    lo, hi = sc.get_bbox()
    tl = divide_image(resx, resy)
    tint = np.array([0.6, 1.0, 1.0], dtype=np.float32)      # rank 3 of src/render.cpp:119-128
    out = {"res": a.res, "lights": 1, "arith": "ieee", "tiles": len(tl), "unit": "host wall ms per frame, median of %d alternating runs" % a.reps, "rows": []}
    for n in (int(c) for c in a.counts.split(",")):
        rot, tr, bi = scenes.instance_field(lo, hi, n, seed=1)
        isc = InstancedScene([sc], rot, tr, bi)
        nd = isc.nodes()[0]
        cam = survey_camera(tv) if n == 1 else survey_camera(np.concatenate([nd["bmin"], nd["bmax"], nd["bmin"]]).reshape(1, 9))
        c, ext = (nd["bmin"] + nd["bmax"]) * 0.5, nd["bmax"] - nd["bmin"]
        light = np.array([[c[0], c[1] + 0.3 * ext[1], c[2], 1.0, 1.0, 1.0, float(np.linalg.norm(ext))]], dtype=np.float32)
        data, offsets, _ = isc.render_tiles_host(cam, resx, resy, tl, light)
        AA = InstancedScene.RENDER_AA4
        runs = {"tiles": lambda: isc.render_tiles_host(cam, resx, resy, tl, light, offsets=offsets, data=data),
                "tiles_aa": lambda: isc.render_tiles_host(cam, resx, resy, tl, light, flags=AA, offsets=offsets, data=data),
                "tiles_aa_tint": lambda: isc.render_tiles_host(cam, resx, resy, tl, light, flags=AA, tint=tint, offsets=offsets, data=data),
                "image": lambda: isc.render_image_host(cam, resx, resy, light)}
        ms = {k: [] for k in runs}
        for k, fn in runs.items():      # warm-up (the cached lists, the handle's sets)
            fn(); fn()
        for _ in range(a.reps):         # alternating
            for k, fn in runs.items():
                t0 = time.perf_counter(); fn()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        row = {"instances": n}
        for k in ms:
            row[k + "_ms"] = round(statistics.median(ms[k]), 3)
            row[k + "_min_ms"] = round(min(ms[k]), 3)
        out["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        isc.close()
    sc.close()
    print(json.dumps(out))


def procedural_shading(hb, tv, seed=7):
    """uv, per-vertex normals (the plane normal bent, not normalised again), material index and flat flags of the INPUT triangles, and a
    material list with every kind the full-shading kernels know: (uv, nrm, mat_index, flat, material_map, materials, textures)"""
    from snail_amd import materials as P
    n = len(tv)
    rng = np.random.RandomState(seed)
    plane = np.zeros((n, 3), dtype=np.float32)
    plane[hb.perm] = hb.tris.view(np.float32).reshape(-1, 16)[:, 12:15]
    plane[~np.isfinite(plane).all(axis=1)] = (0.0, 1.0, 0.0)
    uv = ((rng.rand(n, 1, 2) * 4.0 - 2.0) + (rng.rand(n, 3, 2) - 0.5)).astype(np.float32)
    nrm = (plane[:, None, :] + (rng.rand(n, 3, 3) - 0.5) * 0.6).astype(np.float32)
    ys, xs = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    tex = [np.clip((((xs // 8 + ys // 8) & 1) * 120 + 40)[..., None] + rng.randint(-40, 90, size=(64, 64, 3)), 0, 255).astype(np.uint8),
           rng.randint(0, 256, size=(8, 32, 3)).astype(np.uint8)]
    mats = [P.Material.simple((0.3, 0.8, 0.6), False), P.Material.textured(0, True), P.Material.textured(1, False),
            P.Material.uber((0.9, 0.4, 0.1), (0.2, 0.6, 1.0), 0.0), P.Material.uber((0.2, 0.7, 0.5), (1.0, 0.3, 0.1), 1.0)]
    # materials in runs of 64 input triangles (neighbouring triangles mostly share one, as in a modelled mesh)
    return uv, nrm, ((np.arange(n) // 64) % 6).astype(np.int32), (np.arange(n) % 3) == 1, [-1, 0, 1, 2, 3, 4], mats, [P.Texture(t) for t in tex]


def materials(torch, a, resx, resy):
    import statistics
    import time
    from snail_amd.instances_materials import InstancedMaterialSet
    rays = resx * resy
    tv = scenes.atrium()
    hb = HostBVH.build(tv)
    sc = Scene(hb, 0)
    lo, hi = sc.get_bbox()
    uv, nrm, mi, flat, mmap, mats, texs = procedural_shading(hb, tv)
    if a.plane_normals:
        plane = np.zeros((len(tv), 3), dtype=np.float32)
        plane[hb.perm] = hb.tris.view(np.float32).reshape(-1, 16)[:, 12:15]
        nrm, flat, mi, mmap = np.repeat(plane[:, None, :], 3, axis=1), np.ones(len(tv), dtype=bool), np.zeros(len(tv), dtype=np.int32), [-1]
    refl = bool(a.reflections)
    out = {"res": a.res, "lights": 1, "reflections": refl, "plane_normals": bool(a.plane_normals), "unit": "host wall ms per frame, synchronised, median of %d alternating runs" % a.reps, "rows": []}
    for arith in ("ieee", "host_sse"):
        sc.set_arith(arith)
        for n in (int(c) for c in a.counts.split(",")):
            rot, tr, bi = scenes.instance_field(lo, hi, n, seed=1)
            isc = InstancedScene([sc], rot, tr, bi)
            ms_set = InstancedMaterialSet(isc, [(uv, nrm, mi, flat, mmap)], mats, texs)
            nd = isc.nodes()[0]
            cam = survey_camera(tv) if n == 1 else survey_camera(np.concatenate([nd["bmin"], nd["bmax"], nd["bmin"]]).reshape(1, 9))
            c, ext = (nd["bmin"] + nd["bmax"]) * 0.5, nd["bmax"] - nd["bmin"]
            light = np.array([[c[0], c[1] + 0.3 * ext[1], c[2], 1.0, 1.0, 1.0, float(np.linalg.norm(ext))]], dtype=np.float32)
            frame = torch.zeros((resy, resx, 3), dtype=torch.uint8, device="cuda")
            runs = {"full": lambda: ms_set.render(cam, resx, resy, light, out=frame, reflections=refl),
                    "simple": lambda: isc.render_whitted(cam, resx, resy, light, out=frame, reflections=refl)}
            ms = {k: [] for k in runs}
            for k, fn in runs.items():      # warm-up: the sets' intermediates, the cached packet lists, first launches
                fn(); fn(); torch.cuda.synchronize()
            for _ in range(a.reps):         # alternating
                for k, fn in runs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
                    ms[k].append((time.perf_counter() - t0) * 1e3)
            row = {"arith": arith, "instances": n, "nonblack_pixels": int((frame.cpu().numpy() != 0).any(axis=2).sum())}
            if a.plane_normals:     # the two paths' last frames, byte for byte
                fn_full, fn_simple = runs["full"], runs["simple"]
                fn_full(); full_frame = frame.cpu().numpy().copy()
                fn_simple(); row["frames_equal"] = bool(np.array_equal(full_frame, frame.cpu().numpy()))
            for k in ms:
                m = statistics.median(ms[k])
                row[k + "_ms"] = round(m, 3); row[k + "_min_ms"] = round(min(ms[k]), 3); row[k + "_max_ms"] = round(max(ms[k]), 3); row[k + "_mrays"] = round(rays / m / 1e3, 1)
            row["full_over_simple"] = round(row["full_ms"] / row["simple_ms"], 3)
            out["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            ms_set.close()
            isc.close()
    sc.close()
    print(json.dumps(out))


def materials_transparency(torch, a, resx, resy):
    import statistics
    import time
    from snail_amd import materials as P
    from snail_amd.instances_materials import InstancedMaterialSet
    rays = resx * resy
    depth = int(a.transparency)
    tv = scenes.atrium()
    hb = HostBVH.build(tv)
    sc = Scene(hb, 0)
    lo, hi = sc.get_bbox()
    uv, nrm, mi, flat, mmap, mats, texs = procedural_shading(hb, tv)
    capable = list(mats)
    capable[2] = P.Material.transparent(1, 0, False)                    # TEX over texture 1 -> TRANSPARENT, texture 0's first channel as opacity
    capable[3] = P.Material.uber((0.9, 0.4, 0.1), (0.2, 0.6, 1.0), 0.5)   # UBER dissolve 0 -> 0.5
    out = {"res": a.res, "lights": 1, "max_depth": depth, "unit": "host wall ms per frame, synchronised, median of %d alternating runs" % a.reps, "rows": []}
    for arith in ("ieee", "host_sse"):
        sc.set_arith(arith)
        for n in (int(c) for c in a.counts.split(",")):
            rot, tr, bi = scenes.instance_field(lo, hi, n, seed=1)
            isc = InstancedScene([sc], rot, tr, bi)
            opaque_set = InstancedMaterialSet(isc, [(uv, nrm, mi, flat, mmap)], mats, texs)
            transp_set = InstancedMaterialSet(isc, [(uv, nrm, mi, flat, mmap)], capable, texs, transparent=True)
            nd = isc.nodes()[0]
            cam = survey_camera(tv) if n == 1 else survey_camera(np.concatenate([nd["bmin"], nd["bmax"], nd["bmin"]]).reshape(1, 9))
            c, ext = (nd["bmin"] + nd["bmax"]) * 0.5, nd["bmax"] - nd["bmin"]
            light = np.array([[c[0], c[1] + 0.3 * ext[1], c[2], 1.0, 1.0, 1.0, float(np.linalg.norm(ext))]], dtype=np.float32)
            frame = torch.zeros((resy, resx, 3), dtype=torch.uint8, device="cuda")
            trunc = torch.zeros(1, dtype=torch.int64, device="cuda")
            runs = {"transp": lambda: transp_set.render_transparent(cam, resx, resy, light, out=frame, max_depth=depth, truncated=trunc),
                    "flags0": lambda: opaque_set.render(cam, resx, resy, light, out=frame)}
            ms = {k: [] for k in runs}
            for k, fn in runs.items():      # warm-up: the sets' intermediates (the levels' part among them), the cached packet lists, first launches
                fn(); fn(); torch.cuda.synchronize()
            for _ in range(a.reps):         # alternating
                for k, fn in runs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
                    ms[k].append((time.perf_counter() - t0) * 1e3)
            trunc.zero_()
            st = isc.new_stats()
            transp_set.render_transparent(cam, resx, resy, light, out=frame, max_depth=depth, truncated=trunc, stats=st)
            st0 = isc.new_stats()
            row = {"arith": arith, "instances": n, "nonblack_pixels": int((frame.cpu().numpy() != 0).any(axis=2).sum()), "truncated_lanes": int(trunc.cpu().numpy()[0]),
                   "traced_rays": int(st.cpu().numpy()[2])}
            opaque_set.render(cam, resx, resy, light, out=frame, stats=st0)
            row["flags0_traced_rays"] = int(st0.cpu().numpy()[2])
            for k in ms:
                m = statistics.median(ms[k])
                row[k + "_ms"] = round(m, 3); row[k + "_min_ms"] = round(min(ms[k]), 3); row[k + "_max_ms"] = round(max(ms[k]), 3); row[k + "_mrays"] = round(rays / m / 1e3, 1)
            row["transp_over_flags0"] = round(row["transp_ms"] / row["flags0_ms"], 3)
            out["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            transp_set.close(); opaque_set.close()
            isc.close()
    sc.close()
    print(json.dumps(out))


def tree_scene(a):
    """the scene of --materials --transparency: the atrium BLAS, its procedural shading, the opaque list and the capable one"""
    from snail_amd import materials as P
    tv = scenes.atrium()
    hb = HostBVH.build(tv)
    sc = Scene(hb, 0)
    uv, nrm, mi, flat, mmap, mats, texs = procedural_shading(hb, tv)
    capable = list(mats)
    capable[2] = P.Material.transparent(1, 0, False)                    # TEX over texture 1 -> TRANSPARENT, texture 0's first channel as opacity
    capable[3] = P.Material.uber((0.9, 0.4, 0.1), (0.2, 0.6, 1.0), 0.5)   # UBER dissolve 0 -> 0.5
    return tv, sc, (uv, nrm, mi, flat, mmap), mats, capable, texs


def tree_view(tv, isc, n):
    nd = isc.nodes()[0]
    cam = survey_camera(tv) if n == 1 else survey_camera(np.concatenate([nd["bmin"], nd["bmax"], nd["bmin"]]).reshape(1, 9))
    c, ext = (nd["bmin"] + nd["bmax"]) * 0.5, nd["bmax"] - nd["bmin"]
    return cam, np.array([[c[0], c[1] + 0.3 * ext[1], c[2], 1.0, 1.0, 1.0, float(np.linalg.norm(ext))]], dtype=np.float32)


def tree_times(torch, fn, reps):
    import statistics
    import time
    for _ in range(9):      # warm-up: every one of the set's 8 groups of intermediates has been allocated, the cached lists, first launches
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def materials_tree(torch, a, resx, resy):
    from snail_amd import _lib
    from snail_amd import materials as P
    old = a.tree_child == "old"
    if old:      # the other build has none of the tree's symbols: bind none (the child calls the older entry points alone)
        _lib.INSTANCES_MATERIALS_TREE_SIGNATURES.clear()
    from snail_amd.instances_materials import InstancedMaterialSet
    tv, sc, per_blas, mats, capable, texs = tree_scene(a)
    lo, hi = sc.get_bbox()
    pw, ph = (resx + 15) // 16, (resy + 15) // 16
    xy = torch.from_numpy(np.array([(x * 16, y * 16) for y in range(ph) for x in range(pw)], dtype=np.int32)).cuda()
    flags = (P.RENDER_REFLECTIONS if a.reflections else 0) | (P.RENDER_AA4 if a.aa else 0)
    depths = [int(a.transparency)] if a.transparency else ([4] if a.tree_child else [1, 4, 8])
    out = {"res": a.res, "lights": 1, "flags": flags, "tiles": bool(a.tiles), "library": a.tree_child or "this build",
           "unit": "host wall ms per frame, synchronised, median / min / max of %d runs" % a.reps, "rows": []}
    tiles = np.array([(x, y, 64, 64) for y in range(0, resy, 64) for x in range(0, resx, 64)], dtype=np.int32)
    for arith in ("ieee", "host_sse"):
        sc.set_arith(arith)
        for n in (int(c) for c in a.counts.split(",")):
            rot, tr, bi = scenes.instance_field(lo, hi, n, seed=1)
            isc = InstancedScene([sc], rot, tr, bi)
            cam, light = tree_view(tv, isc, n)
            bgr = torch.zeros((pw * ph, 256, 3), dtype=torch.uint8, device="cuda")
            trunc = torch.zeros(1, dtype=torch.int64, device="cuda")
            transp_set = InstancedMaterialSet(isc, [per_blas], capable, texs, transparent=True)
            if a.tree_child:      # the two frames that had a device path before, by this build's new entry point or the other build's old one
                opaque_set = InstancedMaterialSet(isc, [per_blas], mats, texs)
                d = depths[0]
                if old:
                    runs = {"transp": lambda: transp_set.render_transparent_packets(cam, resx, resy, xy, light, out=bgr, max_depth=d, truncated=trunc),
                            "bounce": lambda: opaque_set.render_packets(cam, resx, resy, xy, light, out=bgr, reflections=True)}
                else:
                    runs = {"transp": lambda: transp_set.tree_frame_packets(cam, resx, resy, xy, light, 0, out=bgr, max_depth=d, truncated=trunc),
                            "bounce": lambda: opaque_set.tree_frame_packets(cam, resx, resy, xy, light, P.RENDER_REFLECTIONS, out=bgr, max_depth=1, truncated=trunc)}
                row = {"arith": arith, "instances": n, "max_depth": d}
                for k, fn in runs.items():
                    row[k] = tree_times(torch, fn, a.reps)
                    row[k]["checksum"] = int(bgr.sum().item())
                out["rows"].append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
                opaque_set.close()
            else:
                for d in depths:
                    one = transp_set.level_bytes(1, flags, d)
                    row = {"arith": arith, "instances": n, "max_depth": d, "slices": -(-(pw * ph) // max(1, min(pw * ph, (1 << 30) // one)))}
                    if a.tiles:
                        ht = np.zeros(1, dtype=np.uint64)
                        fn = lambda: transp_set.render_tree_tiles_host(cam, resx, resy, tiles, None, light, flags, max_depth=d, truncated=ht)      # noqa: E731
                    else:
                        fn = lambda: transp_set.tree_frame_packets(cam, resx, resy, xy, light, flags, out=bgr, max_depth=d, truncated=trunc)      # noqa: E731
                    row.update(tree_times(torch, fn, a.reps))
                    trunc.zero_()
                    st = isc.new_stats()
                    transp_set.tree_frame_packets(cam, resx, resy, xy, light, flags, out=bgr, max_depth=d, truncated=trunc, stats=st)
                    row["truncated_lanes"] = int(trunc.cpu().numpy()[0]); row["traced_rays"] = int(st.cpu().numpy()[2])
                    out["rows"].append(row)
                    print(json.dumps(row), file=sys.stderr, flush=True)
            transp_set.close()
            isc.close()
    sc.close()
    print(json.dumps(out))


def materials_tree_compare(a):
    """children alternating between this build and --baseline-lib: this, that, this, that; one JSON line with both processes' figures per row"""
    import subprocess
    base = [sys.executable, os.path.abspath(__file__), "--materials", "--tree", "--res", a.res, "--reps", str(a.reps), "--counts", a.counts,
            "--transparency", str(a.transparency or 4), "--baseline-lib", a.baseline_lib]
    res = {"new": [], "old": []}
    for which in ("new", "old", "new", "old"):
        env = dict(os.environ)
        if which == "old":
            env["SNAIL_LIB_PATH"] = os.path.abspath(a.baseline_lib)
        r = subprocess.run(base + ["--tree-child", which], env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            raise SystemExit("child %s failed with status %d" % (which, r.returncode))
        res[which].append(json.loads(r.stdout.strip().splitlines()[-1]))
    rows = []
    for i, r0 in enumerate(res["new"][0]["rows"]):
        for k in ("transp", "bounce"):
            new = [p["rows"][i][k] for p in res["new"]]
            old = [p["rows"][i][k] for p in res["old"]]
            row = {"arith": r0["arith"], "instances": r0["instances"], "frame": k, "max_depth": r0["max_depth"] if k == "transp" else 1,
                   "this_ms": [x["ms"] for x in new], "this_max_ms": [x["max_ms"] for x in new], "other_ms": [x["ms"] for x in old], "other_max_ms": [x["max_ms"] for x in old],
                   "frames_equal": len({x["checksum"] for x in new + old}) == 1}
            row["other_spread"] = round(max(row["other_ms"]) / min(row["other_ms"]), 4)
            row["this_over_other"] = round((sum(row["this_ms"]) / len(new)) / (sum(row["other_ms"]) / len(old)), 4)
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps({"res": a.res, "lights": 1, "other": a.baseline_lib, "unit": res["new"][0]["unit"] + "; per build the medians of its two processes", "rows": rows}))


class OtherBuild:
    """Another build of the library (--baseline-lib) in THIS process: bound with this build's signature tables as far as it exports them, and
    swapped in as snail_amd._lib's library while its handles are made, called or closed."""

    def __init__(self, path):
        import ctypes as C

        from snail_amd import _lib
        self._lib = _lib
        self.L = C.CDLL(os.path.abspath(path))
        for key, table in vars(_lib).items():
            if key.endswith("SIGNATURES"):
                for name, (res, args) in table.items():
                    fn = getattr(self.L, name, None)
                    if fn is not None:
                        fn.restype, fn.argtypes = res, args

    def __enter__(self):
        self.prev = self._lib.lib()
        self._lib._lib = self.L
        return self

    def __exit__(self, *exc):
        self._lib._lib = self.prev


def materials_heat(torch, a, resx, resy):
    """--materials --heat: the heat-map beside the lit frame it replaces, and beside the same lit call of --baseline-lib"""
    import statistics
    import time

    from snail_amd import materials as P
    from snail_amd.instances_materials import InstancedMaterialSet
    if not torch.cuda.is_available():
        raise SystemExit("instances_time.py measures on the GPU; there is none here")
    flags = (P.RENDER_REFLECTIONS if a.reflections else 0) | (P.RENDER_AA4 if a.aa else 0)
    depth = int(a.transparency) if a.transparency else 4
    n = int(a.counts.split(",")[0])
    pw, ph = (resx + 15) // 16, (resy + 15) // 16
    xy = torch.from_numpy(np.array([(x * 16, y * 16) for y in range(ph) for x in range(pw)], dtype=np.int32)).cuda()
    tiles = np.array([(x, y, 64, 64) for y in range(0, resy, 64) for x in range(0, resx, 64)], dtype=np.int32)
    data = np.zeros(int((3 * tiles[:, 2].astype(np.int64) * tiles[:, 3]).sum()), dtype=np.uint8)

    def build():
        """the scene, the instances and the capable set in whichever build is snail_amd._lib's at the moment"""
        tv, sc, per_blas, mats, capable, texs = tree_scene(a)
        lo, hi = sc.get_bbox()
        rot, tr, bi = scenes.instance_field(lo, hi, n, seed=1)
        isc = InstancedScene([sc], rot, tr, bi)
        cam, light = tree_view(tv, isc, n)
        return sc, isc, InstancedMaterialSet(isc, [per_blas], capable, texs, transparent=True), cam, light, len(tv)

    sc, isc, ms, cam, light, ntris = build()
    other = OtherBuild(a.baseline_lib) if a.baseline_lib else None
    if other:
        with other:
            osc, oisc, oms, _, _, _ = build()
    out = [torch.zeros((pw * ph, 256, 3), dtype=torch.uint8, device="cuda") for _ in range(3)]
    trunc = torch.zeros(1, dtype=torch.int64, device="cuda")
    htrunc = np.zeros(1, dtype=np.uint64)

    def in_other(fn):
        def run(s=None):
            with other:
                return fn(s)
        return run
    if a.tiles:
        variants = {"tree_tiles": lambda s=None: ms.render_tree_tiles_host(cam, resx, resy, tiles, None, light, flags, data=data, max_depth=depth, truncated=htrunc),
                    "heat_tiles": lambda s=None: ms.render_heat_tiles_host(cam, resx, resy, tiles, None, light, flags, data=data, max_depth=depth, truncated=htrunc)}
        if other:
            variants["parent_tiles"] = in_other(lambda s=None: oms.render_tree_tiles_host(cam, resx, resy, tiles, None, light, flags, data=data, max_depth=depth, truncated=htrunc))
    else:
        variants = {"tree_packets": lambda s=None: ms.tree_frame_packets(cam, resx, resy, xy, light, flags, out=out[0], stats=s, max_depth=depth, truncated=trunc),
                    "heat_packets": lambda s=None: ms.render_heat_packets(cam, resx, resy, xy, light, flags, out=out[1], stats=s, max_depth=depth, truncated=trunc)}
        if other:
            variants["parent_packets"] = in_other(lambda s=None: oms.tree_frame_packets(cam, resx, resy, xy, light, flags, out=out[2], stats=s, max_depth=depth, truncated=trunc))
    for fn in variants.values():        # warm-up: code objects, every group of the set's intermediates at its largest, the cached lists and tile job
        for _ in range(9):
            fn()
    torch.cuda.synchronize()
    if a.tiles:
        got = [np.asarray(fn()[2]) for fn in variants.values()]
    else:
        st = [isc.new_stats() for _ in variants]
        for fn, s in zip(variants.values(), st):
            fn(s)
        torch.cuda.synchronize()
        got = [s.cpu().numpy() for s in st]
    same = all(bool(np.array_equal(got[0], g)) for g in got[1:])
    lit_equal = (not other) or a.tiles or bool(torch.equal(out[0], out[2]))
    times = {k: [] for k in variants}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.reps):
        for k, fn in variants.items():      # alternating: one window of each per round
            if a.tiles:
                t0 = time.perf_counter()
                for _ in range(a.frames):
                    fn()
                times[k].append((time.perf_counter() - t0) * 1e3 / a.frames)
            else:
                e0.record()
                for _ in range(a.frames):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / a.frames)
    med = {k: statistics.median(v) for k, v in times.items()}
    names = list(med)
    lit, hm = names[0], names[1]
    ratio = med[hm] / med[lit]
    what = ("snail_instances_materials_tree_render_tiles", "snail_instances_materials_render_heat_tiles") if a.tiles else (
        "snail_instances_materials_tree_frame_packets_dev", "snail_instances_materials_heat_packets_dev")
    lines = ["", "the heat-map under full shading of an instanced scene: atrium BLAS (%d triangles) x %d instances, the capable set of --materials --tree, one light, IEEE, "
             "%dx%d (%d packets), flags %s%s, max_depth %d; %d rounds of %d calls per variant, alternating, after 9 warm-up calls each; %s, ms per call: median (min .. max)" % (
                 ntris, n, resx, resy, pw * ph, "REFLECTIONS " if a.reflections else "", "AA4" if a.aa else "", depth, a.reps, a.frames,
                 "host clock, call by call (each call ends in its device-to-host copy)" if a.tiles else "device events around a window enqueued back to back"),
             "device: %s" % torch.cuda.get_device_name(0),
             "%s = %s; %s = %s, the same arguments%s" % (lit, what[0], hm, what[1], "; %s = %s of the parent commit's build, in the same process" % (names[2], what[0]) if other else ""),
             "TreeStats of the launches equal: %s (%s)%s" % (same, np.asarray(got[1]).tolist(), "" if a.tiles or not other else "; lit bytes of the two builds equal: %s" % lit_equal)]
    for k, v in times.items():
        lines.append("  %-15s %9.3f  (%.3f .. %.3f)" % (k, med[k], min(v), max(v)))
    lines.append("  %s / %s: %.3f%s" % (hm, lit, ratio, "   -- the heat-map is SLOWER than the frame it replaces" if ratio > 1.0 else ""))
    if other:
        pk = names[2]
        lo_, hi_ = min(min(times[pk]), min(times[lit])), max(max(times[pk]), max(times[lit]))
        inside = min(times[pk]) <= med[lit] <= max(times[pk]) or min(times[lit]) <= med[pk] <= max(times[lit])
        lines.append("  %s / %s: %.4f; the run's own spread of the two lit calls: %.3f .. %.3f (max / min %.4f); one build's median within the other's min .. max: %s" % (
            lit, pk, med[lit] / med[pk], lo_, hi_, hi_ / lo_, inside))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(text + "\n")
    if other:
        with other:
            oms.close(); oisc.close(); osc.close()
    ms.close(); isc.close(); sc.close()
    if not same or not lit_equal:
        raise SystemExit("the heat launch's TreeStats differ from the lit frame's, or the two builds' lit frames differ")


def bumpy_sheet(n_tris, phase, amp=0.25):
    """a g x g grid of quads (2 g^2 >= n_tris triangles, cut to n_tris) over [-1, 1]^2, z a smooth function of the position and the phase"""
    g = int(np.ceil(np.sqrt(n_tris / 2.0)))
    u = np.linspace(-1.0, 1.0, g + 1)
    x, y = np.meshgrid(u, u, indexing="ij")
    z = amp * np.sin(2.3 * x + phase) * np.cos(1.7 * y - 0.5 * phase)
    p = np.stack([x, y, z], axis=-1).astype(np.float32)
    a, b, c, d = p[:-1, :-1], p[1:, :-1], p[1:, 1:], p[:-1, 1:]
    tris = np.stack([np.stack([a, b, c], axis=2), np.stack([a, c, d], axis=2)], axis=2).reshape(-1, 3, 3)
    return np.ascontiguousarray(tris[:n_tris], dtype=np.float32)


def materials_dynamic(torch, a, resx, resy):
    import statistics
    import subprocess
    import time
    from snail_amd import materials as P
    from snail_amd.instances_materials import DevBlasShading, InstancedMaterialSet
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "describe", "--always", "--dirty"], capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = "unknown"
    dv = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")      # noqa: E731
    lines = ["instanced full shading of k deforming BLASes (tools/instances_time.py --materials --dynamic), one MI355X, commit %s" % commit,
             "frame %dx%d, one light; ms per step: median (min .. max) of %d windows of %d back-to-back steps between device events; host_route on the host clock" % (resx, resy, a.reps, a.frames),
             ""]
    rows = []

    def window(step):
        step(); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(a.reps):
            e0.record()
            for f in range(a.frames):
                step(f)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / a.frames)
        return ms

    def alternating(steps):
        """window()'s figures for several steps that take turns, window by window"""
        for step in steps.values():
            step()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = {name: [] for name in steps}
        for _ in range(a.reps):
            for name, step in steps.items():
                e0.record()
                for f in range(a.frames):
                    step(f)
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1) / a.frames)
        return ms

    for n_tris in (int(c) for c in a.dyn_tris.split(",")):
        for k in (int(c) for c in a.dyn_blas.split(",")):
            rng = np.random.RandomState(5)
            tv = [[bumpy_sheet(n_tris, ph + 0.37 * b) for ph in (0.0, 0.9)] for b in range(k)]
            n = len(tv[0][0])
            uv = ((rng.rand(n, 1, 2) * 4.0 - 2.0) + (rng.rand(n, 3, 2) - 0.5)).astype(np.float32)
            mi = ((np.arange(n) // 64) % 6).astype(np.int32)
            flat = ((np.arange(n) % 3) == 1).astype(np.uint8)
            ys, xs = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
            texs = [P.Texture(np.clip((((xs // 8 + ys // 8) & 1) * 120 + 40)[..., None] + rng.randint(-40, 90, size=(64, 64, 3)), 0, 255).astype(np.uint8))]
            mats = [P.Material.simple((0.3, 0.8, 0.6), False), P.Material.textured(0, True), P.Material.simple((0.8, 0.3, 0.2), True),
                    P.Material.uber((0.9, 0.4, 0.1), (0.2, 0.6, 1.0), 0.0), P.Material.uber((0.2, 0.7, 0.5), (1.0, 0.3, 0.1), 1.0)]
            mmap = [-1, 0, 1, 2, 3, 4]
            d_tv = [[dv(t) for t in pair] for pair in tv]
            scs = [Scene.from_fast_dev(d_tv[b][0], 0) for b in range(k)]
            side = int(np.ceil(np.sqrt(k)))
            tr = np.array([[2.2 * (b % side), 2.2 * (b // side), 0.0] for b in range(k)], dtype=np.float32)
            rot = np.stack([np.eye(3, dtype=np.float32)] * k)
            bi = np.arange(k, dtype=np.int32)
            isc = InstancedScene(scs, rot, tr, bi)
            d_uv, d_mi, d_flat = dv(uv), dv(mi), dv(flat)
            ms_set = InstancedMaterialSet.from_dev(isc, [DevBlasShading(d_uv, d_mi, d_flat, mmap, d_verts=d_tv[b][0]) for b in range(k)], mats, texs)
            d_xf, d_bi = dv(np.concatenate([rot.reshape(k, 9), tr], axis=1).astype(np.float32)), dv(bi)
            isc.update_dev(d_xf, d_bi)
            nd = isc.nodes()[0]
            cam = survey_camera(np.concatenate([nd["bmin"], nd["bmax"], nd["bmin"]]).reshape(1, 9))
            c, ext = (nd["bmin"] + nd["bmax"]) * 0.5, nd["bmax"] - nd["bmin"]
            light = np.array([[c[0], c[1], c[2] - 1.5 * float(np.linalg.norm(ext)), 1.0, 1.0, 1.0, 4.0 * float(np.linalg.norm(ext))]], dtype=np.float32)
            frame = torch.zeros((resy, resx, 3), dtype=torch.uint8, device="cuda:0")
            def rebuild_single(f=0):
                for b in range(k):
                    scs[b].rebuild_fast_dev(d_tv[b][f & 1])
                ms_set.update_blas_dev({b: (None, d_tv[b][f & 1]) for b in range(k)})

            rebuilds = {
                "rebuild_batched": lambda f=0: ms_set.rebuild_blas_dev({b: (d_tv[b][f & 1], None) for b in range(k)}),
                "rebuild_single": rebuild_single,
                "rebuild_all": lambda f=0: ms_set.rebuild_all_dev({b: (d_tv[b][f & 1], None) for b in range(k)}, d_xf, d_bi),
            }
            row = {"k": k, "tris_per_blas": n}
            for name, ms in alternating(rebuilds).items():
                row[name] = (statistics.median(ms), min(ms), max(ms))
            steps = {
                "pack_batched": lambda f=0: ms_set.update_blas_dev({b: (None, d_tv[b][1]) for b in range(k)}),
                "pack_single": lambda f=0: [ms_set.update_blas_dev({b: (None, d_tv[b][1])}) for b in range(k)],
                "top_level": lambda f=0: isc.update_dev(d_xf, d_bi),
                "frame": lambda f=0: ms_set.render(cam, resx, resy, light, out=frame),
            }
            for name, step in steps.items():
                if name == "pack_batched":      # (the packs run on the last pose the rebuilds left: pose index (frames - 1) & 1 = 1 for an even count)
                    ms_set.rebuild_blas_dev({b: (d_tv[b][1], None) for b in range(k)})
                ms = window(step)
                row[name] = (statistics.median(ms), min(ms), max(ms))
            row["nonblack_pixels"] = int((frame.cpu().numpy() != 0).any(axis=2).sum())
            # the host route, over a host-built twin of the trees the handle holds now (pose 1)
            tw = [Scene.from_fast(tv[b][1], 0) for b in range(k)]
            tisc = InstancedScene(tw, rot, tr, bi)
            nrm = [np.repeat(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])[:, None, :], 3, axis=1).astype(np.float32) for t in (tv[b][1] for b in range(k))]
            prev, host = None, []
            for _ in range(max(a.reps, 3)):
                t0 = time.perf_counter()
                torch.cuda.synchronize()
                perms = [scs[b].d_perm.cpu().numpy() for b in range(k)]
                sh = [P.pack_shtris(uv, nrm[b], mi, flat, perms[b]) for b in range(k)]
                new = InstancedMaterialSet.__new__(InstancedMaterialSet)
                new.isc, new.shtris = tisc, sh
                from snail_amd.instances_materials import create_instanced_set
                new._h = create_instanced_set(tisc._h, sh, [mmap] * k, mats, texs)
                if prev is not None:
                    prev.close()
                prev = new
                host.append((time.perf_counter() - t0) * 1e3)
            prev.close()
            row["host_route"] = (statistics.median(host), min(host), max(host))
            rows.append(row)
            print(json.dumps({kk: ([round(x, 4) for x in v] if isinstance(v, tuple) else v) for kk, v in row.items()}), file=sys.stderr, flush=True)
            tisc.close()
            for s in tw:
                s.close()
            ms_set.close(); isc.close()
            for s in scs:
                s.close()
    cols = ["rebuild_batched", "rebuild_single", "rebuild_all", "pack_batched", "pack_single", "top_level", "frame", "host_route"]
    lines.append("%4s %9s  " % ("k", "tris/BLAS") + "  ".join("%-26s" % c for c in cols))
    for r in rows:
        lines.append("%4d %9d  " % (r["k"], r["tris_per_blas"]) + "  ".join("%-26s" % ("%.3f (%.3f .. %.3f)" % r[c]) for c in cols))
    lines.append("")
    for r in rows:
        lines.append("k = %d, %d triangles each: k single-entry packs take %.2f x the batched pack (%.3f ms against %.3f ms per frame); the pack is %.1f %% of the "
                     "batched rebuild; %d non-black pixels in the frame" % (r["k"], r["tris_per_blas"], r["pack_single"][0] / r["pack_batched"][0], r["pack_single"][0],
                                                                            r["pack_batched"][0], 100.0 * r["pack_batched"][0] / r["rebuild_batched"][0], r["nonblack_pixels"]))
    lines.append("")
    lines.append("the batched pass against k single builds (rebuild_single: the parent commit's kernels and launch count), medians of the same run:")
    for r in rows:
        b, s1, al = r["rebuild_batched"], r["rebuild_single"], r["rebuild_all"]
        spread = s1[2] - s1[1]
        verdict = "not slower" if b[0] <= s1[0] else ("slower, within rebuild_single's spread" if b[0] - s1[0] <= spread else "SLOWER by more than rebuild_single's spread")
        lines.append("k = %d, %d triangles each: rebuild_single / rebuild_batched = %.2f (%.3f ms against %.3f ms; rebuild_single's min .. max spread %.3f ms): %s; "
                     "rebuild_all %.3f ms against rebuild_batched + top_level = %.3f ms" % (r["k"], r["tris_per_blas"], s1[0] / b[0], s1[0], b[0], spread, verdict, al[0],
                                                                                             b[0] + r["top_level"][0]))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


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


def rebuild_dev(torch, counts, reps):
    import statistics
    import time
    tv = scenes.atrium()
    sc = Scene(HostBVH.build(tv), 0)
    lo, hi = sc.get_bbox()
    out = {"unit": "ms per rebuild, median of %d alternating runs" % reps, "rows": []}
    for n in counts:
        frames = []
        for k in range(4):          # a few different fields, so that no run rebuilds what it has just built
            rot, tr, bi = scenes.instance_field(lo, hi, n, seed=3 + k)
            xf = np.ascontiguousarray(np.concatenate([rot.reshape(-1, 9), tr], axis=1), dtype=np.float32)
            frames.append((rot, tr, bi, torch.from_numpy(xf).cuda(), torch.from_numpy(bi).cuda()))
        isc = InstancedScene([sc], frames[0][0], frames[0][1], frames[0][2])
        info = torch.empty(4, dtype=torch.int32, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = {"update_host": [], "update_dev": [], "update_dev_device": []}
        for k in range(reps + 2):   # (two warm-up rounds: buffer growth, first launches)
            rot, tr, bi, d_xf, d_bi = frames[k % len(frames)]
            torch.cuda.synchronize()
            t0 = time.perf_counter(); isc.update(rot, tr, bi); torch.cuda.synchronize(); t1 = time.perf_counter()
            isc.update_dev(d_xf, d_bi, info=info)       # (untimed: the first update_dev after an update() re-seeds the scene's device copy of perm)
            torch.cuda.synchronize()
            e0.record()
            t2 = time.perf_counter(); isc.update_dev(d_xf, d_bi, info=info); e1.record(); torch.cuda.synchronize(); t3 = time.perf_counter()
            if k >= 2:
                ms["update_host"].append((t1 - t0) * 1e3)
                ms["update_dev"].append((t3 - t2) * 1e3)
                ms["update_dev_device"].append(e0.elapsed_time(e1))
        assert int(info.cpu()[0]) == 0
        row = {"instances": n}
        for k, v in ms.items():
            row[k + "_ms"] = round(statistics.median(v), 4)
            row[k + "_min_ms"] = round(min(v), 4)
        row["host_over_dev"] = round(row["update_host_ms"] / row["update_dev_ms"], 2)
        out["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        isc.close()
    sc.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
