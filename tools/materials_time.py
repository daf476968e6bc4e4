"""What full shading costs: ms per 1920x1080 frame of the atrium stand-in with one light, IEEE arithmetic, of
  whitted        snail_render_whitted_dev (simple shading; with --parent-lib PATH: of THAT build of libsnailhip.so, e.g. the parent commit's,
                 loaded beside the product library; without it: of the product build, and labelled so),
  default_flat   MaterialSet.render with every material the default and every triangle flat with its plane normal (the same picture),
  textured       MaterialSet.render with the tests' textured set (tests/materials_cases.py: materials by input index mod 5, uv in [-3, 3],
                 bent vertex normals),
and the sample stage alone (snail_materials_shade_packets_dev over the frame's packets, textured set).  Every figure: device events around a
window of --frames frames enqueued back to back (400: a fifth of a second per window for the frames), the variants alternating, --reps
rounds, medians (and the spread).  For the sample stage that figure is the launch-to-launch interval of back-to-back launches, an upper bound
on its kernel time; the kernel time itself comes from a kernel trace of a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/materials_time.py --trace 50
(--trace N: N textured frames and N launches of the sample stage after the warm-up, nothing timed, nothing written).  The frames of
whitted and default_flat are compared byte for byte before anything is timed.  No threshold: a measurement.  Writes the report to --out
(default: stdout only).  The shading data comes from the tests' case helpers (tests/materials_cases.py: vertex_data, plane_normals,
materials_mod5, TEXTURES), which are handed the product's HostBVH where they document an OracleScene -- they read only .tris["plane"] and
.perm, which both carry; importing them imports tests/oracle_lib.py but never loads or builds the oracle library.

--reflections: the same measurement of the one mirrored bounce of gVals[7] (include/snail_materials_bounce.h) instead -- whitted_refl
(snail_render_whitted_dev with SNAIL_WHITTED_REFLECTIONS, the simple-shading bounce, always of THIS build), default_flat_refl and
textured_refl (MaterialSet.render(reflections=True)), and the three stages that have entry points of their own, launch to launch over the
frame's packets with the textured set: mirror (snail_materials_mirror_packets_dev), mirror+walk (that and snail_trace_rays_dev with masks and
barycentrics) and sample_rays (snail_materials_shade_rays_dev).  The frames of whitted_refl and default_flat_refl are compared byte for
byte first.  The kernels' own times, the nested light and colour stages included, come from a kernel trace of --reflections --trace N.

--tiles [--aa]: snail_materials_render_tiles (include/snail_materials_tiles.h) over the reference's 16x64 tile map of the frame (divide_image),
textured set, without and with the bounce (and, with --aa, under SNAIL_RENDER_AA4 as well), beside the per-frame time of
snail_materials_bounce_dev at the same resolution in the same run.  The tile call is a host call -- it returns after its one device-to-host copy
-- so it is timed on the host's clock, one call after the other; the frame call is timed by device events around a window enqueued back to
back, and once more call by call with a wait after each, which is the like-for-like figure.  No threshold: a measurement.  --out APPENDS in
this mode, with --commit as the label of what was measured.

--transparency N: frames with the transparency continuation (include/snail_materials_transparency.h), at most N levels deep, of the tests'
`panes` case (tests/materials_transparency_cases.py: five panes and a wall, 12 triangles) at its own 96x64 and at 1920x1080 --
snail_materials_transparent_dev -- beside snail_render_materials_dev on the same set rebuilt with opaque stand-ins, in the same run, both by
device events around windows enqueued back to back.  No rate is promised: the rows are the record.  --out APPENDS, --commit labels.

--tree [--reflections] [--aa] [--tiles]: the continuation TOGETHER with the bounce, 4x AA and tile lists (include/snail_materials_tree.h) on the
tests' `room` case (tests/materials_tree_cases.py: `panes` and a wall behind the camera, 14 triangles) at --res, max_depth 8 --
snail_materials_tree_render_frame (with --tiles: snail_materials_tree_render_tiles over the 16x64 tile map) with the flags asked for -- beside,
in the same run and the same build, snail_materials_transparent_image (flags = 0) on the same set and snail_materials_render_tiles with the same
flags on the set rebuilt with opaque stand-ins.  All three are host calls that return after their device-to-host copy: host clock, call by
call, after a warm-up, the variants alternating, --reps rounds of --frames calls, median (min .. max).  No threshold: a measurement.  --out APPENDS.

--dynamic [--sheet NUxNV]: a DEFORMING mesh under full shading (include/snail_materials_dynamic.h): the tests' patch scene
(tests/materials_cases.py: patch_scene, a sheet of NU x NV quads, textured set by input index mod 5) alternating between two poses, one
rebuild and one frame at --res per step, in the same run and alternating:
  dynamic      MaterialSet.rebuild_dev + .render on one stream, nothing waited for: device events around a window of --frames steps;
  host_route   what a caller had to do without that header: Scene.rebuild_fast_dev, a host wait, the perm downloaded, pack_shtris on the host,
               a new set over the rebuilt handle through the C-ABI (snail_materials_create, every texture uploaded again; the Python class
               refuses such a scene), .render, the old set destroyed -- timed by the HOST clock, a wait at the end of the window, because
               it contains host work;
  build_alone  Scene.rebuild_fast_dev alone (k_fast_* and the builder's kernels), device events;
  repack_alone MaterialSet.update_dev alone (k_shd_pack), device events, launch to launch.
The two routes' last frames are compared byte for byte first.  No rate is promised: the rows are the record.  --out APPENDS.

--heat [--reflections] [--aa] [--tiles]: the gVals[5] heat-map under full shading (include/snail_materials_heatmap.h) on the `room` case at --res,
max_depth 8, beside the lit frame it replaces, with the same arguments, in the same run and the same build, the two alternating:
snail_materials_heat_packets_dev against snail_materials_tree_frame_packets_dev over the frame's packet list, both asynchronous -- device events
around a window of --frames launches enqueued back to back; with --tiles snail_materials_render_heat_tiles against
snail_materials_tree_render_tiles over the 16x64 tile map, host calls that return after their device-to-host copy -- host clock, call by call.
The heat launch runs fewer kernels (no blend, no colour stage) plus a few atomics per wave; the report states both times and their ratio, and
says so if the heat-map came out slower.  The two launches' TreeStats are compared first.  No gate: a measurement.  --out APPENDS.

    python tools/materials_time.py [--res 1920x1080] [--frames 400] [--reps 7] [--parent-lib PATH] [--out profiles/materials.txt] [--trace N] [--reflections]
                                   [--tiles [--aa] [--commit LABEL]] [--transparency N]
                                   [--tree [--reflections] [--aa] [--tiles]]
                                   [--dynamic [--sheet 180x140]]
                                   [--heat [--reflections] [--aa] [--tiles]]"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from snail_amd import FPSCamera, HostBVH, _lib, scenes  # noqa: E402
from snail_amd import materials as P  # noqa: E402
from snail_amd.scene import Scene, _stream_ptr  # noqa: E402


class ParentScene:
    """snail_scene_create + snail_render_whitted_dev of another build of the library, through raw ctypes (the C-ABI of snail_hip.h)"""

    def __init__(self, path, hb):
        L = C.CDLL(path)
        for name in ("snail_scene_create", "snail_render_whitted_dev", "snail_scene_destroy", "snail_last_error"):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]
        self.L = L
        h = L.snail_scene_create(_lib.ptr(hb.nodes), hb.n_nodes, _lib.ptr(hb.tris), hb.n_tris, hb.depth, 0)
        if not h:
            raise RuntimeError("parent snail_scene_create: %s" % L.snail_last_error().decode())
        self.h = C.c_void_p(h)

    def render_whitted(self, cam13, resx, resy, lights, amb, col, out):
        rc = self.L.snail_render_whitted_dev(self.h, _lib.ptr(cam13), resx, resy, _lib.ptr(lights), len(lights), _lib.ptr(amb), _lib.ptr(col), 0, _lib.ptr(out),
                                             resx * 3, None, _stream_ptr(None))
        if rc:
            raise RuntimeError("parent snail_render_whitted_dev: %s" % self.L.snail_last_error().decode())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", default="1920x1080")
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--detail", type=float, default=scenes.ATRIUM_DETAIL)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--reflections", action="store_true")
    ap.add_argument("--tiles", action="store_true")
    ap.add_argument("--aa", action="store_true")
    ap.add_argument("--commit", default="unlabelled")
    ap.add_argument("--transparency", type=int, default=0, metavar="N")
    ap.add_argument("--tree", action="store_true")
    ap.add_argument("--dynamic", action="store_true")
    ap.add_argument("--heat", action="store_true")
    ap.add_argument("--sheet", default="180x140")
    a = ap.parse_args()
    resx, resy = (int(v) for v in a.res.split("x"))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("materials_time.py measures on the GPU; there is none here")
    from tests import materials_cases as K
    if a.transparency:
        return transparency(a)
    if a.heat:
        return heat(a, resx, resy)
    if a.tree:
        return tree(a, resx, resy)
    if a.dynamic:
        return dynamic(a, resx, resy)

    tv = scenes.atrium(detail=a.detail)
    hb = HostBVH.build(tv)
    sc = Scene(hb, 0)
    pos, ang, pitch = scenes.atrium_camera()
    cam = FPSCamera(pos, ang, pitch).camera()
    cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32)
    lo, hi = hb.bbox()
    lights = np.array([[*(lo + (hi - lo) * np.array([0.5, 0.7, 0.5], dtype=np.float32)), 1.0, 0.9, 0.8, 2.0 * float((hi - lo).max())]], dtype=np.float32)
    amb = np.full(3, 0.1, dtype=np.float32); white = np.ones(3, dtype=np.float32)

    n = len(tv)
    flat_set = P.MaterialSet(sc, np.zeros((n, 3, 2), np.float32), K.plane_normals(hb), np.zeros(n, np.int32), np.ones(n, bool))
    uv, nrm, flat = K.vertex_data(hb, tv, 22)
    descs, mmap = K.materials_mod5()
    mats = [P.Material.simple(d[1], d[2]) if d[0] == "simple" else P.Material.textured(d[1], d[2]) if d[0] == "tex" else P.Material.uber(d[1], d[2], d[3]) for d in descs]
    tex_set = P.MaterialSet(sc, uv, nrm, np.arange(n, dtype=np.int32) % 5, flat, mmap, mats, [P.Texture(t) for t in K.TEXTURES()])
    if a.tiles:
        return tiles(a, sc, cam, resx, resy, lights, tex_set, n)
    if a.reflections:
        return bounce(a, sc, cam, resx, resy, lights, flat_set, tex_set, n)
    parent = ParentScene(a.parent_lib, hb) if a.parent_lib else None

    out = [torch.zeros((resy, resx, 3), dtype=torch.uint8, device="cuda:0") for _ in range(3)]
    variants = {
        "whitted": (lambda: parent.render_whitted(cam13, resx, resy, lights, amb, white, out[0])) if parent else (lambda: sc.render_whitted(cam, resx, resy, lights, out=out[0])),
        "default_flat": lambda: flat_set.render(cam, resx, resy, lights, out=out[1]),
        "textured": lambda: tex_set.render(cam, resx, resy, lights, out=out[2]),
    }
    for fn in variants.values():        # warm-up: code objects, the handles' scratch, the origin-relative node copies
        fn(); fn()
    torch.cuda.synchronize()
    same = bool(torch.equal(out[0], out[1]))
    # the sample stage alone
    pw, ph = (resx + 15) // 16, (resy + 15) // 16
    xy = torch.tensor([(x * 16, y * 16) for y in range(ph) for x in range(pw)], dtype=torch.int32, device="cuda:0")
    hits = sc.trace_packets(cam, resx, resy, xy)
    smp = tex_set.shade_packets(cam, resx, resy, xy, hits)
    variants["sample_stage"] = lambda: tex_set.shade_packets(cam, resx, resy, xy, hits, out=smp)
    torch.cuda.synchronize()
    if a.trace:         # a run under a kernel trace: the launches, nothing else
        for _ in range(a.trace):
            variants["textured"]()
        for _ in range(a.trace):
            variants["sample_stage"]()
        torch.cuda.synchronize()
        print("trace run: %d textured frames, %d sample-stage launches" % (a.trace, a.trace))
        return

    times = {k: [] for k in variants}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.reps):
        for k, fn in variants.items():      # alternating: one window of each per round
            e0.record()
            for _ in range(a.frames):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.frames)
    rays = pw * ph * 256
    lines = ["full shading, %s, %dx%d (%d packets), one light, IEEE; %d rounds of %d frames per variant, alternating; ms per frame: median (min .. max)" %
             ("atrium detail %.2f: %d triangles" % (a.detail, n), resx, resy, pw * ph, a.reps, a.frames),
             "device: %s" % torch.cuda.get_device_name(0),
             "whitted = snail_render_whitted_dev of %s" % ("the build given as --parent-lib" if parent else "THIS build (no --parent-lib given)"),
             "default_flat frame equals the whitted frame byte for byte: %s" % same]
    med = {}
    for k, v in times.items():
        med[k] = statistics.median(v)
        lines.append("  %-13s %8.3f  (%.3f .. %.3f)" % (k, med[k], min(v), max(v)))
    lines.append("default_flat - whitted: %+.3f ms; textured - whitted: %+.3f ms; sample stage, launch to launch: %.3f ms (an upper bound on its kernel time; %.1f GB/s over its 36 B/ray written + 16 B/ray of hit records read)"
                 % (med["default_flat"] - med["whitted"], med["textured"] - med["whitted"], med["sample_stage"], rays * 52 / med["sample_stage"] / 1e6))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    if not same:
        raise SystemExit("default_flat and whitted frames differ")


def bounce(a, sc, cam, resx, resy, lights, flat_set, tex_set, n):
    """--reflections: the bounce under simple and under full shading, and its stages"""
    import torch
    out = [torch.zeros((resy, resx, 3), dtype=torch.uint8, device="cuda:0") for _ in range(3)]
    variants = {
        "whitted_refl": lambda: sc.render_whitted(cam, resx, resy, lights, out=out[0], reflections=True),
        "default_flat_refl": lambda: flat_set.render(cam, resx, resy, lights, out=out[1], reflections=True),
        "textured_refl": lambda: tex_set.render(cam, resx, resy, lights, out=out[2], reflections=True),
    }
    for fn in variants.values():
        fn(); fn()
    torch.cuda.synchronize()
    same = bool(torch.equal(out[0], out[1]))
    if a.trace:
        for _ in range(a.trace):
            variants["textured_refl"]()
        torch.cuda.synchronize()
        print("trace run: %d textured frames with the bounce" % a.trace)
        return
    # the stages with entry points of their own, on the textured set's own intermediates
    pw, ph = (resx + 15) // 16, (resy + 15) // 16
    xy = torch.tensor([(x * 16, y * 16) for y in range(ph) for x in range(pw)], dtype=torch.int32, device="cuda:0")
    hits = sc.trace_packets(cam, resx, resy, xy)
    smp = tex_set.shade_packets(cam, resx, resy, xy, hits)
    org, d, idir, mask, dist, obj = tex_set.mirror_packets(cam, resx, resy, xy, hits[0], smp)
    np_ = pw * ph
    bary = torch.zeros((np_, 64, 8), dtype=torch.float32, device="cuda:0")
    L = _lib.lib()
    cam13 = np.ascontiguousarray(cam.as_array13(), dtype=np.float32)

    def mirror():
        _lib.check(L.snail_materials_mirror_packets_dev(tex_set._h, _lib.ptr(cam13), resx, resy, _lib.ptr(xy), np_, _lib.ptr(hits[0]), _lib.ptr(smp), _lib.ptr(org), _lib.ptr(d),
                                                        _lib.ptr(idir), _lib.ptr(mask), _lib.ptr(dist), _lib.ptr(obj), None, _stream_ptr(None)), "snail_materials_mirror_packets_dev")

    def walk():      # (after the first launch the distances are the hits': every later walk finds nothing nearer -- so the mirror stage runs before each)
        _lib.check(L.snail_trace_rays_dev(sc._h, np_, 64, 0, _lib.ptr(org), _lib.ptr(d), _lib.ptr(idir), _lib.ptr(mask), _lib.ptr(dist), _lib.ptr(obj), _lib.ptr(bary), None,
                                             _stream_ptr(None)), "snail_trace_rays_dev")

    def mirror_and_walk():
        mirror(); walk()
    mirror_and_walk()
    t, tid = dist.reshape(np_, 256).clone(), obj.reshape(np_, 256).clone()
    u, v = bary[:, :, 0:4].reshape(np_, 256).contiguous(), bary[:, :, 4:8].reshape(np_, 256).contiguous()
    nsmp = tex_set.shade_rays(d, mask, t, u, v, tid)
    variants["mirror"] = mirror
    variants["mirror+walk"] = mirror_and_walk
    variants["sample_rays"] = lambda: tex_set.shade_rays(d, mask, t, u, v, tid, out=nsmp)
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.reps):
        for k, fn in variants.items():
            e0.record()
            for _ in range(a.frames):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.frames)
    lines = ["the mirrored bounce (gVals[7]), %s, %dx%d (%d packets), one light, IEEE; %d rounds of %d frames per variant, alternating; ms per frame: median (min .. max)" %
             ("atrium detail %.2f: %d triangles" % (a.detail, n), resx, resy, pw * ph, a.reps, a.frames),
             "device: %s" % torch.cuda.get_device_name(0),
             "whitted_refl = snail_render_whitted_dev with SNAIL_WHITTED_REFLECTIONS of THIS build, in the same run",
             "default_flat_refl frame equals the whitted_refl frame byte for byte: %s" % same,
             "mirrored lanes selected: %d of %d; of them hit: %d" % (int((dist > float("-inf")).sum()), np_ * 256, int(torch.isfinite(t).sum()))]
    med = {}
    for k, v in times.items():
        med[k] = statistics.median(v)
        lines.append("  %-18s %8.3f  (%.3f .. %.3f)" % (k, med[k], min(v), max(v)))
    lines.append("default_flat_refl / whitted_refl: %.3f; textured_refl / whitted_refl: %.3f; mirrored walk alone (mirror+walk - mirror): %.3f ms; the stage figures are launch to launch (upper bounds on kernel times)"
                 % (med["default_flat_refl"] / med["whitted_refl"], med["textured_refl"] / med["whitted_refl"], med["mirror+walk"] - med["mirror"]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    if not same:
        raise SystemExit("default_flat_refl and whitted_refl frames differ")


def tiles(a, sc, cam, resx, resy, lights, tex_set, n):
    """--tiles: the tile list of a full-shaded frame beside the frame call"""
    import time

    import torch
    from snail_amd.render import divide_image
    tl = divide_image(resx, resy)
    out = torch.zeros((resy, resx, 3), dtype=torch.uint8, device="cuda:0")
    size = int((3 * tl[:, 2].astype(np.int64) * tl[:, 3]).sum())
    data = np.zeros(size, dtype=np.uint8)
    flag_sets = [("", 0), ("_refl", P.RENDER_REFLECTIONS)] + ([("_aa", P.RENDER_AA4), ("_aa_refl", P.RENDER_AA4 | P.RENDER_REFLECTIONS)] if a.aa else [])
    frame = {"frame" + k: (lambda f=f: tex_set.render(cam, resx, resy, lights, out=out, reflections=bool(f))) for k, f in flag_sets[:2]}
    tile = {"tiles" + k: (lambda f=f: tex_set.render_tiles_host(cam, resx, resy, tl, lights7=lights, flags=f, data=data)) for k, f in flag_sets}
    for fn in list(frame.values()) + list(tile.values()):      # warm-up: code objects, the set's groups at their largest, the cached tile job
        fn(); fn()
    torch.cuda.synchronize()
    # the planes of the tile call are the frame call's pixels (R, G-R, B-R per tile, src/render.cpp:146-168)
    frame["frame_refl"]()
    torch.cuda.synchronize()
    tile["tiles_refl"]()
    f = out.cpu().numpy()
    want = []
    for x, y, w, h in tl.tolist():
        t = f[y:y + h, x:x + w]
        want += [t[..., 2].reshape(-1), (t[..., 1] - t[..., 2]).reshape(-1), (t[..., 0] - t[..., 2]).reshape(-1)]
    same = bool(np.array_equal(np.concatenate(want), data))
    ev = {k: [] for k in frame}
    wall = {k: [] for k in list(frame) + list(tile)}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.reps):
        for k, fn in frame.items():       # a window enqueued back to back, device events
            e0.record()
            for _ in range(a.frames):
                fn()
            e1.record()
            e1.synchronize()
            ev[k].append(e0.elapsed_time(e1) / a.frames)
        for k, fn in list(frame.items()) + list(tile.items()):       # call by call on the host's clock, a wait after each frame call
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.frames):
                fn()
                if k in frame:
                    torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3 / a.frames)
    pw, ph = (resx + 15) // 16, (resy + 15) // 16
    lines = ["", "full-shaded tile list [%s], %s, %dx%d, %d tiles of 16x64 (%d packets; the frame: %d), one light, IEEE, textured set; %d rounds of %d calls per variant, alternating; ms per call: median (min .. max)" %
             (a.commit, "atrium detail %.2f: %d triangles" % (a.detail, n), resx, resy, len(tl), int(sum(((w + 15) // 16) * ((h + 15) // 16) for _, _, w, h in tl.tolist())), pw * ph, a.reps, a.frames),
             "device: %s" % torch.cuda.get_device_name(0),
             "frame* = snail_render_materials_dev / snail_materials_bounce_dev; tiles* = snail_materials_render_tiles (planar store + ONE device-to-host copy of %d bytes inside the call)" % size,
             "tiles_refl planes equal the planar encoding of the frame_refl frame: %s" % same]
    for k, v in ev.items():
        lines.append("  %-16s %8.3f  (%.3f .. %.3f)   back to back, device events" % (k, statistics.median(v), min(v), max(v)))
    for k, v in wall.items():
        lines.append("  %-16s %8.3f  (%.3f .. %.3f)   call by call, host clock" % (k, statistics.median(v), min(v), max(v)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(text + "\n")
    if not same:
        raise SystemExit("the tile list and the frame differ")


def transparency(a):
    """--transparency N: the panes case with the continuation beside its opaque stand-in"""
    import torch
    from tests import materials_transparency_cases as TK
    c = TK.panes()
    sc = Scene(HostBVH.build(c["tv"]), 0)

    def material(d, opaque):
        if d[0] == "transp":
            return P.Material.textured(d[1], d[3]) if opaque else P.Material.transparent(d[1], d[2], d[3])
        if d[0] == "uber":
            return P.Material.uber(d[1], d[2], 0.0 if opaque and 0.0 < d[3] < 1.0 else d[3])
        return P.Material.simple(d[1], d[2]) if d[0] == "simple" else P.Material.textured(d[1], d[2])
    tex = [P.Texture(t) for t in c["textures"]]
    sets = {op: P.MaterialSet(sc, c["uv"], c["nrm"], c["mat_index"], c["flat"], c["material_map"], [material(d, op) for d in c["descs"]], tex, transparent=True)
            for op in (False, True)}
    assert sets[False].can_select_transparent and not sets[True].can_select_transparent
    lines = ["", "transparency continuation [%s], the tests' panes case (%d triangles), its two lights, IEEE, max_depth %d; %d rounds of %d frames per variant, alternating; ms per frame: median (min .. max)" %
             (a.commit, len(c["tv"]), a.transparency, a.reps, a.frames), "device: %s" % torch.cuda.get_device_name(0),
             "transparent = snail_materials_transparent_dev; opaque = snail_render_materials_dev on the same set rebuilt with opaque stand-ins (TEX for TRANSPARENT, UBER 0 for UBER 0.5)"]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for resx, resy in ((96, 64), (1920, 1080)):
        out = torch.zeros((resy, resx, 3), dtype=torch.uint8, device="cuda:0")
        trunc = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        variants = {"transparent": lambda: sets[False].render_transparent(c["cam"], resx, resy, c["lights"], out=out, max_depth=a.transparency, truncated=trunc),
                    "opaque": lambda: sets[True].render(c["cam"], resx, resy, c["lights"], out=out)}
        for fn in variants.values():
            fn(); fn()
        torch.cuda.synchronize()
        trunc.zero_()
        variants["transparent"]()
        torch.cuda.synchronize()
        cut = int(trunc.item())
        times = {k: [] for k in variants}
        for _ in range(a.reps):
            for k, fn in variants.items():
                e0.record()
                for _ in range(a.frames):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / a.frames)
        for k, v in times.items():
            lines.append("  %4dx%-4d %-12s %8.3f  (%.3f .. %.3f)%s" % (resx, resy, k, statistics.median(v), min(v), max(v), "   truncated lanes per frame: %d" % cut if k == "transparent" else ""))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


def tree(a, resx, resy):
    """--tree: the room case through the tree functions beside the continuation alone and the opaque tile renderer"""
    import time

    import torch
    from snail_amd.render import divide_image
    from tests import materials_tree_cases as K
    c = K.room()
    sc = Scene(HostBVH.build(c["tv"]), 0)

    def material(d, opaque):
        if d[0] == "transp":
            return P.Material.textured(d[1], d[3]) if opaque else P.Material.transparent(d[1], d[2], d[3])
        if d[0] == "uber":
            return P.Material.uber(d[1], d[2], 0.0 if opaque and 0.0 < d[3] < 1.0 else d[3])
        return P.Material.simple(d[1], d[2]) if d[0] == "simple" else P.Material.textured(d[1], d[2])
    tex = [P.Texture(t) for t in c["textures"]]
    sets = {op: P.MaterialSet(sc, c["uv"], c["nrm"], c["mat_index"], c["flat"], c["material_map"], [material(d, op) for d in c["descs"]], tex, transparent=True)
            for op in (False, True)}
    flags = (P.RENDER_REFLECTIONS if a.reflections else 0) | (P.RENDER_AA4 if a.aa else 0)
    tl = divide_image(resx, resy)
    data = np.zeros(int((3 * tl[:, 2].astype(np.int64) * tl[:, 3]).sum()), dtype=np.uint8)
    trunc = np.zeros(1, dtype=np.uint64)
    variants = {
        "tree_tiles" if a.tiles else "tree_frame": (lambda: sets[False].render_tree_tiles_host(c["cam"], resx, resy, tl, lights7=c["lights"], flags=flags, data=data, truncated=trunc))
        if a.tiles else (lambda: sets[False].render_tree_frame_host(c["cam"], resx, resy, c["lights"], flags=flags, truncated=trunc)),
        "transparent_image": lambda: sets[False].render_transparent_image_host(c["cam"], resx, resy, c["lights"], max_depth=8),
        "opaque_tiles": lambda: sets[True].render_tiles_host(c["cam"], resx, resy, tl, lights7=c["lights"], flags=flags, data=data),
    }
    for fn in variants.values():        # warm-up: code objects, the sets' groups at their largest, the cached tile jobs
        fn(); fn()
    torch.cuda.synchronize()
    wall = {k: [] for k in variants}
    for _ in range(a.reps):
        for k, fn in variants.items():
            t0 = time.perf_counter()
            for _ in range(a.frames):
                fn()
            wall[k].append((time.perf_counter() - t0) * 1e3 / a.frames)
    pw, ph = (resx + 15) // 16, (resy + 15) // 16
    one = P.MaterialSet.level_bytes(len(c["lights"]), flags, 8)
    per = max(1, min((1 << 30) // one, pw * ph))
    lines = ["", "the tree [%s]: room case (%d triangles), its two lights, IEEE, %dx%d (%d packets), flags %s%s, max_depth 8; %d rounds of %d calls per variant, alternating, "
             "after 2 warm-up calls each; host clock, ms per call: median (min .. max)" % (a.commit, len(c["tv"]), resx, resy, pw * ph, "REFLECTIONS " if a.reflections else "",
                                                                                            "AA4" if a.aa else "", a.reps, a.frames), "device: %s" % torch.cuda.get_device_name(0),
             "tree_* = snail_materials_tree_render_%s with those flags; transparent_image = snail_materials_transparent_image (flags = 0) on the same set; opaque_tiles = "
             "snail_materials_render_tiles with those flags on the set rebuilt with opaque stand-ins" % ("tiles" if a.tiles else "frame"),
             "levels of one output packet: %d bytes; default budget: %d output packets per slice, %d slice(s); truncated lanes per tree call: %d" % (
                 one, per, -(-(pw * ph) // per), int(trunc[0]) // (a.reps * a.frames + 2))]
    for k, v in wall.items():
        lines.append("  %-18s %9.3f  (%.3f .. %.3f)" % (k, statistics.median(v), min(v), max(v)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


def heat(a, resx, resy):
    """--heat: the heat-map of the room case beside the lit frame it replaces, same arguments"""
    import time

    import torch
    from snail_amd.render import divide_image
    from tests import materials_tree_cases as K
    c = K.room()
    sc = Scene(HostBVH.build(c["tv"]), 0)

    def material(d):
        if d[0] == "transp":
            return P.Material.transparent(d[1], d[2], d[3])
        if d[0] == "uber":
            return P.Material.uber(d[1], d[2], d[3])
        return P.Material.simple(d[1], d[2]) if d[0] == "simple" else P.Material.textured(d[1], d[2])
    ms = P.MaterialSet(sc, c["uv"], c["nrm"], c["mat_index"], c["flat"], c["material_map"], [material(d) for d in c["descs"]], [P.Texture(t) for t in c["textures"]], transparent=True)
    flags = (P.RENDER_REFLECTIONS if a.reflections else 0) | (P.RENDER_AA4 if a.aa else 0)
    pw, ph = (resx + 15) // 16, (resy + 15) // 16
    xy = torch.tensor([(x * 16, y * 16) for y in range(ph) for x in range(pw)], dtype=torch.int32, device="cuda:0")
    out = [torch.zeros((pw * ph, 256, 3), dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    trunc = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    st = [sc.new_stats(), sc.new_stats()]
    tl = divide_image(resx, resy)
    data = np.zeros(int((3 * tl[:, 2].astype(np.int64) * tl[:, 3]).sum()), dtype=np.uint8)
    htrunc = np.zeros(1, dtype=np.uint64)
    if a.tiles:
        variants = {"tree_tiles": lambda s=None: ms.render_tree_tiles_host(c["cam"], resx, resy, tl, lights7=c["lights"], flags=flags, data=data, truncated=htrunc),
                    "heat_tiles": lambda s=None: ms.render_heat_tiles_host(c["cam"], resx, resy, tl, lights7=c["lights"], flags=flags, data=data, truncated=htrunc)}
    else:
        variants = {"tree_packets": lambda s=None: ms.tree_frame_packets(c["cam"], resx, resy, xy, c["lights"], flags=flags, out=out[0], stats=s, truncated=trunc),
                    "heat_packets": lambda s=None: ms.render_heat_packets(c["cam"], resx, resy, xy, c["lights"], flags=flags, out=out[1], stats=s, truncated=trunc)}
    for fn in variants.values():        # warm-up: code objects, every group of the set's intermediates at its largest, the cached tile job
        for _ in range(9):
            fn()
    torch.cuda.synchronize()
    if a.tiles:
        got = [fn()[2] for fn in variants.values()]
    else:
        for fn, s in zip(variants.values(), st):
            fn(s)
        torch.cuda.synchronize()
        got = [s.cpu().numpy() for s in st]
    same = bool(np.array_equal(got[0], got[1]))
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
    lit, hm = list(med)
    ratio = med[hm] / med[lit]
    lines = ["", "the heat-map under full shading [%s]: room case (%d triangles), its two lights, IEEE, %dx%d (%d packets), flags %s%s, max_depth 8; %d rounds of %d calls per "
             "variant, alternating, after 9 warm-up calls each; %s, ms per call: median (min .. max)" % (
                 a.commit, len(c["tv"]), resx, resy, pw * ph, "REFLECTIONS " if a.reflections else "", "AA4" if a.aa else "", a.reps, a.frames,
                 "host clock, call by call (each call ends in its device-to-host copy)" if a.tiles else "device events around a window enqueued back to back"),
             "device: %s" % torch.cuda.get_device_name(0),
             "%s = %s; %s = %s, the same arguments" % ((lit, "snail_materials_tree_render_tiles", hm, "snail_materials_render_heat_tiles") if a.tiles else
                                                      (lit, "snail_materials_tree_frame_packets_dev", hm, "snail_materials_heat_packets_dev")),
             "TreeStats of the two launches equal: %s (%s)" % (same, np.asarray(got[1]).tolist())]
    for k, v in times.items():
        lines.append("  %-14s %9.3f  (%.3f .. %.3f)" % (k, med[k], min(v), max(v)))
    lines.append("  %s / %s: %.3f%s" % (hm, lit, ratio, "   -- the heat-map is SLOWER than the frame it replaces" if ratio > 1.0 else ""))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(text + "\n")
    if not same:
        raise SystemExit("the heat launch's TreeStats differ from the lit frame's")


def dynamic(a, resx, resy):
    """--dynamic: rebuild + frame of a deforming sheet through the dynamic set, beside the route over the host and the build alone"""
    import time

    import torch
    from tests import materials_cases as K
    nu, nv = (int(v) for v in a.sheet.split("x"))
    tvA = K.patch_scene(nu=nu, nv=nv)
    x, y = tvA[..., 0].astype(np.float64), tvA[..., 1].astype(np.float64)
    tvB = tvA.copy()
    tvB[..., 2] = (tvA[..., 2] + 0.22 * np.sin(1.9 * x + 0.4) * np.cos(1.3 * y - 0.2)).astype(np.float32)
    n = len(tvA)
    uv, nrmA, flat = K.vertex_data(HostBVH.build_fast(tvA), tvA, 22)
    nrmB = (nrmA + (np.random.RandomState(31).rand(*nrmA.shape) - 0.5) * 0.5).astype(np.float32)
    mi = np.arange(n, dtype=np.int32) % 5
    descs, mmap = K.materials_mod5()
    mats = [P.Material.simple(d[1], d[2]) if d[0] == "simple" else P.Material.textured(d[1], d[2]) if d[0] == "tex" else P.Material.uber(d[1], d[2], d[3]) for d in descs]
    tex = [P.Texture(t) for t in K.TEXTURES()]
    cam = FPSCamera(np.array([0.0, 0.0, -3.2], dtype=np.float32), 0.0, 0.0).camera()
    lights = np.array([[-0.6, 1.6, -2.6, 1.0, 0.9, 0.8, 14.0]], dtype=np.float32)
    to = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0")      # noqa: E731
    dV, dN, nrm = [to(tvA), to(tvB)], [to(nrmA), to(nrmB)], [nrmA, nrmB]
    fl = np.ascontiguousarray(flat).astype(np.uint8)
    out = [torch.zeros((resy, resx, 3), dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    # one handle per route: each keeps the tree of its own last step
    sc = [Scene.from_fast_dev(dV[0], 0) for _ in range(4)]
    ms = P.MaterialSet.from_dev(sc[0], to(uv), to(mi), to(fl), mmap, mats, tex, d_nrm=dN[0])
    ms_pack = P.MaterialSet.from_dev(sc[3], to(uv), to(mi), to(fl), mmap, mats, tex, d_nrm=dN[0])
    held = {"set": None}

    def dyn_step(k):
        ms.rebuild_dev(dV[k], dN[k])
        ms.render(cam, resx, resy, lights, out=out[0])

    def host_step(k):
        sc[1].rebuild_fast_dev(dV[k])
        torch.cuda.synchronize()
        perm = sc[1].d_perm.cpu().numpy()
        h = P.create_set(sc[1]._h, P.pack_shtris(uv, nrm[k], mi, flat, perm), mmap, mats, tex)
        new = P.MaterialSet.__new__(P.MaterialSet)
        new.scene, new._h, new.shtris = sc[1], h, None
        new.render(cam, resx, resy, lights, out=out[1])
        if held["set"] is not None:
            held["set"].close()
        held["set"] = new

    for k in (1, 0, 1):      # warm-up; both routes end on pose B
        dyn_step(k); host_step(k)
        sc[2].rebuild_fast_dev(dV[k]); ms_pack.update_dev(d_nrm=dN[k])
    torch.cuda.synchronize()
    same = bool(torch.equal(out[0], out[1]))
    colours = len(np.unique(out[0].cpu().numpy().reshape(-1, 3), axis=0))
    ev = {"dynamic": [], "build_alone": [], "repack_alone": []}
    wall = {"host_route": []}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    device_variants = {"dynamic": dyn_step, "build_alone": lambda k: sc[2].rebuild_fast_dev(dV[k]), "repack_alone": lambda k: ms_pack.update_dev(d_nrm=dN[k])}
    for _ in range(a.reps):
        for name, fn in device_variants.items():
            e0.record()
            for f in range(a.frames):
                fn(f & 1)
            e1.record()
            e1.synchronize()
            ev[name].append(e0.elapsed_time(e1) / a.frames)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in range(a.frames):
            host_step(f & 1)
        torch.cuda.synchronize()
        wall["host_route"].append((time.perf_counter() - t0) * 1e3 / a.frames)
    pw, ph = (resx + 15) // 16, (resy + 15) // 16
    lines = ["", "full shading of a deforming mesh [%s]: patch scene %dx%d quads (%d triangles) between two poses, textured set, one light, IEEE, %dx%d (%d packets); "
             "%d rounds of %d steps per variant, alternating, after 3 warm-up steps each; ms per step (one rebuild + one frame): median (min .. max)" %
             (a.commit, nu, nv, n, resx, resy, pw * ph, a.reps, a.frames), "device: %s" % torch.cuda.get_device_name(0),
             "the two routes' frames of pose B are equal byte for byte: %s (%d distinct colours)" % (same, colours)]
    for k, v in ev.items():
        lines.append("  %-13s %9.3f  (%.3f .. %.3f)   device events around the window, no host wait inside" % (k, statistics.median(v), min(v), max(v)))
    for k, v in wall.items():
        lines.append("  %-13s %9.3f  (%.3f .. %.3f)   HOST clock (it contains host work: a wait, the perm's download, the host pack, a new set with its textures)" %
                     (k, statistics.median(v), min(v), max(v)))
    lines.append("  repack_alone moves %d bytes per step (<= 65 read + 64 written per triangle): launch to launch, an upper bound on k_shd_pack's time" % (n * 129))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(text + "\n")
    if not same:
        raise SystemExit("the dynamic set's frame and the host route's differ")


if __name__ == "__main__":
    main()
