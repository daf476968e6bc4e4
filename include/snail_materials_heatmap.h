/*
 * snail_materials_heatmap.h -- per-packet TreeStats and the "scene complexity visualization" (gVals[5]) of plain scenes under FULL shading
 * (gVals[6] on a scene with shading data), on the device.  A header of its own: snail_heatmap.h counts the simple-shading pipeline, and under
 * full shading the counters differ -- the shadow lanes follow the interpolated normals, and the transparency continuation and the bounce nest
 * further RayTrace calls.  snail_materials_tree.h, snail_heatmap.h and their symbol lists stay as they are.  Plain C.  The functions here take
 * ANY set of snail_materials_create / snail_materials_create_transparent / snail_materials_create_dev (rebuilt or not).
 *
 * What is counted (src/scene_trace.cpp).  Scene::RayTrace keeps one TreeStats per call and adds into it: TracingRays of its mask bits (:116-117),
 * its TraversePrimary (:120), the WHOLE TreeStats of TraceReflection (:459) and of TraceTransparency (:476) -- the nested RayTrace calls,
 * recursively -- and TraceLight for every light that is not culled at packet level (:496-502).  With gVals[5] a PRIMARY call then overwrites
 * every ray's colour with StatsShader(stats, size) (:62-76, :513-517):
 *     (r, g, b) = (float(intersects) * (0.002f / size), float(iterations) * (0.02f / size), float(skips * 0.25f)),   size = 64 quads
 * The nested calls are RayGroup<0, 0> or RayGroup<0, 1> (:615-617, :631-633): their flags are 0, they contribute counters and never a colour.
 * Nothing a counter depends on reads a colour -- the selectors come from the sample stage's opacity, the lights from position and normal -- so
 * the functions run every sample, generator, mirror, walk, truncation and light stage of the tree of snail_materials_tree.h (up to 54 RayTrace
 * bodies per packet at maxDepth 8) and leave out the blends and the colour stages.  There is no `ambient` parameter: it reaches no counter.
 *
 * Four words per packet in the order of d_stats: {intersects, iterations, rays, skips}, uint32_t.
 *
 * Conventions are those of snail_materials_tree.h: 0 = success, otherwise snail_last_error() holds the message and nothing is written;
 * arguments are judged before the handle is looked at, the flags first; lights7 is a HOST pointer to nLights (0..SNAIL_MAX_LIGHTS) x {pos[3],
 * color[3], radius}; both arithmetics; thread-safe per handle; the _dev forms are asynchronous on `stream`.  maxDepth is 1..8 and the truncated
 * counter is required: whenever it does not move, the counters are the reference's.  A stale set (the tree was rebuilt and the records did
 * not follow) is refused as the frame functions refuse it.
 *
 * flags: SNAIL_RENDER_REFLECTIONS (gVals[7]) and, where stated, SNAIL_RENDER_AA4 (gVals[9]: each of the four double-resolution sub-packets is
 * a RayTrace call with a tree and a heat colour of its own; the 8x8 quadrant rule is snail_heatmap.h's).  SNAIL_RENDER_DEPTH is refused as in
 * snail_heatmap.h: gVals[1] returns from RayTrace before any of this (:128-137), depth shading has no heat-map.  Any other bit is refused too,
 * with a text that names `flags`.
 *
 * Memory: the levels' intermediates stay within the set's level budget (snail_materials_set_level_budget); the packet list runs in slices, each
 * of which books at its packets' place in the whole list's counters.  Slicing changes no counter and no byte.
 *
 * NOT here (the host renderer keeps them): full-shaded tiles dealt over several devices; the ordered launches (dispatch-order feedback) under
 * full shading.
 */
#ifndef SNAIL_MATERIALS_HEATMAP_H
#define SNAIL_MATERIALS_HEATMAP_H
#include "snail_materials_tree.h"
#include "snail_heatmap.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The TreeStats of every packet's RayTrace call; no image.  d_packet_xy = explicit device packet list (nPackets pairs x, y; a packet may be
 * listed more than once), or NULL = the frame's own grid: packet cy * pw + cx, pw = ceil(resx / 16), and nPackets is ignored.
 * d_packet_stats = uint32_t [packets][4] (4-byte aligned device memory, overwritten); d_stats (optional) += their sum; *d_truncated (a DEVICE
 * word) += the lanes level maxDepth would still select.  flags: SNAIL_RENDER_REFLECTIONS only. */
int snail_materials_packet_stats_dev(SnailMaterials *, const float cam[13], int resx, int resy, const int32_t *d_packet_xy, int nPackets,
                                     const float *lights7, int nLights, int flags, int maxDepth, uint32_t *d_packet_stats,
                                     uint64_t *d_truncated, uint64_t *d_stats, void *stream);

/* The heat-map of the same packets: packet-major B,G,R bytes [packets][256][3] (4-byte aligned).  flags may hold SNAIL_RENDER_AA4.
 * tint (optional, three factors, gVals[8]): c = (c + 0.1) * tint after the heat colour and the antialiasing reduction, before ConvColor, as
 * for instanced scenes.  d_packet_stats (optional): the counters the colours were made from, [packets][4] -- with SNAIL_RENDER_AA4 the four
 * sub-packets' counters, [packets][4][4], sub-packet k of a packet at (2x + 16 (k & 1), 2y + 16 (k >> 1)). */
int snail_materials_heat_packets_dev(SnailMaterials *, const float cam[13], int resx, int resy, const int32_t *d_packet_xy, int nPackets,
                                     const float *lights7, int nLights, int flags, const float *tint, uint8_t *d_bgr_packets,
                                     uint32_t *d_packet_stats, int maxDepth, uint64_t *d_truncated, uint64_t *d_stats, void *stream);

/* snail_materials_tree_render_tiles with gVals[5]: the host-pointer tile list, planes R, G-R, B-R at data + offsets[k]; *truncated is a HOST
 * word (+=), stats[4] (optional) += the call's counters.  flags may hold SNAIL_RENDER_AA4. */
int snail_materials_render_heat_tiles(SnailMaterials *, const float cam[13], int resx, int resy, const int32_t *coords, const int64_t *offsets,
                                      int nTiles, const float *lights7, int nLights, int flags, const float *tint, uint8_t *data, int maxDepth,
                                      uint64_t *truncated, uint64_t stats[4]);

/* snail_materials_tree_render_frame with gVals[5]: interleaved B,G,R into a host image of `pitch` >= 3 * resx bytes per row (bytes between
 * rows are left alone).  flags may hold SNAIL_RENDER_AA4. */
int snail_materials_render_heat_frame(SnailMaterials *, const float cam[13], int resx, int resy, const float *lights7, int nLights, int flags,
                                      uint8_t *image_bgr, int pitch, int maxDepth, uint64_t *truncated, uint64_t stats[4]);

#ifdef __cplusplus
}
#endif
#endif
