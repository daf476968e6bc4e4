/*
 * snail_instances_materials_heatmap.h -- per-packet TreeStats and the "scene complexity visualization" (gVals[5]) of INSTANCED scenes under FULL
 * shading (gVals[6] with DBVH::HasShadingData() answering 1), on the device: what snail_materials_heatmap.h is for a plain scene, function
 * for function, on the tree of snail_instances_materials_tree.h.  A header of its own: snail_heatmap.h counts the simple-shading pipeline of an
 * instanced scene (snail_instances_*), and under full shading the counters differ -- the shadow lanes follow the interpolated, rotated normals,
 * and the transparency continuation and the bounce nest further RayTrace calls.  snail_instances_materials_tree.h, snail_heatmap.h and their
 * symbol lists stay as they are.  Plain C.  The functions here take ANY set of snail_instances_materials_create /
 * snail_instances_materials_create_transparent.
 *
 * What is counted is written in snail_materials_heatmap.h (src/scene_trace.cpp): one TreeStats per RayTrace call -- TracingRays of its mask
 * bits, its TraversePrimary, the WHOLE TreeStats of TraceReflection and of TraceTransparency, recursively, and TraceLight for every light that
 * is not culled at packet level -- and with gVals[5] a PRIMARY call overwrites every ray's colour with StatsShader(stats, 64).  Here the walks
 * are DBVH::TraversePrimary and DBVH::TraverseShadow: a counter word holds the top-level tree's and the instances' trees' work added together,
 * as d_stats does.  Nothing a counter depends on reads a colour -- the selectors come from the sample stage's opacity, the lights from position
 * and normal -- so the functions run every sample, generator, mirror, walk, truncation and light stage of the tree and leave out the blends
 * and the colour stages.  There is no `ambient` parameter: it reaches no counter.  A packet none of whose rays hits anything still books its
 * 256 rays and the walk that found nothing.
 *
 * Four words per packet in the order of d_stats: {intersects, iterations, rays, skips}, uint32_t.
 *
 * Conventions are those of snail_instances_materials_tree.h: 0 = success, otherwise snail_last_error() holds the message and nothing is
 * written; arguments are judged before the handle is looked at, the flags first; lights7 is a HOST pointer to nLights (0..SNAIL_MAX_LIGHTS) x
 * {pos[3], color[3], radius}; both arithmetics; thread-safe per handle; the _dev forms are asynchronous on `stream`.  maxDepth is 1..8 and the
 * truncated counter is required: whenever it does not move, the counters are the reference's.  Launches are ordered against
 * snail_instances_update / snail_instances_rebuild_dev as the handle's frames are; the instance records are read at launch.
 *
 * flags: SNAIL_RENDER_REFLECTIONS (gVals[7]) and, where stated, SNAIL_RENDER_AA4 (gVals[9]: each of the four double-resolution sub-packets is
 * a RayTrace call with a tree and a heat colour of its own; the 8x8 quadrant rule is snail_heatmap.h's).  SNAIL_RENDER_DEPTH is refused as in
 * snail_heatmap.h: gVals[1] returns from RayTrace before any of this, depth shading has no heat-map.  Any other bit is refused too, with a
 * text that names `flags`.
 *
 * Memory: the levels' intermediates stay within the set's level budget (snail_instances_materials_set_level_budget); the packet list runs in
 * slices, each of which books at its packets' place in the whole list's counters.  Slicing changes no counter and no byte.
 *
 * NOT here (the host renderer keeps them): full-shaded tiles dealt over several devices; the ordered launches (dispatch-order feedback) under
 * full shading; routing in snail_adapter.hpp (no reference host can reach this branch through HipDBVH); creating sets for BLASes whose tree is
 * rebuilt on the device (snail_instances_materials_dynamic.h has that; its sets are taken here).
 */
#ifndef SNAIL_INSTANCES_MATERIALS_HEATMAP_H
#define SNAIL_INSTANCES_MATERIALS_HEATMAP_H
#include "snail_instances_materials_tree.h"
#include "snail_heatmap.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The TreeStats of every packet's RayTrace call; no image.  d_packet_xy = explicit device packet list (nPackets pairs x, y; a packet may be
 * listed more than once, and may lie outside the frame), or NULL = the frame's own grid: packet cy * pw + cx, pw = ceil(resx / 16), and
 * nPackets is ignored.  d_packet_stats = uint32_t [packets][4] (4-byte aligned device memory, overwritten); d_stats (optional) += their sum;
 * *d_truncated (a DEVICE word) += the lanes level maxDepth would still select.  flags: SNAIL_RENDER_REFLECTIONS only. */
int snail_instances_materials_packet_stats_dev(SnailInstancesMaterials *, const float cam[13], int resx, int resy, const int32_t *d_packet_xy,
                                               int nPackets, const float *lights7, int nLights, int flags, int maxDepth,
                                               uint32_t *d_packet_stats, uint64_t *d_truncated, uint64_t *d_stats, void *stream);

/* The heat-map of the same packets: packet-major B,G,R bytes [packets][256][3] (4-byte aligned).  flags may hold SNAIL_RENDER_AA4.
 * tint (optional, three factors, gVals[8]): c = (c + 0.1) * tint after the heat colour and the antialiasing reduction, before ConvColor, as
 * in snail_instances_tiles.h.  d_packet_stats (optional): the counters the colours were made from, [packets][4] -- with SNAIL_RENDER_AA4 the
 * four sub-packets' counters, [packets][4][4], sub-packet k of a packet at (2x + 16 (k & 1), 2y + 16 (k >> 1)). */
int snail_instances_materials_heat_packets_dev(SnailInstancesMaterials *, const float cam[13], int resx, int resy, const int32_t *d_packet_xy,
                                               int nPackets, const float *lights7, int nLights, int flags, const float *tint,
                                               uint8_t *d_bgr_packets, uint32_t *d_packet_stats, int maxDepth, uint64_t *d_truncated,
                                               uint64_t *d_stats, void *stream);

/* snail_instances_materials_tree_render_tiles with gVals[5]: the host-pointer tile list, planes R, G-R, B-R at data + offsets[k]; *truncated
 * is a HOST word (+=), stats[4] (optional) += the call's counters.  flags may hold SNAIL_RENDER_AA4.  The set's one cached tile job: calls
 * on one set take turns with snail_instances_materials_tree_render_tiles. */
int snail_instances_materials_render_heat_tiles(SnailInstancesMaterials *, const float cam[13], int resx, int resy, const int32_t *coords,
                                                const int64_t *offsets, int nTiles, const float *lights7, int nLights, int flags,
                                                const float *tint, uint8_t *data, int maxDepth, uint64_t *truncated, uint64_t stats[4]);

/* snail_instances_materials_tree_render_frame with gVals[5]: interleaved B,G,R into a host image of `pitch` >= 3 * resx bytes per row (bytes
 * between rows are left alone).  flags may hold SNAIL_RENDER_AA4. */
int snail_instances_materials_render_heat_frame(SnailInstancesMaterials *, const float cam[13], int resx, int resy, const float *lights7,
                                                int nLights, int flags, uint8_t *image_bgr, int pitch, int maxDepth, uint64_t *truncated,
                                                uint64_t stats[4]);

#ifdef __cplusplus
}
#endif
#endif
