/* snail_heatmap.h -- per-packet TreeStats and the reference's "scene complexity visualization" (gVals[5]) on the device.
 *
 * The reference's Scene::RayTrace keeps a TreeStats of its own for the 16x16 packet it shades (src/scene_trace.cpp:102-120, :454-466,
 * :494-502): TracingRays of the packet's mask bits (256 for a primary packet, at the image edge too), the counters of TraversePrimary,
 * with gVals[7] the whole TreeStats of TraceReflection (the nested RayTrace of the mirrored packet: its rays, its walk, its own
 * lights), and the TreeStats of TraceLight for every light that is not culled at packet level (the shadow lanes with N.L > 0 plus
 * TraverseShadow).  With gVals[5] a primary call then gives EVERY ray of the packet -- hits and misses alike, with or without
 * lights -- one colour made from those counters (:62-76, :513-517; size = 64 quads):
 *     (r, g, b) = (float(intersects) * (0.002f / size), float(iterations) * (0.02f / size), float(skips * 0.25f))
 * followed by ConvColor (B,G,R bytes).  The nested call of a mirrored packet contributes counters, never a colour.
 *
 * The functions below run the staged pipeline of snail_render_whitted_dev -- every walk of the lit frame -- and keep what the other
 * entry points sum away: the counters per packet, as an output of their own (where in the image does the tree cost what) and as the
 * heat-map.  Four words per packet in the order of d_stats: {intersects, iterations, rays, skips}, uint32_t.
 *
 * flags: SNAIL_RENDER_REFLECTIONS (gVals[7]) and, where stated, SNAIL_RENDER_AA4 (gVals[9]: each of the four double-resolution
 * packets of a packet is a RayTrace call with a heat colour of its own; the 8x8 quadrant (k & 1, k >> 1) of the packet is the 2x2
 * reduction of sub-packet k's colour, src/render.cpp:71-110).  SNAIL_RENDER_DEPTH is refused: gVals[1] returns from RayTrace before
 * any of this (src/scene_trace.cpp:128-137) -- depth shading has no heat-map in the reference; render it with the depth entry points.
 * Any other bit is refused as well.
 *
 * Conventions are those of snail_hip.h: 0 = success, otherwise snail_last_error() holds the message and nothing is written; lights7 is
 * a host pointer (at most SNAIL_MAX_LIGHTS lights; position, colour, radius -- the colour does not matter here, position and radius
 * decide which shadow packets are walked); both arithmetics; thread-safe per handle; the _dev forms are asynchronous on `stream` and
 * take their intermediates from the handle's event-guarded scratch sets, so launches in flight on different streams share nothing. */
#ifndef SNAIL_HEATMAP_H
#define SNAIL_HEATMAP_H

#include "snail_hip.h"
#include "snail_instances.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The TreeStats of every packet's RayTrace call; no image.  d_packet_xy = explicit device packet list (n_packets pairs x, y; a packet
 * may be listed more than once), or NULL = the frame's own grid: packet cy * pw + cx, pw = ceil(resx / 16), and n_packets is ignored.
 * d_packet_stats = uint32_t [packets][4] (4-byte aligned device memory, overwritten); d_stats (optional) += their sum. */
int snail_packet_stats_dev(SnailScene *, const float cam[13], int resx, int resy, const int32_t *d_packet_xy, int n_packets,
                           const float *lights7, int n_lights, int flags, uint32_t *d_packet_stats, uint64_t *d_stats, void *stream);

/* The heat-map of the same packets: packet-major B,G,R bytes [packets][256][3] (4-byte aligned; scatter with
 * snail_packets_bgr_to_frame_dev or snail_packets_bgr_to_planar_dev).  flags may hold SNAIL_RENDER_AA4.  d_packet_stats (optional):
 * the counters the colours were made from, [packets][4] -- with SNAIL_RENDER_AA4 the four sub-packets' counters, [packets][4][4]. */
int snail_render_heat_packets_dev(SnailScene *, const float cam[13], int resx, int resy, const int32_t *d_packet_xy, int n_packets,
                                  const float *lights7, int n_lights, int flags, uint8_t *d_bgr_packets, uint32_t *d_packet_stats,
                                  uint64_t *d_stats, void *stream);

/* snail_render_tiles with gVals[5]: the host-pointer tile list, planes R, G-R, B-R at data + offsets[k]; same tile rules, same cached
 * lists, stats[4] (optional) += the call's counters.  flags may hold SNAIL_RENDER_AA4. */
int snail_render_heat_tiles(SnailScene *, const float cam[13], int resx, int resy, const int32_t *coords, const int64_t *offsets, int nTiles,
                            const float *lights7, int n_lights, int flags, uint8_t *data, uint64_t stats[4]);

/* snail_render_image with gVals[5]: interleaved B,G,R into a host image of `pitch` >= 3 * resx bytes per row (bytes between rows are
 * left alone).  flags may hold SNAIL_RENDER_AA4. */
int snail_render_heat_image(SnailScene *, const float cam[13], int resx, int resy, const float *lights7, int n_lights, int flags,
                            uint8_t *image_bgr, int pitch, uint64_t stats[4]);

/* ---- instanced scenes (SnailInstances, include/snail_instances.h): the same four, over Scene<DBVH>::RayTrace ----------------------------- */
/* The counters include the top-level walk's (one loop iteration per top-level node, Intersection per instance leaf), as d_stats of
 * snail_instances_render_whitted_dev does; their sum over the packets IS that d_stats.  `tint` (optional, 3 floats) is the rank tint of
 * gVals[8] as in snail_instances_shade_packets_dev: c = (c + 0.1) * tint after the heat colour (and after the antialiasing reduction),
 * before ConvColor (src/render.cpp:118-132). */
int snail_instances_packet_stats_dev(SnailInstances *, const float cam[13], int resx, int resy, const int32_t *d_packet_xy, int n_packets,
                                     const float *lights7, int n_lights, int flags, uint32_t *d_packet_stats, uint64_t *d_stats,
                                     void *stream);
int snail_instances_heat_packets_dev(SnailInstances *, const float cam[13], int resx, int resy, const int32_t *d_packet_xy, int n_packets,
                                     const float *lights7, int n_lights, int flags, const float *tint, uint8_t *d_bgr_packets,
                                     uint32_t *d_packet_stats, uint64_t *d_stats, void *stream);
int snail_instances_render_heat_tiles(SnailInstances *, const float cam[13], int resx, int resy, const int32_t *coords, const int64_t *offsets,
                                      int nTiles, const float *lights7, int n_lights, int flags, const float *tint, uint8_t *data,
                                      uint64_t stats[4]);
int snail_instances_render_heat_frame(SnailInstances *, const float cam[13], int resx, int resy, const float *lights7, int n_lights, int flags,
                                      uint8_t *image_bgr, int pitch, uint64_t stats[4]);

#ifdef __cplusplus
}
#endif
#endif
