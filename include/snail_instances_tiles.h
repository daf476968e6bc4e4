/*
 * snail_instances_tiles.h -- the tile renderer of the two-level instanced scenes of snail_instances.h: RenderTask::Work (src/render.cpp:47-211)
 * around Scene<DBVH>::RayTrace, entirely on the device -- the tile list with its planar store, 4x antialiasing (gVals[9]) and the per-rank
 * tint (gVals[8]).  Part of snail_instances.h, which includes this file last: a host includes snail_instances.h and gets all three.
 *
 * What the reference's render node does every frame (src/node.cpp:326-338, src/rtracer.cpp:359-361: MakeDBVH, then Render(dscene, ...)):
 *   Render(scene, camera, resx, resy, data, coords, offsets, options, rank, threads)   <->  snail_instances_render_tiles
 *   Render(scene, camera, image, options, threads)                                      <->  snail_instances_render_frame
 * Conventions are those of snail_hip.h and snail_instances_shade.h: 0 = success, otherwise snail_last_error() holds the message and nothing
 * was written; lights7 is a HOST pointer to nLights (0..SNAIL_MAX_LIGHTS) x {pos[3], color[3], radius}; d_stats / stats += {intersects,
 * iterations, traced rays, skips}; both arithmetics.
 *
 * flags = SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_DEPTH | SNAIL_RENDER_AA4 (snail_hip.h), any combination:
 *   SNAIL_RENDER_DEPTH        gVals[1]: colour = Inv(t) * (20, 250, 2) in the handle's arithmetic (src/scene_trace.cpp:128-137); lights and
 *                             SNAIL_RENDER_REFLECTIONS are ignored
 *   SNAIL_RENDER_REFLECTIONS  gVals[7]: one mirrored bounce, as SNAIL_WHITTED_REFLECTIONS
 *   SNAIL_RENDER_AA4          gVals[9] (src/render.cpp:60-62, :71-110): every 16x16 packet is the 2x2 reduction of the four packets of the
 *                             (2 resx, 2 resy) frame at (2x + 16 (k & 1), 2y + 16 (k >> 1)), k = 0..3, which run through the same pipeline:
 *                             out = ((a0 + b0) * 0.25) + ((a1 + b1) * 0.25) per channel on the float colours, a = row 2r, b = row 2r + 1.
 *                             The counters are summed over those four packets: traced rays = four times the plain count + secondary rays.
 * tint = const float[3] or NULL: gVals[8] (colorizeNodes, src/render.cpp:118-132): colour = (colour + 0.1) * tint per channel, two separately
 *   rounded operations, after the reduction and before ConvColor; under SNAIL_RENDER_DEPTH too.  The reference takes the factors from a table
 *   of sixteen colours by rank % 16; the library holds no such table (snail::detail::RankTint of snail_adapter.hpp does).  Must be finite.
 * ConvColor: Trunc(Clamp(c * 255, 0, 255)) per channel (src/render.cpp:11-17).
 */
#ifndef SNAIL_INSTANCES_TILES_H
#define SNAIL_INSTANCES_TILES_H
#include "snail_instances.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Any flag combination (and the tint) over an explicit list of packets (int2 pixel origins in device memory): packet-major B,G,R bytes
 * [nPackets][256][3], 4-byte aligned.  With flags in {0, SNAIL_RENDER_REFLECTIONS} and no tint: the bytes and counters of
 * snail_instances_render_whitted_packets_dev.  Intermediates (with SNAIL_RENDER_AA4 those of 4 nPackets packets) come from the handle's
 * eight event-guarded sets, grown as needed; concurrency and the ordering against snail_instances_update are those of the other launches.
 * nPackets <= 0 returns 0. */
int snail_instances_shade_packets_dev(SnailInstances *, const float cam[13], int resx, int resy, const int32_t *d_packet_xy, int nPackets,
                                      const float *lights7, int nLights, const float ambient[3], const float color[3], int flags,
                                      const float *tint, uint8_t *d_bgr_packets, uint64_t *d_stats, void *stream);
/* The tile list.  coords = nTiles x {x, y, w, h}, every rect non-empty with x, y >= 0; every tile is written, 16x64 (the only size the
 * reference stores, src/render.cpp:141-144) or not: its packets run in RenderTask::Work order (16-row bands outer, columns inner; packets are
 * traced whole and counted whole, pixels outside the rect dropped) and its three planes R, G-R, B-R (mod 256; 3 w h bytes,
 * src/render.cpp:146-168) land at data + offsets[k].  The store is clipped to the image as well: what a tile holds beyond resx x resy is
 * zero in all three planes.  Bytes of `data` outside the tiles are not touched.  One call = one pipeline run over all tiles and ONE device-to-host
 * copy.  The device-side packet and tile lists are cached in the handle and rebuilt when (resx, resy, coords) change.  Calls on one handle
 * take turns (one cached list per handle); calls on different handles do not.  nTiles <= 0 returns 0. */
int snail_instances_render_tiles(SnailInstances *, const float cam[13], int resx, int resy, const int32_t *coords, const int64_t *offsets,
                                 int nTiles, const float *lights7, int nLights, const float ambient[3], const float color[3], int flags,
                                 const float *tint, uint8_t *data, uint64_t stats[4]);
/* The image form with SNAIL_RENDER_AA4 accepted: interleaved B,G,R rows of `pitch` bytes in host memory, every pixel inside resx x resy.  No
 * tint: the reference tints tile lists only.  Without SNAIL_RENDER_AA4 exactly snail_instances_render_image. */
int snail_instances_render_frame(SnailInstances *, const float cam[13], int resx, int resy, const float *lights7, int nLights,
                                 const float ambient[3], const float color[3], int flags, uint8_t *image_bgr, int pitch, uint64_t stats[4]);

#ifdef __cplusplus
}
#endif
#endif
