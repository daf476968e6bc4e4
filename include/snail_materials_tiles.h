/*
 * snail_materials_tiles.h -- the tile renderer of full-shaded plain scenes: RenderTask::Work (src/render.cpp:47-211) around the gVals[6]
 * branch of Scene::RayTrace (snail_materials.h) and its mirrored bounce (snail_materials_bounce.h), entirely on the device -- the tile list
 * with its planar store, 4x antialiasing (gVals[9]), depth shading (gVals[1]) and the per-rank tint (gVals[8]).  A header of its own:
 * snail_hip.h, snail_materials.h, snail_materials_bounce.h and their symbol lists stay as they are, and their frame functions keep refusing
 * the flags they refuse.  Plain C.  It mirrors snail_instances_tiles.h function for function.
 *
 * What the reference's render node does every frame with full shading on:
 *   Render(scene, camera, resx, resy, data, coords, offsets, options, rank, threads)   <->  snail_materials_render_tiles
 *   Render(scene, camera, image, options, threads)                                      <->  snail_materials_render_frame
 * Conventions are those of snail_hip.h and snail_materials.h: 0 = success, otherwise snail_last_error() holds the message and nothing was
 * written; lights7 is a HOST pointer to nLights (0..SNAIL_MAX_LIGHTS) x {pos[3], color[3], radius}; d_stats / stats += {intersects,
 * iterations, traced rays, skips}; both arithmetics.  Bad arguments are judged before the handle is looked at, the flags first.
 *
 * flags = SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_DEPTH | SNAIL_RENDER_AA4 (snail_hip.h), any combination; anything else is refused with a
 * text that names `flags`:
 *   SNAIL_RENDER_DEPTH        gVals[1] (src/scene_trace.cpp:128-137) returns before the full-shading branch: colour = Inv(t) * (20, 250, 2) in
 *                             the scene's arithmetic; lights and SNAIL_RENDER_REFLECTIONS are ignored; the counters are the primary walk's alone
 *   SNAIL_RENDER_REFLECTIONS  gVals[7]: the one mirrored bounce of snail_materials_bounce.h, unchanged
 *   SNAIL_RENDER_AA4          gVals[9] (src/render.cpp:60-62, :71-110): every 16x16 packet at (x, y) is the 2x2 reduction of the four packets of
 *                             the (2 resx, 2 resy) frame at (2x + 16 (k & 1), 2y + 16 (k >> 1)), k = 0..3.  Each of the four is a RayTrace call
 *                             of its own through the same pipeline: texture mip selection, the three block branches, the light cull and the
 *                             bounce are those of the double-resolution packets.  out = ((a0 + b0) * 0.25) + ((a1 + b1) * 0.25) per channel on
 *                             the float colours, a = row 2r, b = row 2r + 1.  The counters are summed over the four.
 * tint = const float[3] or NULL (none): gVals[8] (colorizeNodes, src/render.cpp:118-132): colour = (colour + 0.1) * tint per channel, two
 *   separately rounded operations, after the reduction and before ConvColor; under SNAIL_RENDER_DEPTH too.  The library holds no table of rank
 *   colours (snail::detail::RankTint of snail_adapter.hpp does).  Must be finite.
 * ConvColor: Trunc(Clamp(c * 255, 0, 255)) per channel (src/render.cpp:11-17).
 *
 * Equivalences:
 *   flags in {0, SNAIL_RENDER_REFLECTIONS} without tint      the bytes and counters of snail_materials_bounce_packets_dev
 *   SNAIL_RENDER_DEPTH, with or without SNAIL_RENDER_AA4     the bytes and counters of snail_render_tiles on the set's scene with the same flags
 *
 * NOT here (the host renderer keeps them): tiles, 4x antialiasing and the tint with the transparency continuation (the transparent kinds and
 * the continuation's plain frames are snail_materials_transparency.h's; a set that can select a transparent lane is refused by the functions here);
 * full-shaded tiles dealt over several devices; the ordered launches (dispatch-order feedback); materials on instanced scenes.  The heat-map
 * (gVals[5]) under full shading is snail_materials_heatmap.h's.
 */
#ifndef SNAIL_MATERIALS_TILES_H
#define SNAIL_MATERIALS_TILES_H
#include "snail_materials_bounce.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Any flag combination (and the tint) over an explicit list of packets (int2 pixel origins in device memory): packet-major B,G,R bytes
 * [nPackets][256][3], 4-byte aligned.  Intermediates (with SNAIL_RENDER_AA4 those of 4 nPackets packets) come from the set's eight
 * event-guarded groups, grown as needed; launches are booked under the scene's lock like every other launch on it.  nPackets <= 0 returns 0. */
int snail_materials_frame_packets_dev(SnailMaterials *, const float cam[13], int resx, int resy, const int32_t *d_packet_xy, int nPackets,
                                      const float *lights7, int nLights, const float ambient[3], int flags, const float *tint,
                                      uint8_t *d_bgr_packets, uint64_t *d_stats, void *stream);
/* The tile list.  coords = nTiles x {x, y, w, h}, every rect non-empty with x, y >= 0; every tile is written, 16x64 (the only size the
 * reference stores, src/render.cpp:141-144) or not: its packets run in RenderTask::Work order (16-row bands outer, columns inner; packets are
 * traced whole and counted whole, pixels outside the rect dropped) and its three planes R, G-R, B-R (mod 256; 3 w h bytes,
 * src/render.cpp:146-168) land at data + offsets[k].  The store is clipped to the image as well: what a tile holds beyond resx x resy is zero
 * in all three planes.  Bytes of `data` outside the tiles are not touched.  One call = one pipeline run over all tiles and ONE device-to-host
 * copy.  The device-side packet and tile lists are cached in the set and rebuilt when (resx, resy, coords) change.  Calls on one set take
 * turns (one cached list per set); calls on different sets do not.  nTiles <= 0 returns 0. */
int snail_materials_render_tiles(SnailMaterials *, const float cam[13], int resx, int resy, const int32_t *coords, const int64_t *offsets,
                                 int nTiles, const float *lights7, int nLights, const float ambient[3], int flags, const float *tint,
                                 uint8_t *data, uint64_t stats[4]);
/* The image form: interleaved B,G,R rows of `pitch` bytes in host memory, every pixel inside resx x resy.  No tint: the reference tints tile
 * lists only.  With flags in {0, SNAIL_RENDER_REFLECTIONS} exactly snail_materials_bounce_image. */
int snail_materials_render_frame(SnailMaterials *, const float cam[13], int resx, int resy, const float *lights7, int nLights,
                                 const float ambient[3], int flags, uint8_t *image_bgr, int pitch, uint64_t stats[4]);

#ifdef __cplusplus
}
#endif
#endif
