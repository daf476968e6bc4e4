/*
 * snail_materials_tree.h -- the transparency continuation of full-shaded plain scenes TOGETHER with the one mirrored bounce (gVals[7]), the
 * tile renderer, 4x antialiasing (gVals[9]), depth shading (gVals[1]) and the tint (gVals[8]), entirely on the device.  A header of its own:
 * snail_materials.h, snail_materials_bounce.h, snail_materials_tiles.h, snail_materials_transparency.h and their symbol lists stay as they
 * are, and their functions keep refusing what they refuse (every nonzero flag with the continuation; a set that can select a transparent lane
 * everywhere else).  Plain C.  The functions here take ANY set of snail_materials_create / snail_materials_create_transparent.
 *
 * The calls the reference nests with gVals[6] and gVals[7] (src/scene_trace.cpp:454-483, :603-634):
 *   RayTrace with cache.reflections == 0 calls TraceReflection = RayTrace with cache.reflections == 1 on the mirrored rays of its hit lanes and
 *     blends diffuse += (refl - diffuse) * 0.3 there; THEN calls TraceTransparency = RayTrace with cache.reflections == 0 again on the lanes its
 *     selector holds and blends VLerp(transColor, diffuse, opacity) there; then runs its lights.
 *   RayTrace with cache.reflections == 1 never mirrors; it does continue through its transparent lanes, still with reflections == 1.
 * With the depth cut of snail_materials_transparency.h (maxDepth D = 1..8, counted in continuations on the path from the primary packet; a
 * lane that level D would still select is counted in the truncated-lane counter and treated as not selected) the calls form a triangle:
 *   chain A   levels A_0 (the primary packets) .. A_D, reflections == 0
 *   chain B   every A_k starts one: the mirrored call B_{k,k} and its continuations B_{k,k+1} .. B_{k,D}, reflections == 1 (B_{D,D} takes
 *             place too, and is cut at once)
 * (D + 1) + (D + 1)(D + 2) / 2 RayTrace bodies, 54 at D = 8.  A packet of A_k none of whose lanes hit is still mirrored (reflSel.Any() is
 * commented out, :454), and its walk is counted.  Counter 0 after the call <=> the frame and the TreeStats are the reference's.
 *
 * Conventions are those of snail_hip.h and snail_materials_tiles.h: 0 = success, otherwise snail_last_error() holds the message and nothing
 * was written; lights7 is a HOST pointer to nLights (0..SNAIL_MAX_LIGHTS) x {pos[3], color[3], radius}; d_stats / stats += {intersects,
 * iterations, traced rays, skips}; both arithmetics.  Bad arguments are judged before the handle is looked at, the flags first.
 *
 * flags = SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_DEPTH | SNAIL_RENDER_AA4 in any combination, with the meanings of snail_materials_tiles.h;
 * anything else is refused with a text that names `flags`.  SNAIL_RENDER_DEPTH returns before full shading, as there (no level runs, the
 * counter does not move).  Under SNAIL_RENDER_AA4 each of the four double-resolution RayTrace calls has its own tree.  tint, ConvColor and the
 * planar store are snail_materials_tiles.h's.
 *
 * Equivalences (bytes, TreeStats and the counter; counter 0 where the older function has none):
 *   (a) flags = 0, no tint                               snail_materials_transparent_packets_dev at the same maxDepth
 *   (b) a set that cannot select a transparent lane      snail_materials_frame_packets_dev / snail_materials_render_tiles /
 *                                                        snail_materials_render_frame with the same flags and tint, at every maxDepth
 *   (c) SNAIL_RENDER_DEPTH                               snail_render_tiles on the set's scene with the same flags
 *
 * Memory.  The levels' intermediates (D A-levels and, with the bounce, D + 1 B-levels reused by every chain; 4 nPackets packets each under
 * SNAIL_RENDER_AA4) are bounded per group of intermediates: the packet list runs in slices of whole output packets, back to back on the same
 * stream and arena, sized so that the levels stay within the set's level budget.  Packets are independent: slicing changes no byte and no counter.
 *
 * NOT here (the host renderer keeps them): full-shaded tiles dealt over several devices; the ordered launches (dispatch-order feedback) under
 * full shading (the heat-map, gVals[5], of these frames is snail_materials_heatmap.h); materials on instanced scenes (the reference's DBVH::HasShadingData() returns 0); maxDepth
 * above 8 (the reference has no cut: a frame whose counter moved is not the reference's).
 */
#ifndef SNAIL_MATERIALS_TREE_H
#define SNAIL_MATERIALS_TREE_H
#include "snail_materials_transparency.h"
#include "snail_materials_tiles.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Scene::TraceReflection from a level's GENERIC packets (snail_materials_mirror_packets_dev reads the primary ones): d_origin_in / d_dir_in
 * [n][64][3][4], d_mask_in [n][64] (NULL: every lane selected), d_t [n][256] and the level's samples d_samples [n][9][64][4] -> the mirrored
 * packets in the layouts of snail_materials_mirror_packets_dev, selector = mask bit set and t < inf, + d_order [n].  d_order_in (or NULL: every
 * packet) is the level's own order list: for a packet whose word is negative d_order gets -1 and NOTHING else is written; every other packet
 * gets its index, whether or not a lane of it hit.  *d_stats (or NULL) += the nested call's TracingRays.  Float buffers 16-byte aligned. */
int snail_materials_mirror_rays_dev(SnailMaterials *, int nPackets, const float *d_origin_in, const float *d_dir_in, const uint8_t *d_mask_in,
                                    const float *d_t, const float *d_samples, const int32_t *d_order_in, float *d_origin, float *d_dir,
                                    float *d_idir, uint8_t *d_mask, float *d_distance, int32_t *d_object, int32_t *d_order, uint64_t *d_stats,
                                    void *stream);

/* snail_materials_frame_packets_dev for any set: + maxDepth (1..8) and *d_truncated (a DEVICE word, +=), before the stats. */
int snail_materials_tree_frame_packets_dev(SnailMaterials *, const float cam[13], int resx, int resy, const int32_t *d_packet_xy, int nPackets,
                                           const float *lights7, int nLights, const float ambient[3], int flags, const float *tint,
                                           uint8_t *d_bgr_packets, int maxDepth, uint64_t *d_truncated, uint64_t *d_stats, void *stream);
/* snail_materials_render_tiles for any set: + maxDepth and *truncated (a HOST word, +=), before the stats. */
int snail_materials_tree_render_tiles(SnailMaterials *, const float cam[13], int resx, int resy, const int32_t *coords, const int64_t *offsets,
                                      int nTiles, const float *lights7, int nLights, const float ambient[3], int flags, const float *tint,
                                      uint8_t *data, int maxDepth, uint64_t *truncated, uint64_t stats[4]);
/* snail_materials_render_frame for any set: + maxDepth and *truncated (a HOST word, +=), before the stats. */
int snail_materials_tree_render_frame(SnailMaterials *, const float cam[13], int resx, int resy, const float *lights7, int nLights,
                                      const float ambient[3], int flags, uint8_t *image_bgr, int pitch, int maxDepth, uint64_t *truncated,
                                      uint64_t stats[4]);

/* The level budget of the set's groups of intermediates, in bytes (the default: SNAIL_MAT_LEVEL_BUDGET).  A call clamps it up to what ONE
 * output packet needs, snail_materials_level_bytes(nLights, flags, maxDepth): the bytes of the levels of one output packet (4 double-resolution
 * packets under SNAIL_RENDER_AA4; D A-levels, + D + 1 B-levels with SNAIL_RENDER_REFLECTIONS; 0 under SNAIL_RENDER_DEPTH), or -1 for arguments
 * the frame functions would refuse. */
int snail_materials_set_level_budget(SnailMaterials *, uint64_t bytes);
int64_t snail_materials_level_bytes(int nLights, int flags, int maxDepth);
/* 1 GiB: at 8 lights and maxDepth 8 with the bounce and antialiasing one output packet (4 double-resolution packets) takes (8 + 9) levels
 * x 136.75 KiB + 4.5 KiB = 2 329.25 KiB, so a slice is 450 output packets and a 1920 x 1080 frame (8 160 packets, 18.1 GiB unsliced) runs
 * in 19 slices. */
#define SNAIL_MAT_LEVEL_BUDGET (1ull << 30)

#ifdef __cplusplus
}
#endif
#endif
