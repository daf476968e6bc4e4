/*
 * snail_instances_materials_tree.h -- the transparency continuation of full-shaded INSTANCED scenes TOGETHER with the one mirrored bounce
 * (gVals[7]), the tile renderer, 4x antialiasing (gVals[9]), depth shading (gVals[1]) and the tint (gVals[8]), entirely on the device: what
 * snail_materials_tree.h is for a plain scene, function for function, with the DBVH walk on per-ray origins, the (slot, triId) keys, GetSElement
 * through ShTriangle::Transform and DBVH::TraverseShadow of snail_instances_materials.h.  A header of its own: snail_instances_materials.h,
 * snail_instances_materials_bounce.h, snail_instances_materials_transparency.h and their symbol lists stay as they are, and their functions
 * keep refusing what they refuse (every nonzero flag with the continuation; a set that can select a transparent lane with the bounce).
 * Plain C.  The functions here take ANY set of snail_instances_materials_create / snail_instances_materials_create_transparent.
 *
 * Semantics are those written in snail_materials_tree.h: the triangle of calls (chain A, levels A_0 .. A_D with cache.reflections == 0; every
 * A_k starts a chain B, the mirrored call B_{k,k} and its continuations B_{k,k+1} .. B_{k,D} with cache.reflections == 1, which continue but
 * never mirror again); a packet of A_k none of whose lanes hit is still mirrored and its walk is counted; in every call of chain A the
 * reflection blend comes before the transparency blend, and then the lights; lanes that level D would still select are counted in the
 * truncated-lane counter and treated as not selected.  Counter 0 after the call <=> the frame and the TreeStats are the reference's with
 * DBVH::HasShadingData() answering 1.  The keys, the clamps, the (slot 0, triId 0) quirk and GetSElement through Transform are those of
 * snail_instances_materials.h; the TreeStats accounting is that of snail_instances_materials_bounce.h and
 * snail_instances_materials_transparency.h added together.
 *
 * Conventions are those of snail_hip.h and snail_materials_tree.h: 0 = success, otherwise snail_last_error() holds the message and nothing was
 * written; lights7 is a HOST pointer to nLights (0..SNAIL_MAX_LIGHTS) x {pos[3], color[3], radius}; d_stats / stats += {intersects, iterations,
 * traced rays, skips}; both arithmetics.  Bad arguments are judged before the handle is looked at, the flags first; nPackets <= 0 and
 * nTiles <= 0 are no work (0).
 *
 * flags = SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_DEPTH | SNAIL_RENDER_AA4 in any combination, with the meanings of snail_instances_tiles.h;
 * anything else is refused with a text that names `flags`.  SNAIL_RENDER_DEPTH returns before the full-shading branch: the hit distances of the
 * primary walk alone, no level runs, the counter does not move.  Under SNAIL_RENDER_AA4 each of the four double-resolution RayTrace calls has
 * its own tree.  tint, ConvColor and the planar store are snail_instances_tiles.h's.
 *
 * Equivalences (bytes, TreeStats and the counter; counter 0 where the older function has none):
 *   (a) flags = 0, no tint                               snail_instances_materials_transparent_packets_dev at the same maxDepth
 *   (b) a set that cannot select a transparent lane      snail_instances_materials_bounce_packets_dev with flags 0 or SNAIL_RENDER_REFLECTIONS,
 *                                                        at every maxDepth
 *   (c) SNAIL_RENDER_DEPTH                               snail_instances_shade_packets_dev / snail_instances_render_tiles on the set's scene
 *                                                        with the same flags and tint
 *
 * Memory.  The levels' intermediates (D A-levels and, with the bounce, D + 1 B-levels reused by every chain; 4 nPackets packets each under
 * SNAIL_RENDER_AA4) are bounded per group of intermediates: the packet list runs in slices of whole output packets, back to back on the same
 * stream and arena, sized so that the levels stay within the set's level budget.  Packets are independent: slicing changes no byte and no
 * counter.  Launches are ordered against snail_instances_update / snail_instances_rebuild_dev as the handle's other launches are; the instance
 * records are read at launch.
 *
 * NOT here (the host renderer keeps them): the heat-map (gVals[5]) and per-packet TreeStats of these frames; frames dealt over several devices;
 * the ordered launches; routing in snail_adapter.hpp (no reference host can reach this branch through HipDBVH); creating sets for BLASes whose tree is
 * rebuilt on the device (snail_instances_materials_dynamic.h has that; its sets are taken here); maxDepth above 8 (the reference has no cut: a frame whose counter moved is not the
 * reference's).
 */
#ifndef SNAIL_INSTANCES_MATERIALS_TREE_H
#define SNAIL_INSTANCES_MATERIALS_TREE_H
#include "snail_instances_materials_transparency.h"
#include "snail_instances_materials_bounce.h"
#include "snail_materials_tree.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Scene::TraceReflection from a level's GENERIC packets (snail_instances_materials_mirror_packets_dev reads the primary ones): the arguments,
 * outputs and arithmetic of snail_materials_mirror_rays_dev (it reads nothing of the scene), with what snail_instances_trace_rays_dev needs
 * besides: d_element [n][256] and d_bary [n][64][2][4] are written as zeros -- the instanced walk leaves the object, element and barycentrics
 * of a lane without a hit as it found them, exactly as snail_instances_materials_mirror_packets_dev documents.  d_object (0) is that walk's
 * instance slot.  d_order_in (or NULL: every packet) is the level's own order list: for a packet whose word is negative d_order gets -1 and
 * NOTHING else of that packet is written, d_element and d_bary included; every other packet gets its index, whether or not a lane of it hit.
 * *d_stats (or NULL) += the nested call's TracingRays.  Buffers 16-byte aligned (the masks and order lists: any alignment).  Arguments are
 * judged before the handle. */
int snail_instances_materials_mirror_rays_dev(SnailInstancesMaterials *, int nPackets, const float *d_origin_in, const float *d_dir_in,
                                              const uint8_t *d_mask_in, const float *d_t, const float *d_samples, const int32_t *d_order_in,
                                              float *d_origin, float *d_dir, float *d_idir, uint8_t *d_mask, float *d_distance, int32_t *d_object,
                                              int32_t *d_element, float *d_bary, int32_t *d_order, uint64_t *d_stats, void *stream);

/* The lit packets of a packet list with any flag combination and tint (or NULL) -> packet-major B,G,R bytes [nPackets][256][3]; maxDepth
 * (1..SNAIL_MAT_TRANSP_MAX_DEPTH) and *d_truncated (a DEVICE word, +=), before the stats. */
int snail_instances_materials_tree_frame_packets_dev(SnailInstancesMaterials *, const float cam[13], int resx, int resy, const int32_t *d_packet_xy,
                                                     int nPackets, const float *lights7, int nLights, const float ambient[3], int flags,
                                                     const float *tint, uint8_t *d_bgr_packets, int maxDepth, uint64_t *d_truncated,
                                                     uint64_t *d_stats, void *stream);
/* The tile list of snail_instances_render_tiles (coords [nTiles][4] = x, y, w, h; offsets [nTiles] into data; per tile the planes R, G-R, B-R,
 * clipped to the image: what a tile holds beyond resx x resy is zero; one device-to-host copy) under full shading: + maxDepth and *truncated
 * (a HOST word, +=), before the stats.  One cached tile job per set: calls on one set take turns. */
int snail_instances_materials_tree_render_tiles(SnailInstancesMaterials *, const float cam[13], int resx, int resy, const int32_t *coords,
                                                const int64_t *offsets, int nTiles, const float *lights7, int nLights, const float ambient[3],
                                                int flags, const float *tint, uint8_t *data, int maxDepth, uint64_t *truncated, uint64_t stats[4]);
/* The image form, without tint: B,G,R rows of `pitch` bytes in host memory; + maxDepth and *truncated (a HOST word, +=), before the stats. */
int snail_instances_materials_tree_render_frame(SnailInstancesMaterials *, const float cam[13], int resx, int resy, const float *lights7, int nLights,
                                                const float ambient[3], int flags, uint8_t *image_bgr, int pitch, int maxDepth, uint64_t *truncated,
                                                uint64_t stats[4]);

/* The level budget of the set's groups of intermediates, in bytes (the default: SNAIL_MAT_LEVEL_BUDGET, snail_materials_tree.h).  A call clamps
 * it up to what ONE output packet needs, snail_instances_materials_level_bytes(nLights, flags, maxDepth): the bytes of the levels of one output
 * packet (4 double-resolution packets under SNAIL_RENDER_AA4; D A-levels, + D + 1 B-levels with SNAIL_RENDER_REFLECTIONS; 0 under
 * SNAIL_RENDER_DEPTH), or -1 for arguments the frame functions would refuse.
 * An instanced level carries the triId plane besides the instance slot, one plane more than a plain scene's: at 8 lights and maxDepth 8 with
 * the bounce and antialiasing one output packet (4 double-resolution packets) takes (8 + 9) levels x 140.75 KiB + 4.5 KiB = 2 397.25 KiB, so
 * under the default budget of 1 GiB a slice is 437 output packets and a 1920 x 1080 frame (8 160 packets, 18.7 GiB unsliced) runs in 19 slices. */
int snail_instances_materials_set_level_budget(SnailInstancesMaterials *, uint64_t bytes);
int64_t snail_instances_materials_level_bytes(int nLights, int flags, int maxDepth);

#ifdef __cplusplus
}
#endif
#endif
