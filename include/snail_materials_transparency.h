/*
 * snail_materials_transparency.h -- transparent materials under full shading, on the device: the material kinds that can select a transparent
 * lane (TransparentMaterial<NDotR>, src/shading/transparent_material.h; UberMaterial with 0 < dissolve < 1, src/shading/uber_material.h), the
 * sample stages with Sample::opacity and the transSel selector (src/scene_trace.cpp:190, :306, :347-349, :472), and the generator of
 * Scene::TraceTransparency's packets (:620-634) from full-shading samples and, below the first level, from generic packets.
 * A header of its own: snail_materials.h, _bounce.h, _tiles.h and their symbol lists stay as they are.  Plain C.
 *
 * The frames at the end run these stages level by level and blend back up (:468-483).
 *
 * NOT here (the host renderer keeps them): transparency together with the bounce (with gVals[7] the reference nests a bounce inside every
 * continuation and continuations inside the bounce, a tree of calls), tiles / 4x antialiasing / the tint with transparency -- so every entry
 * point of snail_materials.h, _bounce.h and _tiles.h refuses a set that can select a transparent lane (below), and the adapter's
 * SNAIL_ADAPTER_DEVICE_MATERIALS routing, which goes through the tile functions, leaves such a set's frames with the reference's own renderer --
 * multi-device frames, MTL / OBJ ingest, the rgba8, DXT and SAT samplers (the heat-map, gVals[5], of full shading is snail_materials_heatmap.h's).
 */
#ifndef SNAIL_MATERIALS_TRANSPARENCY_H
#define SNAIL_MATERIALS_TRANSPARENCY_H
#include "snail_materials_bounce.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the deepest level a frame may ask for (the reference has no limit; lanes a deeper level would still select are counted, not traced) */
enum { SNAIL_MAT_TRANSP_MAX_DEPTH = 8 };

/* ---- creation -----------------------------------------------------------------------------------------------------------------------------
 * snail_materials_create with the kinds it refuses.  Accepted beyond it:
 *   SNAIL_MAT_TRANSPARENT  TransparentMaterial<nDotR> over two PointSamplers: `texture` is the colour map, opacityTexture[k] the opacity map
 *                          (both validated against nTex).  Flags fTexCoords | fTransparency.  Both maps are sampled WITHOUT mip-mapping
 *                          (Sample(samples, sc, 0): level 0 whatever texDiff says); diffuse = colour [* (d.n), no Abs], specular = diffuse,
 *                          opacity = the opacity sample's first channel (byte 0 of a texel), masked path and unmasked path alike
 *   SNAIL_MAT_UBER         with any dissolve but NaN (which stays refused): opacity = dissolve, fTransparency iff dissolve > 0
 * opacityTexture: int32 [nMats], read for SNAIL_MAT_TRANSPARENT entries only; may be NULL when no entry is of that kind.
 * Every other rule, refusal and text of snail_materials_create holds; snail_materials_create itself keeps refusing exactly what it refused. */
SnailMaterials *snail_materials_create_transparent(SnailScene *scene, const void *shtris64, int nTris, const int32_t *matMap, int nMap,
                                                   const SnailMaterial *mats, int nMats, const int32_t *opacityTexture, const SnailTexture *textures,
                                                   int nTex);

/* 1 when the set holds a material that can select a transparent lane (SNAIL_MAT_TRANSPARENT, or SNAIL_MAT_UBER with 0 < dissolve < 1), 0 when it
 * holds none (every set of snail_materials_create), -1 for a NULL handle.  Every entry point of snail_materials.h, snail_materials_bounce.h and
 * snail_materials_tiles.h that takes a set returns an error naming "transparent" for a set that answers 1, before anything touches a device:
 * their kernels do not know the kind. */
int snail_materials_can_select_transparent(const SnailMaterials *);

/* ---- the sample stages with transparency ----------------------------------------------------------------------------------------------------
 * snail_materials_shade_packets_dev / snail_materials_shade_rays_dev (whose arguments and nine sample planes these are, byte for byte for a
 * set without a transparent-capable material) for ANY set, with two more outputs:
 *   d_opacity [nPackets][256]  Sample::opacity per ray: the opacity sample's first channel (SNAIL_MAT_TRANSPARENT), dissolve (SNAIL_MAT_UBER);
 *                              0 for the kinds that never write it and for a lane that missed
 *   d_sel [nPackets][64]       one byte per quad, low 4 bits = transSel AFTER the opacity < 1 filter (:472).
 * Every buffer but d_sel (and d_packet_xy) 16-byte aligned, the hit records included.
 * The selector as the reference writes it: branches (a) and (b) give the whole block its ONE material's flag; branch (c) ASSIGNS
 * transSel[b4 + q] = mask[q] for every material of the block that carries fTransparency, in the order of its material list -- first appearance
 * over the quads, then the lanes, among the selected lanes -- so the LAST flagged material of a block wins and de-selects the lanes of an
 * earlier one.  SNAIL_MAT_UBER with dissolve >= 1 is flagged, never has opacity < 1, and still takes a SNAIL_MAT_TRANSPARENT neighbour's lanes
 * out of the selector that way. */
int snail_materials_shade_packets_transp_dev(SnailMaterials *, const float cam[13], int resx, int resy, const int32_t *d_packet_xy, int nPackets,
                                             const float *d_t, const float *d_u, const float *d_v, const int32_t *d_triId, float *d_samples,
                                             float *d_opacity, uint8_t *d_sel, void *stream);
int snail_materials_shade_rays_transp_dev(SnailMaterials *, int nPackets, const float *d_dir, const uint8_t *d_mask, const float *d_t,
                                          const float *d_u, const float *d_v, const int32_t *d_triId, float *d_samples, float *d_opacity,
                                          uint8_t *d_sel, void *stream);

/* ---- the continuation generator -----------------------------------------------------------------------------------------------------------------
 * Scene::TraceTransparency's packets (:620-634) of one level from that level's rays, hits d_t [nPackets][256] and selector d_sel
 * [nPackets][64] (the byte the sample stages write): per selected ray origin = dir * (t + 0.001) + origin, dir and idir as the level carries
 * them.  The level's rays: cam / resx / resy / d_packet_xy for the primary level (d_origin_in = d_dir_in = d_idir_in = NULL; idir =
 * SafeInv(dir), as the primary RayGroup carries it), or the generic packets d_origin_in / d_dir_in / d_idir_in [nPackets][64][3][4] (cam and
 * d_packet_xy are then not read and may be NULL).  A lane is selected when its bit of d_sel is set and d_t < inf.
 * Output: the next level's packets in the layouts snail_trace_rays_dev takes, as snail_materials_mirror_packets_dev writes them -- d_origin /
 * d_dir [nPackets][64][3][4] with zeros for masked lanes, d_idir (SafeInv(0) for masked lanes, as there), d_mask [nPackets][64], d_distance
 * [nPackets][256] (inf selected, -inf masked), d_object (0) -- and d_order [nPackets] (int32): the packet's index when any of its lanes is
 * selected, -1 otherwise: the order list under which a walk leaves out the packets that make no nested call.
 * d_stats (optional) += the nested call's TracingRays: the selected lanes.  Buffers 16-byte aligned; outputs must not alias inputs. */
int snail_materials_continue_packets_dev(SnailMaterials *, const float cam[13], int resx, int resy, const int32_t *d_packet_xy, int nPackets,
                                         const float *d_origin_in, const float *d_dir_in, const float *d_idir_in, const float *d_t,
                                         const uint8_t *d_sel, float *d_origin, float *d_dir, float *d_idir, uint8_t *d_mask, float *d_distance,
                                         int32_t *d_object, int32_t *d_order, uint64_t *d_stats, void *stream);

/* ---- frames with the continuation -----------------------------------------------------------------------------------------------------------
 * The arguments of snail_render_materials_dev / _packets_dev / _image, plus maxDepth (1 .. SNAIL_MAT_TRANSP_MAX_DEPTH) and a truncated-lane
 * counter (a DEVICE word for the _dev functions, a host word for _image; += as the stats).  flags must be 0: anything else, including
 * SNAIL_RENDER_REFLECTIONS, is refused with a text that names `flags`, before the handle is looked at.  Any set is accepted.
 * Way down: primary walk -> sample -> for level L = 1 .. maxDepth: generator (from level L - 1's rays, hits and selector) -> the walk of the
 * generated packets (per-ray origins, mask, barycentrics, under the generator's order list: a packet without a selected lane takes no part in
 * level L or any deeper level, in any stage -- no rays, no walk, no light) -> nested sample.  Lanes that level maxDepth still selects are
 * added to the counter and treated as NOT selected: they keep their own diffuse.  Way up: for L = maxDepth .. 1: on the lanes level L
 * selected, diffuse = transColor + (diffuse - transColor) * opacity with transColor = level L + 1's colour (VLerp, veclib/vecbase.h:81; before
 * the lights, specular untouched) -> the packet-level cull and Scene::TraceLight on level L's samples -> colour = diffuse * lDiffuse +
 * specular * lSpecular (diffuse alone without lights), float.  Then the same blend on the primary samples from level 1's colour, the primary
 * lights, ConvColor, B,G,R.  The frame is the reference's byte for byte whenever the counter stays unchanged, and stats add up as in the
 * reference: primary rays and walk, per level the selected lanes and their walk, the shadow lanes with N.L > 0 and their walks.
 * The _dev calls are stream-ordered without host synchronisation (apart from buffer growth); the per-level intermediates are a fourth, lazily
 * allocated part of the set's 8 event-guarded groups, sized by the depth asked for. */
int snail_materials_transparent_dev(SnailMaterials *, const float cam[13], int resx, int resy, const float *lights7, int nLights, const float ambient[3],
                                    int flags, uint8_t *d_frame_bgr, int pitch, int maxDepth, uint64_t *d_truncated, uint64_t *d_stats, void *stream);
int snail_materials_transparent_packets_dev(SnailMaterials *, const float cam[13], int resx, int resy, const int32_t *d_packet_xy, int nPackets,
                                            const float *lights7, int nLights, const float ambient[3], int flags, uint8_t *d_bgr_packets, int maxDepth,
                                            uint64_t *d_truncated, uint64_t *d_stats, void *stream);
int snail_materials_transparent_image(SnailMaterials *, const float cam[13], int resx, int resy, const float *lights7, int nLights, const float ambient[3],
                                      int flags, uint8_t *image_bgr, int pitch, int maxDepth, uint64_t *truncated, uint64_t stats[4]);

#ifdef __cplusplus
}
#endif
#endif
