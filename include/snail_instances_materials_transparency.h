/*
 * snail_instances_materials_transparency.h -- transparent materials under full shading of a two-level instanced scene, on the device: the
 * transparency continuation of Scene<DBVH>::RayTrace (src/scene_trace.cpp:468-483) and Scene::TraceTransparency (:620-634, instantiated for DBVH
 * at :657-659) with the samples of snail_instances_materials.h, i.e. what snail_materials_transparency.h is for a plain scene: the material kinds
 * that can select a transparent lane (TransparentMaterial<NDotR>, src/shading/transparent_material.h; UberMaterial's dissolve), the sample stages
 * with Sample::opacity and the transSel selector, the generator of the next level's packets, and the frames that run the levels down and blend
 * back up -- with the DBVH walk on per-ray origins, the (slot, triId) keys, GetSElement through ShTriangle::Transform and DBVH::TraverseShadow.
 * As with the rest of instanced full shading, DBVH::HasShadingData() answering 1 is THIS PROJECT's completion of the reference's TODO
 * (src/dbvh/tree.h:207-209); everything below it is the reference's own code path.
 * A header of its own: snail_instances_materials.h, snail_instances_materials_bounce.h, snail_materials_transparency.h and their symbol lists stay
 * as they are.  Plain C.
 *
 * NOT here: the continuation together with the bounce on instanced scenes (with gVals[7] the reference nests a bounce inside every continuation and
 * continuations inside the bounce, a tree of calls), tile lists, 4x antialiasing and the tint: snail_instances_materials_tree.h has them, for any
 * set, and the frames here keep refusing every nonzero flag; the heat-map (gVals[5]) for instanced full shading (not on the device);
 * multi-device frames; routing in snail_adapter.hpp (no reference host can reach this branch through HipDBVH); device-packed records for BLASes
 * whose tree is rebuilt on the device (snail_instances_materials_dynamic.h has them; its sets are taken here).
 */
#ifndef SNAIL_INSTANCES_MATERIALS_TRANSPARENCY_H
#define SNAIL_INSTANCES_MATERIALS_TRANSPARENCY_H
#include "snail_instances_materials_bounce.h"
#include "snail_materials_transparency.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- creation -----------------------------------------------------------------------------------------------------------------------------
 * snail_instances_materials_create with the kinds it refuses: accepted beyond it is exactly what snail_materials_create_transparent accepts
 * beyond snail_materials_create -- SNAIL_MAT_TRANSPARENT (colour map `texture`, opacity map opacityTexture[k], both validated against nTex) and
 * SNAIL_MAT_UBER with any dissolve but NaN.  opacityTexture: int32 [nMats], read for SNAIL_MAT_TRANSPARENT entries only; may be NULL when no
 * entry is of that kind.  Every other rule, refusal and text of snail_instances_materials_create holds; snail_instances_materials_create itself
 * keeps refusing exactly what it refused. */
SnailInstancesMaterials *snail_instances_materials_create_transparent(SnailInstances *, const SnailBlasShading *perBlas, int nBlas, const SnailMaterial *mats,
                                                                      int nMats, const int32_t *opacityTexture, const SnailTexture *textures, int nTex);

/* 1 when the set holds a material that can select a transparent lane (SNAIL_MAT_TRANSPARENT, or SNAIL_MAT_UBER with 0 < dissolve < 1), 0 when it
 * holds none (every set of snail_instances_materials_create), -1 for a NULL handle.  Every entry point of snail_instances_materials.h and
 * snail_instances_materials_bounce.h that takes a set returns an error naming "transparent" for a set that answers 1, before anything touches a
 * device: their kernels do not know the kind. */
int snail_instances_materials_can_select_transparent(const SnailInstancesMaterials *);

/* ---- the sample stages with transparency ----------------------------------------------------------------------------------------------------
 * snail_instances_materials_shade_packets_dev / snail_instances_materials_shade_rays_dev (whose arguments and nine sample planes these are, byte
 * for byte for a set without a transparent-capable material) for ANY set, with two more outputs:
 *   d_opacity [nPackets][256]  Sample::opacity per ray: the opacity sample's first channel (SNAIL_MAT_TRANSPARENT), dissolve (SNAIL_MAT_UBER); 0
 *                              for the kinds that never write it and for a lane that missed
 *   d_sel [nPackets][64]       one byte per quad, low 4 bits = transSel AFTER the opacity < 1 filter (:472)
 * (both all zero for a set without a capable material).  The selector rule is the one snail_materials_transparency.h documents: branches (a) and
 * (b) give the whole block its ONE material's flag; in branch (c) the LAST flagged material of the block's list -- first appearance over the
 * quads, then the lanes, among the selected lanes -- wins and de-selects the lanes of an earlier one.  A material's identity is its index in the
 * ONE scene-wide list: two BLASes' triangles that map to the same entry are one candidate.  Everything about keys is
 * snail_instances_materials_shade_packets_dev's: the pairs (slot, triId), the (slot 0, triId 0) quirk, the clamps of a slot or triId outside the
 * scene, GetSElement through Transform.  TransparentMaterial carries fTexCoords (branch (a) interpolates its texture coordinates), and both its
 * maps are sampled at mip level 0.  Every buffer but d_sel, d_mask and d_packet_xy 16-byte aligned, the hit records included.  These functions
 * judge their arguments before the handle: nPackets <= 0 is no work (0), a null or misaligned buffer is refused whatever the handle is.  The
 * instance records are read at launch. */
int snail_instances_materials_shade_packets_transp_dev(SnailInstancesMaterials *, const float cam[13], int resx, int resy, const int32_t *d_packet_xy,
                                                       int nPackets, const float *d_t, const float *d_u, const float *d_v, const int32_t *d_inst,
                                                       const int32_t *d_triId, float *d_samples, float *d_opacity, uint8_t *d_sel, void *stream);
int snail_instances_materials_shade_rays_transp_dev(SnailInstancesMaterials *, int nPackets, const float *d_dir, const uint8_t *d_mask, const float *d_t,
                                                    const float *d_bary, const int32_t *d_inst, const int32_t *d_triId, float *d_samples, float *d_opacity,
                                                    uint8_t *d_sel, void *stream);

/* ---- the continuation generator -----------------------------------------------------------------------------------------------------------------
 * snail_materials_continue_packets_dev (its arguments, outputs and arithmetic: it reads nothing of the scene) for an instanced set, with what
 * snail_instances_trace_rays_dev needs besides: d_element [nPackets][256] and d_bary [nPackets][64][2][4] are written as zeros -- the instanced
 * walk leaves the element and barycentrics of a lane without a hit as it found them, exactly as snail_instances_materials_mirror_packets_dev
 * documents.  d_object (0) is that walk's instance slot.  d_order[p] = p when any lane of packet p is selected, -1 otherwise; d_stats (optional)
 * += the selected lanes.  Arguments are judged before the handle, as above. */
int snail_instances_materials_continue_packets_dev(SnailInstancesMaterials *, const float cam[13], int resx, int resy, const int32_t *d_packet_xy,
                                                   int nPackets, const float *d_origin_in, const float *d_dir_in, const float *d_idir_in, const float *d_t,
                                                   const uint8_t *d_sel, float *d_origin, float *d_dir, float *d_idir, uint8_t *d_mask, float *d_distance,
                                                   int32_t *d_object, int32_t *d_element, float *d_bary, int32_t *d_order, uint64_t *d_stats, void *stream);

/* ---- frames with the continuation -----------------------------------------------------------------------------------------------------------
 * The arguments of snail_instances_render_materials_dev / _packets_dev / _image, plus maxDepth (1 .. SNAIL_MAT_TRANSP_MAX_DEPTH) and a
 * truncated-lane counter (a DEVICE word for the _dev functions, a host word for _image; += as the stats).  flags must be 0: anything else,
 * including SNAIL_RENDER_REFLECTIONS, is refused with a text that names `flags`, before the handle is looked at.  Any set is accepted.
 * Semantics are exactly the "way down / way up" paragraph of snail_materials_transparency.h with DBVH::TraversePrimary<0, 1> on the generated
 * packets (per-ray origins, mask, barycentrics), the (slot, triId) samples and DBVH::TraverseShadow: a packet whose order word is negative takes
 * part in no stage of that level or of any deeper level -- no rays, no walk, no light, no TreeStats; lanes that level maxDepth would still select
 * are counted and treated as not selected; stats += the primary rays and walk, per level the selected lanes and their walk, the shadow lanes with
 * N.L > 0 and their walks.  The per-level intermediates are a lazily allocated part of the set's 8 event-guarded groups, sized by the depth asked
 * for; launches are ordered against snail_instances_update / snail_instances_rebuild_dev as the handle's other launches are; the instance records
 * are read at launch. */
int snail_instances_materials_transparent_dev(SnailInstancesMaterials *, const float cam[13], int resx, int resy, const float *lights7, int nLights,
                                              const float ambient[3], int flags, uint8_t *d_frame_bgr, int pitch, int maxDepth, uint64_t *d_truncated,
                                              uint64_t *d_stats, void *stream);
int snail_instances_materials_transparent_packets_dev(SnailInstancesMaterials *, const float cam[13], int resx, int resy, const int32_t *d_packet_xy,
                                                      int nPackets, const float *lights7, int nLights, const float ambient[3], int flags,
                                                      uint8_t *d_bgr_packets, int maxDepth, uint64_t *d_truncated, uint64_t *d_stats, void *stream);
int snail_instances_materials_transparent_image(SnailInstancesMaterials *, const float cam[13], int resx, int resy, const float *lights7, int nLights,
                                                const float ambient[3], int flags, uint8_t *image_bgr, int pitch, int maxDepth, uint64_t *truncated,
                                                uint64_t stats[4]);

#ifdef __cplusplus
}
#endif
#endif
