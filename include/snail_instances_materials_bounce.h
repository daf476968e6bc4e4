/*
 * snail_instances_materials_bounce.h -- the one mirrored bounce of gVals[7] under full shading of a two-level instanced scene, on the device:
 * Scene<DBVH>::RayTrace's call of Scene::TraceReflection (src/scene_trace.cpp:454-466, :603-618) with the samples of
 * snail_instances_materials.h, i.e. the nested RayTrace<0, hasMask> of the mirrored packets with materials, textures and interpolated, rotated
 * normals on rays that do not come from the camera and hit several instances.  A header of its own: snail_instances_materials.h (whose frame
 * functions keep refusing every nonzero flag), snail_materials_bounce.h, snail_instances.h and their symbol lists stay as they are.  Plain C.
 *
 * The nested call never bounces again (cache.reflections < 1), and no set snail_instances_materials_create accepts can select a transparent
 * lane, so it takes neither continuation; a set of snail_instances_materials_create_transparent that can is refused by every function here.
 *
 * NOT here: tile lists, 4x antialiasing and the tint with the bounce, and the transparency continuation together with it
 * (snail_instances_materials_tree.h has them; snail_instances_materials_transparency.h: the continuation without the bounce); the heat-map
 * (gVals[5]) under full shading of instanced scenes (not on the device); multi-device frames; routing in snail_adapter.hpp (no reference host can reach this branch through HipDBVH);
 * creating sets for BLASes whose tree is rebuilt on the device (snail_instances_materials_dynamic.h has that; its sets are taken here).
 */
#ifndef SNAIL_INSTANCES_MATERIALS_BOUNCE_H
#define SNAIL_INSTANCES_MATERIALS_BOUNCE_H
#include "snail_instances_materials.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the mirror stage -----------------------------------------------------------------------------------------------------------------------
 * Scene::TraceReflection on the primary samples of a packet list: per ray reflDir = Reflect(dir, normal) with the normal of d_samples (the
 * buffer of snail_instances_materials_shade_packets_dev: the INTERPOLATED, ROTATED normal, zeros on a lane that missed), reflOrig = position +
 * reflDir * 0.001, idir = SafeInv(reflDir); the selector is the set of lanes that hit (d_t < inf).  The arithmetic is that of
 * snail_materials_mirror_packets_dev: it reads nothing of the scene.  Output: exactly what snail_instances_trace_rays_dev takes as in/out for
 * packets of 64 quads with per-ray origins: d_origin / d_dir / d_idir [nPackets][64][3][4], d_mask [nPackets][64] (one byte per quad, low 4 bits =
 * lanes), d_distance [nPackets][256] (inf for a selected lane, -inf for a masked one), d_object / d_element [nPackets][256] (0) and d_bary
 * [nPackets][64][2][4] (0): the instanced walk leaves the object, element and barycentrics of a lane without a hit as it found them, so they are
 * defined here.  Masked lanes: zeros everywhere.  d_stats (optional) += the nested call's TracingRays: the selected lanes.  Buffers 16-byte
 * aligned (the mask: any alignment).  This function and the next judge their arguments before the handle: nPackets <= 0 is no work (0), a
 * null or misaligned buffer is refused whatever the handle is. */
int snail_instances_materials_mirror_packets_dev(SnailInstancesMaterials *, const float cam[13], int resx, int resy, const int32_t *d_packet_xy, int nPackets,
                                                 const float *d_t, const float *d_samples, float *d_origin, float *d_dir, float *d_idir, uint8_t *d_mask,
                                                 float *d_distance, int32_t *d_object, int32_t *d_element, float *d_bary, uint64_t *d_stats, void *stream);

/* ---- the sample stage on generic packets ------------------------------------------------------------------------------------------------------
 * The full-shading branch (src/scene_trace.cpp:145-358) for RayGroup<0, hasMask> of a DBVH: packets of 64 quads whose directions d_dir
 * [nPackets][64][3][4] are the caller's, with hit records d_t / d_inst / d_triId [nPackets][256] and d_bary [nPackets][64][2][4] = the distance,
 * object, element and bary of snail_instances_trace_rays_dev for such packets (bary interleaved per quad: four u, then four v), and d_mask
 * [nPackets][64] or NULL = every lane selected.  A lane counts as hit when t < inf AND its mask bit is set (a masked lane carries -inf).
 * hasMask is the PACKET's, as in snail_materials_shade_rays_dev: a packet whose 256 lanes are all selected is shaded as RayGroup<0, 0>, any other
 * as RayGroup<0, 1>; branch (a) shades with it (SNAIL_MAT_UBER takes `specular` there on a masked packet and the sample's diffuse on an
 * unmasked one), branch (b)'s single-material call is unmasked whatever the packet is, branch (c) masked.  Everything else is
 * snail_instances_materials_shade_packets_dev's: the keys are the pairs (slot, triId), a lane that is not hit carries (0, 0), the (slot 0,
 * triId 0) quirk, GetSElement through Transform, and the clamps of a slot or triId outside the scene written in snail_instances_materials.h.
 * The instance records are read at launch.  d_samples [nPackets][9][64][4]; buffers 16-byte aligned (the mask: any alignment). */
int snail_instances_materials_shade_rays_dev(SnailInstancesMaterials *, int nPackets, const float *d_dir, const uint8_t *d_mask, const float *d_t,
                                             const float *d_bary, const int32_t *d_inst, const int32_t *d_triId, float *d_samples, void *stream);

/* ---- lit frames with the bounce -----------------------------------------------------------------------------------------------------------------
 * The arguments of snail_instances_render_materials_dev / _packets_dev / _image.  flags: 0 or SNAIL_RENDER_REFLECTIONS (snail_hip.h); anything
 * else is refused with a text that names `flags`, before the handle is looked at.  flags == 0: exactly what those functions produce.  With the
 * flag: primary packets (DBVH::TraversePrimary, with barycentrics) -> samples -> mirrored packets -> their walk (DBVH::TraversePrimary<0, 1>,
 * with barycentrics) -> nested samples -> nested lights (the packet-level cull and Scene::TraceLight on the nested samples; position = reflDir *
 * t + reflOrig; DBVH::TraverseShadow) -> nested colour = diffuse * lDiffuse + specular * lSpecular (diffuse alone without lights), float ->
 * primary lights -> on the lanes that hit, diffuse += (colour - diffuse) * 0.3 before the lights (specular untouched; the primary lights keep
 * the primary sample's normal) -> ConvColor -> B,G,R.
 * stats += primary rays and walk, the mirrored packets' selected lanes and walk, the nested shadow lanes with N.L > 0 and their walks, the
 * primary shadow lanes and walks: the accounting of snail_materials_bounce.h with the walk counters of snail_instances.h.  The additional
 * intermediates belong to the set's 8 event-guarded groups and exist only once a bounce was asked for; launches are ordered against
 * snail_instances_update and snail_instances_rebuild_dev as the handle's other launches are. */
int snail_instances_materials_bounce_dev(SnailInstancesMaterials *, const float cam[13], int resx, int resy, const float *lights7, int nLights,
                                         const float ambient[3], int flags, uint8_t *d_frame_bgr, int pitch, uint64_t *d_stats, void *stream);
int snail_instances_materials_bounce_packets_dev(SnailInstancesMaterials *, const float cam[13], int resx, int resy, const int32_t *d_packet_xy, int nPackets,
                                                 const float *lights7, int nLights, const float ambient[3], int flags, uint8_t *d_bgr_packets,
                                                 uint64_t *d_stats, void *stream);
int snail_instances_materials_bounce_image(SnailInstancesMaterials *, const float cam[13], int resx, int resy, const float *lights7, int nLights,
                                           const float ambient[3], int flags, uint8_t *image_bgr, int pitch, uint64_t stats[4]);

#ifdef __cplusplus
}
#endif
#endif
