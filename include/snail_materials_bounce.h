/*
 * snail_materials_bounce.h -- the one mirrored bounce of gVals[7] under full shading, on the device: Scene::RayTrace's call of
 * Scene::TraceReflection (src/scene_trace.cpp:454-466, :603-618) with the samples of snail_materials.h, i.e. the nested
 * RayTrace<0, hasMask> of the mirrored packets with materials, textures and interpolated normals on rays that do not come from the camera.
 * A header of its own: snail_materials.h (whose frame functions keep refusing every nonzero flag), snail_hip.h and their symbol lists stay
 * as they are.  Plain C.
 *
 * The nested call never bounces again (cache.reflections < 1), and no set these functions accept can select a transparent lane (a set of
 * snail_materials_create_transparent that can is refused, snail_materials_transparency.h), so it takes neither continuation.
 *
 * NOT here: 4x antialiasing, depth shading, the tint and tile lists with the bounce are snail_materials_tiles.h's, and with them the adapter's
 * routing of a call with gVals[6] (SNAIL_ADAPTER_DEVICE_MATERIALS, snail_adapter.hpp); the transparent kinds and the frames of the
 * transparency continuation are snail_materials_transparency.h's.  The host renderer keeps the transparency continuation together with
 * the bounce, multi-device frames and the ordered launches (dispatch-order feedback) under the bounce; the heat-map (gVals[5]) of full shading,
 * with and without the bounce, is snail_materials_heatmap.h's.
 */
#ifndef SNAIL_MATERIALS_BOUNCE_H
#define SNAIL_MATERIALS_BOUNCE_H
#include "snail_materials.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the mirror stage -----------------------------------------------------------------------------------------------------------------------
 * Scene::TraceReflection on the primary samples of a packet list: per ray reflDir = Reflect(dir, normal) with the normal of d_samples (the
 * buffer of snail_materials_shade_packets_dev: the INTERPOLATED normal, zeros on a lane that missed), reflOrig = position + reflDir * 0.001,
 * idir = SafeInv(reflDir); the selector is the set of lanes that hit (d_t < inf).  Output in the layouts snail_trace_rays_dev takes, 64
 * quads per packet: d_origin / d_dir / d_idir [nPackets][64][3][4], d_mask [nPackets][64] (one byte per quad, low 4 bits = lanes),
 * d_distance [nPackets][256] (inf for a selected lane, -inf for a masked one), d_object [nPackets][256] (0).  Masked lanes: zeros.
 * d_stats (optional) += the nested call's TracingRays: the selected lanes.  Buffers 16-byte aligned. */
int snail_materials_mirror_packets_dev(SnailMaterials *, const float cam[13], int resx, int resy, const int32_t *d_packet_xy, int nPackets, const float *d_t,
                                       const float *d_samples, float *d_origin, float *d_dir, float *d_idir, uint8_t *d_mask, float *d_distance,
                                       int32_t *d_object, uint64_t *d_stats, void *stream);

/* ---- the sample stage on generic packets ------------------------------------------------------------------------------------------------------
 * The full-shading branch (src/scene_trace.cpp:145-358) for RayGroup<0, hasMask>: packets of 64 quads whose directions d_dir
 * [nPackets][64][3][4] are the caller's, with hit records d_t / d_u / d_v / d_triId [nPackets][256] (distance and object as
 * snail_trace_rays_dev writes them for such packets; u and v as two planes, as snail_trace_packets_dev writes them) and d_mask
 * [nPackets][64] or NULL = every lane selected.  A lane counts as hit when t < inf AND its mask bit is set (a masked lane carries
 * -inf).  hasMask is the PACKET's: a packet whose 256 lanes are all selected is shaded as
 * RayGroup<0, 0>, any other as RayGroup<0, 1> (:615-617).  It shows in branch (a) alone -- one triangle for a full block calls Shade with the
 * packet's hasMask (:224), so SNAIL_MAT_UBER takes `specular` there on a masked packet and the sample's diffuse on an unmasked one; branch
 * (b)'s single-material call is unmasked whatever the packet is (:308), branch (c) masked.  Everything else as
 * snail_materials_shade_packets_dev; d_samples [nPackets][9][64][4]. */
int snail_materials_shade_rays_dev(SnailMaterials *, int nPackets, const float *d_dir, const uint8_t *d_mask, const float *d_t, const float *d_u,
                                   const float *d_v, const int32_t *d_triId, float *d_samples, void *stream);

/* ---- lit frames with the bounce -----------------------------------------------------------------------------------------------------------------
 * The arguments of snail_render_materials_dev / _packets_dev / _image.  flags: 0 or SNAIL_RENDER_REFLECTIONS (snail_hip.h); anything else
 * is refused with a text that names `flags`, before the handle is looked at.  flags == 0: exactly what those functions produce.  With the
 * flag: primary packets -> samples -> mirrored packets -> their walk (TraversePrimary<0, 1>, with barycentrics) -> nested samples -> nested
 * lights (the packet-level cull and Scene::TraceLight on the nested samples; position = reflDir * t + reflOrig) -> nested colour = diffuse *
 * lDiffuse + specular * lSpecular (diffuse alone without lights), float -> primary lights -> on the lanes that hit, diffuse += (colour -
 * diffuse) * 0.3 before the lights (specular untouched; the primary lights keep the primary sample's normal) -> ConvColor -> B,G,R.
 * stats += primary rays, the mirrored packets' selected lanes and walk, the nested shadow lanes with N.L > 0 and their walks, the primary
 * shadow lanes and walks.  The additional intermediates belong to the set's 8 event-guarded groups and exist only once a bounce was asked
 * for. */
int snail_materials_bounce_dev(SnailMaterials *, const float cam[13], int resx, int resy, const float *lights7, int nLights, const float ambient[3],
                               int flags, uint8_t *d_frame_bgr, int pitch, uint64_t *d_stats, void *stream);
int snail_materials_bounce_packets_dev(SnailMaterials *, const float cam[13], int resx, int resy, const int32_t *d_packet_xy, int nPackets,
                                       const float *lights7, int nLights, const float ambient[3], int flags, uint8_t *d_bgr_packets, uint64_t *d_stats,
                                       void *stream);
int snail_materials_bounce_image(SnailMaterials *, const float cam[13], int resx, int resy, const float *lights7, int nLights, const float ambient[3],
                                 int flags, uint8_t *image_bgr, int pitch, uint64_t stats[4]);

#ifdef __cplusplus
}
#endif
#endif
