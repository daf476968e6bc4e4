/*
 * snail_instances_shade.h -- lit frames of the two-level instanced scenes of snail_instances.h: Scene<DBVH>::RayTrace in the simple-shading
 * configuration (lights, one shadow packet per light, one mirrored bounce) on the device.  Part of snail_instances.h, which includes this
 * file after its traversal entry points: a host includes snail_instances.h and gets both.
 */
#ifndef SNAIL_INSTANCES_SHADE_H
#define SNAIL_INSTANCES_SHADE_H
#include "snail_instances.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- lit frames: Scene<DBVH>::RayTrace in the simple-shading configuration, entirely on the device -----------------------------------
 * DBVH::HasShadingData() is 0, so an instanced scene always takes the simple-shading branch (src/scene_trace.cpp:359-452); RayTrace,
 * TraceLight and TraceReflection are instantiated for DBVH (:642-659).  The pipeline is that of snail_render_whitted_dev (snail_hip.h) with
 * the walks of this header: DBVH::TraversePrimary of the primary packets; samples (position = d*t + o, diffuse = specular = color*|d.n|)
 * whose normal is ObjectInstance::GetNormal = TransformVec(blas.GetNormal(triId)) (src/dbvh/tree.h:21-26,178-181,216-218: the plane normal
 * of triangle triId in the BLAS of the hit's instance slot, x*r.x + y*r.y + z*r.z per rotation row, added left to right); per light the
 * packet-level cull BoxPointDistanceSq(bbox of the packet's hit points, light) > radSq (:494-501) and Scene::TraceLight (:523-601) with
 * DBVH::TraverseShadow (shared origin = the light, no early out at the top level); outColor = diffuse*lDiffuse + specular*lSpecular
 * (:484-512); ConvColor -> B,G,R bytes.  SNAIL_WHITTED_REFLECTIONS = gVals[7], one bounce (:454-466): Scene::TraceReflection (:603-618)
 * mirrors every hit ray about its world-space normal (origin = hit point + 0.001 direction, SafeInv, lane masks = hit lanes), walks the
 * packets as DBVH::TraversePrimary<0,1>, shades them by the same RayTrace (no further bounce) and blends diffuse += (reflected colour -
 * diffuse) * 0.3 on hit lanes.  Lanes the reference leaves uninitialised (misses) are zeros and masked, as for a plain scene.
 * Conventions of snail_render_whitted_dev / _packets_dev / snail_render_image: lights7 is a HOST pointer to nLights (0..SNAIL_MAX_LIGHTS) x
 * {pos[3], color[3], radius}; every pixel inside resx x resy gets its own colour (the store rule of snail_hip.h); d_stats / stats +=
 * {intersects, iterations, traced rays, skips}, traced rays = primary rays + mirrored lanes + shadow lanes with N.L > 0, the walk counters
 * those of the top-level and inner walks as defined above; both arithmetics (table look-ups in their fully checked form).
 * The `_dev` forms keep their intermediates (hits, shadow distances [light][packet][256], mirrored packets and colours) in the handle, one
 * set per launch in flight (8 sets, round-robin, each guarded by an event), and a whole frame's packet list cached by packet-grid size;
 * concurrency and the ordering against snail_instances_update are those of the other launches of this header. */
int snail_instances_render_whitted_dev(SnailInstances *, const float cam[13], int resx, int resy, const float *lights7, int nLights,
                                       const float ambient[3], const float color[3], int flags, uint8_t *d_frame_bgr, int pitch,
                                       uint64_t *d_stats, void *stream);
/* ... for an explicit list of packets: packet-major B,G,R bytes [nPackets][256][3] (4-byte aligned), as snail_render_whitted_packets_dev. */
int snail_instances_render_whitted_packets_dev(SnailInstances *, const float cam[13], int resx, int resy, const int32_t *d_packet_xy,
                                               int nPackets, const float *lights7, int nLights, const float ambient[3],
                                               const float color[3], int flags, uint8_t *d_bgr_packets, uint64_t *d_stats, void *stream);
/* Render(scene, camera, image, options, threads) (src/render.h:21-23) of an instanced scene into a host image of `pitch` bytes per row:
 * flags & SNAIL_RENDER_DEPTH = snail_instances_render_depth (lights ignored), otherwise the lit frame above, SNAIL_RENDER_REFLECTIONS =
 * gVals[7].  SNAIL_RENDER_AA4 is refused (non-zero return, snail_last_error() says so, nothing written).  Staged through device memory of
 * the call; returns when the bytes are in the image. */
int snail_instances_render_image(SnailInstances *, const float cam[13], int resx, int resy, const float *lights7, int nLights,
                                 const float ambient[3], const float color[3], int flags, uint8_t *image_bgr, int pitch, uint64_t stats[4]);

#ifdef __cplusplus
}
#endif
#endif
