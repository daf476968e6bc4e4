/*
 * snail_instances_materials.h -- full shading of the primary packets of a two-level instanced scene (Scene<DBVH>, snail_instances.h) on the
 * device: the gVals[6] && HasShadingData() branch of Scene::RayTrace (src/scene_trace.cpp:145-358) for a DBVH, then the lights
 * (:484-601) on those samples.  A header of its own: snail_instances.h, snail_materials.h and their symbol lists stay as they are.  Plain C.
 *
 * The reference's DBVH::HasShadingData() returns 0 with a "TODO!" (src/dbvh/tree.h:207-209), so its own renderer never takes this branch
 * for a DBVH.  Here it answers 1: that is THIS PROJECT's completion of the TODO.  Everything the branch then does is the reference's own
 * text, which it has written down for a DBVH: GetSElement (src/dbvh/tree.h:211-215) with ShTriangle::Transform (src/triangle.h:206-219),
 * GetMaterialId (:246-248), the (object, element) comparisons of Scene::RayTrace under isctFlags & fElement (src/scene_trace.cpp:162,
 * :179-182, :252-253, :263), and the instantiation of Scene<DBVH>::RayTrace (:642-659).
 *
 * NOT here (the mirrored bounce of gVals[7] is snail_instances_materials_bounce.h's, the transparency continuation
 * snail_instances_materials_transparency.h's): tile lists, 4x antialiasing and the tint, the heat-map under full shading and multi-device frames
 * of instanced scenes; routing in snail_adapter.hpp (no reference host can reach this branch through
 * HipDBVH); device-packed records for BLASes whose tree is rebuilt on the device (a set made here before such a rebuild would shade with
 * another triangle's data, so this creator refuses such a BLAS: snail_instances_materials_dynamic.h has the creator that takes it, and the
 * calls that pack its records again behind every rebuild).
 */
#ifndef SNAIL_INSTANCES_MATERIALS_H
#define SNAIL_INSTANCES_MATERIALS_H
#include "snail_instances.h"
#include "snail_materials.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the material set of an instanced scene -----------------------------------------------------------------------------------------------
 * Per BLAS of the handle (perBlas[b] belongs to the b-th scene given to snail_instances_create): shtris64 = nTris records (= that scene's
 * triangle count) in that BLAS's triId order, exactly snail_shtris_pack's bytes, and matMap [nMap] = that BLAS's BVH::GetMaterialId table.
 * A map entry is -1 (the scene's defaultMat) or an index into mats [nMats]: ONE scene-wide material list (Scene::materials) and ONE texture
 * list for all BLASes -- material identity across BLASes is observable (a block of 16 hit rays on two instances whose triangles map to the same
 * entry is shaded unmasked).  Everything is copied; the instances handle and its BLAS scenes must outlive the set.
 * REFUSED (NULL, snail_last_error() says why), before anything touches a device: nBlas different from the handle's, a BLAS whose nTris is
 * not its scene's triangle count, a record whose matId is outside its BLAS's map, a map entry outside -1 .. nMats - 1, a texture index or
 * shape that snail_materials_create refuses, and every material that could select a transparent lane, by snail_materials_create's check
 * (snail_instances_materials_transparency.h has the creator that accepts those; its sets are refused by every function below). */
typedef struct SnailBlasShading {
	const void *shtris64;
	int32_t nTris;
	const int32_t *matMap;
	int32_t nMap;
} SnailBlasShading;
typedef struct SnailInstancesMaterials SnailInstancesMaterials;
SnailInstancesMaterials *snail_instances_materials_create(SnailInstances *, const SnailBlasShading *perBlas, int nBlas, const SnailMaterial *mats, int nMats,
                                                          const SnailTexture *textures, int nTex);
void snail_instances_materials_destroy(SnailInstancesMaterials *);

/* ---- the sample stage ---------------------------------------------------------------------------------------------------------------------
 * The samples of a packet list from its hit records -- packet-major t, u, v, instance slot, triId as snail_instances_trace_packets_dev
 * writes them -- in the layout of snail_materials_shade_packets_dev: d_samples [nPackets][9][64 quads][4 lanes], 16-byte aligned.
 *   GetSElement(slot, triId): record triId of the BLAS of builder slot `slot`, through Transform with the slot's rotation rows:
 *       nrm[1] += nrm[0]; nrm[2] += nrm[0]; each of the three vectors -> (x r.x + y r.y + z r.z per row, three products added left to right,
 *       fp32, no contraction); nrm[1] -= nrm[0]; nrm[2] -= nrm[0] with the ROTATED nrm[0].  uv and matId (with its flat bit) are untouched,
 *       nothing is renormalised, the translation is not used.  The round trip is not exact in fp32: a slot with the identity rotation does
 *       not in general give the BLAS's untransformed record, and it is not shortcut.
 *   GetMaterialId(shTri.MatId(), slot): the BLAS's map entry.
 *   The three branches of snail_materials.h with every equality on the PAIR (slot, triId); a lane that missed carries (0, 0).  (a) needs all
 *   16 pairs equal: two instances of one BLAS hit at the same triId are not a single triangle, such a block takes (b) (the (a + b bx) + c by
 *   association, texDiff = 0, mip 0).  The "triId 0" quirk becomes the (slot 0, triId 0) quirk: in a quad whose lane 0 missed, a lane that hit
 *   slot 0's triangle 0 keeps the default material and zero normal / texCoord.
 * Material kinds, PointSampler::Sample, the mip choice and the values of lanes that missed are those of snail_materials_shade_packets_dev.
 * The instance records are read at launch: after snail_instances_update / _rebuild_dev the same set shades with the new rotations.
 * A hit lane's slot or triId outside the scene (a lane that missed carries (0, 0) whatever it holds):
 *   the slot is clamped to [0, capacity - 1], capacity = the instance records the handle has room for.  That is the instance count unless an
 *       update shrank it; a slot between the two reads a stale record.
 *   the triId is clamped below to 0.  The block and quad comparisons and the quirk are taken on (clamped slot, lower-clamped triId): the
 *       triId's upper bound is its BLAS's nTris, which needs the slot's record, and the comparisons come before any record is read.
 *   the record read is that of min(triId, nTris - 1) of the slot's BLAS.  Two hit lanes of one slot with triIds nTris + 7 and nTris + 9 read
 *       the same record and still do not count as a single triangle.
 * These clamps keep a corrupted hit record from turning into an address; a traversal never produces such records.
 * The barycentric deviation of snail_instances.h (u / v stored at the hit's own quad) is inherited. */
int snail_instances_materials_shade_packets_dev(SnailInstancesMaterials *, const float cam[13], int resx, int resy, const int32_t *d_packet_xy, int nPackets,
                                                const float *d_t, const float *d_u, const float *d_v, const int32_t *d_inst, const int32_t *d_triId,
                                                float *d_samples, void *stream);

/* ---- lit frames ---------------------------------------------------------------------------------------------------------------------------
 * DBVH::TraversePrimary of the primary packets -> samples -> per light the packet-level cull and Scene::TraceLight on the samples'
 * interpolated, rotated normals with DBVH::TraverseShadow -> outColor = diffuse * lDiffuse + specular * lSpecular -> ConvColor -> B,G,R.
 * Conventions of snail_render_materials_dev / _packets_dev / _image and of snail_instances_shade.h: 0 = success; lights7 a HOST pointer to
 * 0..SNAIL_MAX_LIGHTS x {pos[3], color[3], radius}; the store rule of snail_hip.h; d_stats / stats += {intersects, iterations, traced rays,
 * skips} = the primary walk's counters plus each non-culled light's shadow walk, rays = primary rays + shadow lanes with N.L > 0; both
 * arithmetics (the BLAS scenes'), table look-ups in their fully checked form.  flags: must be 0.  Intermediates live in the set, 8 launches in
 * flight, each guarded by an event, and a whole frame's packet list cached by packet-grid size; launches are ordered against
 * snail_instances_update and snail_instances_rebuild_dev as the handle's other launches are. */
int snail_instances_render_materials_dev(SnailInstancesMaterials *, const float cam[13], int resx, int resy, const float *lights7, int nLights,
                                         const float ambient[3], int flags, uint8_t *d_frame_bgr, int pitch, uint64_t *d_stats, void *stream);
int snail_instances_render_materials_packets_dev(SnailInstancesMaterials *, const float cam[13], int resx, int resy, const int32_t *d_packet_xy, int nPackets,
                                                 const float *lights7, int nLights, const float ambient[3], int flags, uint8_t *d_bgr_packets,
                                                 uint64_t *d_stats, void *stream);
int snail_instances_render_materials_image(SnailInstancesMaterials *, const float cam[13], int resx, int resy, const float *lights7, int nLights,
                                           const float ambient[3], int flags, uint8_t *image_bgr, int pitch, uint64_t stats[4]);

#ifdef __cplusplus
}
#endif
#endif
