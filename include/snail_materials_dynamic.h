/*
 * snail_materials_dynamic.h -- full shading of a DEFORMING mesh: a material set over a handle of snail_scene_create_fast_dev
 * (include/snail_bvh_fast.h) whose 64-byte ShTriangle records are written ON THE DEVICE, in triId order, from input-order data in device
 * memory, and written again on the rebuild's stream whenever the tree is rebuilt.  The reference's builder permutes shTris together with tris
 * (src/bvh/tree.cpp:122-125, :249-252) and Scene::RayTrace indexes shTris[triId]; a set of snail_materials_create is permuted once, on the
 * host, and describes one tree only.  A header of its own: snail_hip.h, the other snail_materials_*.h headers and their symbol lists stay as
 * they are.  Plain C.
 *
 * A set made here is a SnailMaterials like any other: every frame, tile, bounce and transparency entry point of snail_materials.h,
 * _bounce.h, _tiles.h, _transparency.h and _tree.h takes it, in both arithmetics, and snail_materials_destroy frees it.
 *
 * RECORDS.  The bytes are snail_shtris_pack's: uv[0], uv[1] - uv[0], uv[2] - uv[0]; nrm[0], nrm[1] - nrm[0], nrm[2] - nrm[0];
 * matIdx | flat << 31 -- every difference rounded separately in fp32; record i comes from input triangle perm[i].  The arithmetic is plain
 * fp32 whatever the scene's arithmetic mode (no FMA contraction, IEEE divide and square root, denormals kept).
 * FACE NORMALS (d_nrm9 == NULL): BaseScene::Object::GetTriangle for a triangle without vn (src/base_scene.cpp:313-318) from d_verts9:
 * fnrm = (p1 - p0) ^ (p2 - p0); fnrm *= RSqrt(fnrm | fnrm) with veclib's scalar definitions (veclib/vec3.h:92-106, sums left to right;
 * RSqrt(v) = 1.0f / Sqrt(v), veclib/vecbase.h:56).  All three vertex normals are fnrm; the flat bit stays what d_flat says.
 * ONE DEVIATION.  The sample kernels presuppose finite normals and snail_shtris_pack refuses others, but a re-pack that runs behind a
 * rebuild on a stream cannot refuse one triangle without leaving the set inconsistent with its tree.  So a triangle with ANY non-finite
 * normal component -- given, or the face normal of a zero-area triangle (0 * inf) -- gets three zero normals and is counted in
 * zeroedTriangles.  A zero normal is what the sample stage uses for lanes that missed.  (A perm entry outside 0..nTris-1, which no tree of
 * this library produces, reads nothing: its record is all zero and counted as well.)
 *
 * COMMIT RULE.  snail_materials_rebuild_dev commits the records only when the build committed the tree (status 0): the device decides, on
 * the stream, from the build's own status word.  Tree and records therefore always match, and a refused rebuild leaves both as they were.
 * STALENESS.  The scene counts the rebuilds enqueued on it; the set remembers the count its records match.  snail_materials_rebuild_dev and
 * snail_materials_update_dev bring the two together.  Every entry point that takes a set refuses one whose count differs from its scene's
 * -- a snail_scene_rebuild_fast_dev behind its back, or snail_materials_rebuild_dev through another set of the same scene -- with non-zero
 * and a text that names the rebuild, before anything is enqueued.  Sets of the two other creators get no such refusal and behave as before.
 * ORDERING is snail_scene_rebuild_fast_dev's: a re-pack runs after every launch enqueued on the handle before it, on any stream, and after
 * the previous rebuild; every launch enqueued after it, on any stream, waits for it.  No call here waits on the host except the creator.
 *
 * Conventions are those of snail_hip.h: 0 = success, otherwise snail_last_error() holds the message and nothing was enqueued.
 * NOT here: smooth normals averaged over shared vertices (the caller supplies them through d_nrm9, as the reference takes them from vn);
 * changing uv or the material assignment after creation; instanced scenes (snail_instances_materials_dynamic.h has them: the same records
 * per BLAS, several BLASes packed in one launch); OBJ / MTL ingest.
 */
#ifndef SNAIL_MATERIALS_DYNAMIC_H
#define SNAIL_MATERIALS_DYNAMIC_H
#include "snail_materials_transparency.h"
#include "snail_bvh_fast.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The set of a handle of snail_scene_create_fast_dev (anything else is refused).  d_uv6 [n][3][2], d_matIdx [n], d_flat [n] (or NULL: none
 * flat) describe the INPUT triangles in the order the scene's vertices came in; device pointers on the scene's device, copied into the set.
 * d_perm [n]: the perm of the tree the handle holds now, as snail_scene_create_fast_dev / _rebuild_fast_dev wrote it.  Normals: d_nrm9
 * [n][3][3] per vertex in input order, or NULL for face normals from d_verts9 [n][3][3] (one of the two must be given).  matMap, mats,
 * textures: HOST pointers with the meaning of snail_materials_create; opacityTexture == NULL gives that creator's kinds and refusals,
 * non-NULL snail_materials_create_transparent's.  The host data is judged first, before a device is touched; then, on the device, what
 * snail_shtris_pack and the creators judge on the host: uv finite and |uv| < 2^20, 0 <= matIdx < nMap (and 0 <= perm < nTris).  Synchronous
 * (the records are packed on `stream` and waited for).  NULL with a snail_last_error() text on refusal, before any record is written. */
SnailMaterials *snail_materials_create_dev(SnailScene *scene, const float *d_uv6, const int32_t *d_matIdx, const uint8_t *d_flat, int nTris,
                                           const int32_t *d_perm, const float *d_nrm9, const float *d_verts9, const int32_t *matMap, int nMap,
                                           const SnailMaterial *mats, int nMats, const int32_t *opacityTexture, const SnailTexture *textures,
                                           int nTex, void *stream);

/* Rebuilds the set's scene from d_verts9 exactly as snail_scene_rebuild_fast_dev does (its kernels, status rules and ordering) and then, on
 * the same stream, packs the records again through the new permutation -- with d_nrm9, or with face normals of d_verts9 when it is NULL --
 * under the commit rule above.  d_perm (or NULL) receives the perm of the tree the handle holds after the call: the new one on status 0, the
 * previous one otherwise.  d_info (or NULL): 6 int32, the rebuild's {status, nNodes, depth, nTris}, then {recordsCommitted (0 / 1),
 * zeroedTriangles}.  No host wait; the arrays must stay valid until the work enqueued here has run.  A stale set is refused here too
 * (snail_materials_update_dev first): were its build then refused, nothing would bring its records back to the tree the handle keeps. */
int snail_materials_rebuild_dev(SnailMaterials *, const float *d_verts9, const float *d_nrm9, int32_t *d_perm, int32_t *d_info, void *stream);

/* Packs the records again, and nothing else: for a set whose scene was rebuilt by someone else (snail_scene_rebuild_fast_dev, or another
 * set of the same scene), or for new normals alone.  d_perm is the caller's statement of the current tree's perm; normals as above (d_nrm9,
 * or NULL and d_verts9).  d_info2 (or NULL): 2 int32 {1, zeroedTriangles}.  Always commits.  No host wait. */
int snail_materials_update_dev(SnailMaterials *, const int32_t *d_perm, const float *d_nrm9, const float *d_verts9, int32_t *d_info2,
                               void *stream);

#ifdef __cplusplus
}
#endif
#endif
