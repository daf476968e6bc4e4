/*
 * snail_instances_materials_dynamic.h -- full shading of an instanced scene whose BLASes DEFORM on the device: a material set of an instances
 * handle (snail_instances.h) in which the records of every BLAS made by snail_scene_create_fast_dev (snail_bvh_fast.h) are written ON THE
 * DEVICE, in triId order, and written again behind every rebuild of that BLAS -- what snail_materials_dynamic.h does for a plain scene, per
 * BLAS.  BLASes built from host triangles keep their host-packed records, as in snail_instances_materials.h.  A header of its own: every other
 * header and its symbol list stay as they are.  Plain C.
 *
 * A set made here is a SnailInstancesMaterials like any other: every entry point of snail_instances_materials.h, _bounce.h, _transparency.h,
 * _tree.h and _heatmap.h takes it, in both arithmetics, and snail_instances_materials_destroy frees it.
 *
 * RECORDS, FACE NORMALS and the ONE DEVIATION (a triangle with a non-finite normal component gets three zero normals and is counted in
 * zeroedTriangles) are those of snail_materials_dynamic.h: snail_shtris_pack's bytes through the perm of the tree the BLAS holds, plain fp32
 * whatever the arithmetic mode.
 *
 * COMMIT RULE, per BLAS.  snail_instances_materials_rebuild_dev commits a BLAS's records only when that BLAS's build committed its tree
 * (status 0); the device decides, on the stream, from each build's own status word.  A BLAS whose build is refused keeps its tree, its perm and
 * its records; the other BLASes of the same call commit.
 * STALENESS.  Every BLAS scene counts the rebuilds enqueued on it; the set remembers, per dynamic BLAS, the count its records match.  Every
 * function of the snail_instances_materials*.h headers that takes a set refuses one in which a count differs from its scene's -- after a
 * snail_scene_rebuild_fast_dev behind its back, or a rebuild through a snail_materials_create_dev set or another instanced set that shares
 * the BLAS scene -- with non-zero and a text that names the rebuild, before anything is enqueued; snail_instances_materials_update_dev with
 * the current perm brings the set up to date.  Sets of snail_instances_materials_create / _create_transparent hold no dynamic BLAS and behave
 * as before.
 * ORDERING is snail_scene_rebuild_fast_dev's, per listed BLAS: the stream waits for every launch enqueued before the call that reads the BLAS
 * scene, on any stream and through any handle, and for its previous rebuild; every instanced launch enqueued after the call, on any stream,
 * waits for the pack.  Neither call waits on the host, and neither allocates.
 * THE TOP-LEVEL TREE is NOT touched by either call.  A rebuilt BLAS has a new root box, so the caller follows with
 * snail_instances_rebuild_dev (snail_instances_build.h) or snail_instances_update, as snail_instances.h asks after a BLAS rebuild, before the
 * next frame.  The per-frame sequence: snail_instances_materials_rebuild_dev, snail_instances_rebuild_dev, then any frame function.
 * THREADS.  Lock order: the set's render lock, the instances handle's, then the listed BLAS scenes' in ascending BLAS index.
 *
 * Conventions are those of snail_hip.h: 0 = success, otherwise snail_last_error() holds the message and nothing was enqueued -- except that
 * a HIP error in the middle of a list leaves the BLASes rebuilt before it stale (an _update_dev brings them back).
 * NOT here: a snail::HipDBVH route in snail_adapter.hpp (no reference host reaches the branch); changing uv or the material assignment after
 * creation.  The one call that rebuilds BLASes and the top-level tree is snail_instances_materials_rebuild_all.h's.
 */
#ifndef SNAIL_INSTANCES_MATERIALS_DYNAMIC_H
#define SNAIL_INSTANCES_MATERIALS_DYNAMIC_H
#include "snail_instances_materials_transparency.h"
#include "snail_bvh_fast.h"

#ifdef __cplusplus
extern "C" {
#endif

/* perBlas[b] of snail_instances_materials_create_dev.
 * A BLAS that is never rebuilt: exactly SnailBlasShading's four fields (HOST pointers), the six device pointers NULL.
 * A BLAS of snail_scene_create_fast_dev: shtris64 NULL; nTris, matMap (HOST pointer), nMap as above; and DEVICE pointers with the meaning they
 * have in snail_materials_create_dev, describing the INPUT triangles in the order the scene's vertices came in: d_uv6 [n][3][2], d_matIdx [n],
 * d_flat [n] (or NULL: none flat), d_perm [n] (the perm of the tree the BLAS holds now), d_nrm9 [n][3][3] or NULL for face normals from
 * d_verts9 [n][3][3] (one of the two must be given).  uv, matIdx and flat are copied into the set. */
typedef struct {
	const void *shtris64; int32_t nTris; const int32_t *matMap; int32_t nMap;
	const float *d_uv6; const int32_t *d_matIdx; const uint8_t *d_flat; const int32_t *d_perm; const float *d_nrm9; const float *d_verts9;
} SnailBlasShadingDev;

/* One BLAS of a rebuild or update list.  blas: its index in the handle, a BLAS of snail_scene_create_fast_dev.  d_verts9 / d_nrm9 [n][3][3]
 * in input order (d_nrm9 NULL: face normals of d_verts9).
 *   _rebuild_dev: d_verts9 are the new vertices (required).  d_perm (or NULL) RECEIVES the perm of the tree the BLAS holds after the call: the
 *       new one on status 0, the previous one otherwise.  d_info (or NULL): 6 int32, the build's {status, nNodes, depth, nTris}, then
 *       {recordsCommitted (0 / 1), zeroedTriangles}.
 *   _update_dev: d_perm is the caller's STATEMENT of the BLAS's current perm (required; read, not written); one of d_nrm9 / d_verts9 is
 *       required.  d_info (or NULL): 2 int32 {1, zeroedTriangles}.
 * The arrays must stay valid until the work enqueued by the call has run. */
typedef struct { int32_t blas; const float *d_verts9; const float *d_nrm9; int32_t *d_perm; int32_t *d_info; } SnailBlasRebuild;

/* The set.  mats, textures, opacityTexture: HOST pointers with the meaning of snail_instances_materials_create (opacityTexture == NULL: that
 * creator's kinds and refusals; non-NULL: snail_instances_materials_create_transparent's).  All host data is judged first, per BLAS, by
 * snail_materials_create's check; then the device data of every dynamic BLAS is judged on the device (uv finite and |uv| < 2^20,
 * 0 <= matIdx < nMap, 0 <= perm < nTris); all before any record is written.  REFUSED besides (NULL, snail_last_error() names the BLAS): a BLAS
 * of snail_scene_create_fast_dev given host records, a host-built BLAS given device data.  Synchronous: the records are packed on `stream`
 * (all dynamic BLASes in one launch) and waited for. */
SnailInstancesMaterials *snail_instances_materials_create_dev(SnailInstances *, const SnailBlasShadingDev *perBlas, int nBlas, const SnailMaterial *mats, int nMats,
                                                              const int32_t *opacityTexture, const SnailTexture *textures, int nTex, void *stream);

/* Rebuilds every listed BLAS from its d_verts9 with the results, status rules and ordering of snail_scene_rebuild_fast_dev -- all listed builds
 * in ONE batched pass, snail_scenes_rebuild_fast_dev's (snail_bvh_fast_batch.h): each phase of the build is one launch for all of them, and every
 * BLAS ends byte-equal to a rebuild of its own --, perm and status going into the set's own words for that BLAS, and then packs the records of ALL listed BLASes again in one launch on the same stream,
 * under the commit rule above.  REFUSED before anything is enqueued: nList <= 0, a blas index out of range, one that names a BLAS that is never
 * rebuilt, one listed twice, null vertices, a set that was not made by snail_instances_materials_create_dev, and a STALE set
 * (snail_instances_materials_update_dev first: were a build then refused, nothing would bring its records back to the tree the BLAS keeps).
 * No host wait. */
int snail_instances_materials_rebuild_dev(SnailInstancesMaterials *, const SnailBlasRebuild *list, int nList, void *stream);

/* Packs the records of the listed BLASes again, and nothing else: for BLASes rebuilt by someone else, or for new normals alone.  Always
 * commits.  The same refusals except the null vertices and the stale set; a null perm, and neither normals nor vertices, are refused instead.
 * No host wait. */
int snail_instances_materials_update_dev(SnailInstancesMaterials *, const SnailBlasRebuild *list, int nList, void *stream);

#ifdef __cplusplus
}
#endif
#endif
