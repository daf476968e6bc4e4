/*
 * snail_bvh_fast_batch.h -- snail_scene_rebuild_fast_dev (snail_bvh_fast.h) for SEVERAL handles in one batched pass on the device.  An
 * animated scene of many small deforming meshes rebuilds every one of them per frame; one rebuild is a chain of about 35 dependent launches,
 * most of them a few workgroups over a small mesh, and k rebuilds in a row pay that chain k times.  This call enqueues the chain ONCE for up
 * to 16 handles (a longer list takes several passes of 16): every phase is one launch whose workgroups are dealt to the handles.  A header of
 * its own: every other header and its symbol list stay as they are.  Plain C.
 *
 * Not another builder: each listed handle ends BYTE-EQUAL -- nodes, triangle records, perm, info words -- to snail_scene_rebuild_fast_dev on
 * that handle with the same vertices (the kernels call the same code per tree; the result of a build does not depend on which workgroup did
 * what), and so to snail_tris_from_verts + snail_bvh_build_fast on the host.
 *
 * SEMANTICS are snail_scene_rebuild_fast_dev's, PER ENTRY: status 1 / 2 / 3 by that handle's own rules (its depth limit, its fastOK), the
 * commit rule (on status != 0 the handle keeps its previous tree and records, d_perm is left as it was and d_info holds
 * {status, 0, 0, nTris}; the other entries commit), the cached origin-relative node arrays are dropped, and the handle's count of rebuilds
 * (what the material sets of snail_materials_dynamic.h compare) goes up by one.
 * ORDERING, per listed handle: the stream waits for every launch enqueued on that handle before the call, on any stream, and for its previous
 * rebuild; everything enqueued on the handle after the call, on any stream, sees the new tree.  No host wait, no allocation on the device.
 * The vertices must stay valid until the work enqueued here has run.
 * REFUSED with non-zero and NOTHING enqueued, the whole list judged before any handle is touched (snail_last_error() names the entry): a null
 * list, nList <= 0, a null handle or null vertices, a handle not made by snail_scene_create_fast_dev, nTris other than the handle's, a handle
 * listed twice, handles on different devices.
 * THREADS.  The handles' locks are taken in address order (snail_render_tiles_multi's rule), whatever the order of the list.  The calls of
 * snail_instances_materials_dynamic.h take their BLAS scenes' locks in ascending BLAS index instead: a thread in this call and a thread in one of
 * those, over the same scenes, must not run at the same time unless the handle's BLAS order is its address order.
 * NOT here: batches over several devices.  BLASes of an instanced material set go through snail_instances_materials_rebuild_dev
 * (snail_instances_materials_dynamic.h), which uses the same pass and keeps the set's records in step.
 * Conventions are those of snail_hip.h: 0 = success, otherwise snail_last_error() holds the message.
 */
#ifndef SNAIL_BVH_FAST_BATCH_H
#define SNAIL_BVH_FAST_BATCH_H
#include "snail_bvh_fast.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One handle of the list: the arguments of snail_scene_rebuild_fast_dev.  d_perm (nTris int32) and d_info (4 int32) may be NULL. */
typedef struct { SnailScene *scene; const float *d_verts9; int32_t nTris; int32_t *d_perm; int32_t *d_info; } SnailFastRebuild;

int snail_scenes_rebuild_fast_dev(const SnailFastRebuild *list, int nList, void *stream);

#ifdef __cplusplus
}
#endif
#endif
