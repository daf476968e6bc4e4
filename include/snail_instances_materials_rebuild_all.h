/*
 * snail_instances_materials_rebuild_all.h -- the per-frame step of an instanced scene whose BLASes deform on the device, in ONE call:
 * snail_instances_materials_rebuild_dev (snail_instances_materials_dynamic.h: the listed BLASes rebuilt in one batched pass, their records
 * packed again) followed by snail_instances_rebuild_dev (snail_instances_build.h: the top-level tree over the new BLAS root boxes), under one
 * set of locks, so that no launch of the handle comes between the BLAS rebuilds and the top-level rebuild.  A header of its own: every other
 * header and its symbol list stay as they are.  Plain C.
 *
 * snail_instances_materials_dynamic.h is included by no other header, so a translation unit includes it FIRST, then this one.
 *
 * Everything the call leaves behind -- every BLAS's tree, perm and records, the top-level tree, the words written to the callers' arrays -- is
 * what the two calls in a row leave.  SEMANTICS of the list (SnailBlasRebuild, the commit rule per BLAS, staleness) are
 * snail_instances_materials_rebuild_dev's; d_xf12, d_blasIdx, n, d_topPerm and d_topInfo are snail_instances_rebuild_dev's d_xf12, d_blasIdx,
 * n, d_perm and d_info.  The top-level build reads the BLAS root boxes on the stream behind the commits: a BLAS whose build was refused
 * (status 1, 2 or 3) contributes its OLD box, which is the box of the tree it keeps.
 * REFUSED with non-zero and nothing enqueued, all judged before anything is touched: the union of both functions' refusals -- nList <= 0 or a
 * null list, a blas index out of range, a BLAS that is never rebuilt, one listed twice, null vertices, a set not made by
 * snail_instances_materials_create_dev, a stale set; n <= 0, n > 1 << 30, null transforms.
 * ORDERING is the two functions'.  No host wait, except the one-off growth of the handle's buffers that snail_instances_rebuild_dev has
 * (taken before any BLAS is touched), and no allocation besides it.
 * THREADS.  Lock order: the set's render lock, the instances handle's, then the lock of every BLAS scene of the handle that was made by
 * snail_scene_create_fast_dev, in ascending BLAS index.
 * Conventions are those of snail_hip.h: 0 = success, otherwise snail_last_error() holds the message.
 */
#ifndef SNAIL_INSTANCES_MATERIALS_REBUILD_ALL_H
#define SNAIL_INSTANCES_MATERIALS_REBUILD_ALL_H
#ifndef SNAIL_INSTANCES_MATERIALS_DYNAMIC_H
#error "include snail_instances_materials_dynamic.h before snail_instances_materials_rebuild_all.h"
#endif
#include "snail_instances_build.h"

#ifdef __cplusplus
extern "C" {
#endif

int snail_instances_materials_rebuild_all_dev(SnailInstancesMaterials *, const SnailBlasRebuild *list, int nList,
                                              const float *d_xf12, const int32_t *d_blasIdx, int n, int32_t *d_topPerm, int32_t *d_topInfo, void *stream);

#ifdef __cplusplus
}
#endif
#endif
