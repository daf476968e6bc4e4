/*
 * snail_bvh_fast.h -- the reference's FAST builder for plain scenes, BVH::Construct(scene, fastBuild) / BVH::FindSplit
 * (src/bvh/tree.cpp:161-287, :293-314): 16 bins on the longest axis of the node, binned SAH, std::partition, median split when a side
 * comes out empty.  It is the default of BVH::BVH (src/bvh/tree.h:13-15), what -fastRebuild selects (src/rtracer.cpp:480) and what the
 * render nodes run for lm.rebuild == 1 (src/server.cpp:305).  Two forms: on the host next to snail_bvh_build (the sweep builder), and on
 * the device from vertices in device memory into a handle that stays there and can be rebuilt in place on a stream.
 *
 * Not two builders: the node array, the permuted 64-byte triangle records and perm the device form leaves in the handle are BYTE-EQUAL to
 * snail_tris_from_verts followed by snail_bvh_build_fast on the same vertices (plain fp32 in the reference's operation order, IEEE divide
 * and sqrt, denormals kept, min / max that keep the later of two equal operands -- +0 / -0 --, libstdc++'s std::partition order, pre-order
 * node numbering with the left subtree first).
 * ONE DEVIATION, defined where the reference is undefined (the rule of snail_instances_build): the reference indexes bins[int((c - sub) *
 * mul)] unchecked.  Here a bin index that is NaN or below 0 is bin 0 and one of 16 or more is bin 15, in the binning and in the partition
 * predicate alike.  So a node of extent 0 on its longest axis (0 * inf) puts every triangle into bin 0, one side is empty and the
 * reference's median split follows.
 * CAVEAT: the equality holds for triangle boxes without NaN.  Finite vertices always give such boxes (an edge b - a that overflows is
 * +-inf, and a + inf is inf, never NaN), and non-finite vertices are refused; a node extent of inf - inf is NaN on the host and on the
 * device alike and takes the median split on both.
 * Conventions are those of snail_hip.h: 0 = success, otherwise snail_last_error() holds the message.
 */
#ifndef SNAIL_BVH_FAST_H
#define SNAIL_BVH_FAST_H
#include "snail_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The host builder; the contract of snail_bvh_build: tris64 (nTris records of snail_tris_from_verts) is permuted in place, perm[slot] =
 * input index (may be NULL), nodes32 has room for 2 * nTris records, computed under the default floating-point environment whatever the
 * caller's.  A node is a leaf at <= 4 triangles or when count * BoxSA(node) < the best binned cost.  Returns 2 when the tree is deeper than
 * SNAIL_MAX_DEPTH (the reference asserts), 1 for bad arguments. */
int snail_bvh_build_fast(void *tris64, int nTris, void *nodes32, int *nNodes, int *depth, int32_t *perm);

/* The same tree built on the device.  d_verts9 = nTris x 9 floats (three vertices per triangle) in memory of `device`; the build is
 * enqueued on `stream` and this call waits for it (creation is synchronous; snail_scene_rebuild_fast_dev is not).  The handle is a
 * SnailScene like any other: every traversal and render entry point of snail_hip.h takes it, in both arithmetics, and
 * snail_scene_download / snail_scene_info report the tree it holds (after a rebuild they wait for it).
 * d_perm (may be NULL): nTris int32, perm[slot] = caller's triangle.  d_info (may be NULL): 4 int32 {status, nNodes, depth, nTris}.
 * status: 0 ok; 1 a vertex is not finite; 2 the tree is deeper than SNAIL_MAX_DEPTH.  On status != 0 the call returns NULL and d_info
 * holds {status, 0, 0, nTris}. */
SnailScene *snail_scene_create_fast_dev(const float *d_verts9, int nTris, int device, int32_t *d_perm, int32_t *d_info, void *stream);

/* Rebuilds, in place, a handle made by snail_scene_create_fast_dev from new vertices (a deforming mesh).  nTris must be the handle's;
 * anything else, a handle of another kind or null vertices return non-zero with nothing enqueued.  Enqueued on `stream`, no host wait.
 * Ordering against launches is snail_instances_update's: the rebuild runs after everything enqueued on this handle before it, on any
 * stream, and everything enqueued after it, on any stream, sees the new tree.  The cached origin-relative node arrays are dropped (under
 * their event guards).  The vertices must stay valid until the work enqueued here has run.
 * On status != 0 the handle keeps its previous tree and records (launches after it stay safe); d_perm is then left as it was (the commit is the only writer) and d_info holds
 * {status, 0, 0, nTris}.  The host chose the handle's kernels at creation and cannot look at the new tree without waiting, so a rebuilt
 * tree must fit that choice -- besides status 1 and 2 as above:
 *   status 2 also when the tree is deeper than the handle's traversal stack takes: 62 levels, unless the handle was created deeper;
 *   status 3 when the handle was created with records the fast arithmetic paths accept (snail_scene_flags: fastOK) and a rebuilt record
 *            is outside their range (a zero-area triangle, a coordinate beyond 1e9).  A handle created without fastOK takes any finite mesh.
 * A SnailInstances handle records its BLAS root boxes at creation: a BLAS rebuilt under live instances needs
 * snail_instances_rebuild_dev afterwards (instanced launches themselves are ordered against the BLAS rebuild like any other launch).
 * Several handles in one batched pass, with these semantics per handle: snail_scenes_rebuild_fast_dev (snail_bvh_fast_batch.h). */
int snail_scene_rebuild_fast_dev(SnailScene *, const float *d_verts9, int nTris, int32_t *d_perm, int32_t *d_info, void *stream);

#ifdef __cplusplus
}
#endif
#endif
