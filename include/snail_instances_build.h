/*
 * snail_instances_build.h -- the top-level tree of the two-level instanced scenes of snail_instances.h, rebuilt ON THE DEVICE: the device form
 * of DBVH::Construct / FindSplit (src/dbvh/tree.cpp:23-172), which the reference's instanced mode runs before every frame
 * (src/rtracer.cpp:146-178, :359-386; src/node.cpp:326-338).  Part of snail_instances.h, which includes this file last.
 *
 * Not a second builder: the nodes, the element order and the instance records it leaves in the handle are BYTE-EQUAL to what
 * snail_instances_build followed by snail_instances_update leaves (plain fp32 in the host builder's operation order, IEEE division,
 * denormals kept, min / max that keep the later of two equal operands -- +0 / -0 --, libstdc++'s std::partition order, the host's node
 * numbering), so every frame rendered after it equals the host path's.  It does not depend on the BLAS scenes' arithmetic.
 * CAVEAT: the equality holds for instance boxes without NaN.  Finite transforms over finite BLAS boxes give such boxes unless a product
 * overflows to inf - inf; such an input passes validation (as it passes the host builder's) and builds a tree that is safe to traverse, but
 * whose bytes may differ from the host's, which folds NaN through its min / max in element order.
 * Conventions are those of snail_instances.h: 0 = success, otherwise snail_last_error() holds the message.
 */
#ifndef SNAIL_INSTANCES_BUILD_H
#define SNAIL_INSTANCES_BUILD_H
#include "snail_instances.h"

#ifdef __cplusplus
extern "C" {
#endif

/* DBVH::Construct on the device.  d_xf12 = n x 12 floats, d_blasIdx = n int32 (NULL: all 0), both in the CALLER's instance order, in device
 * memory of the handle's GPU.  Enqueued on `stream`; ordered against launches exactly as snail_instances_update is.  No host wait, except
 * the one-off growth of the handle's buffers that snail_instances_update also has.  The BLAS root boxes are those of the handle's BLAS
 * scenes at snail_instances_create.  The inputs must stay valid until the work enqueued here has run.
 * d_perm (may be NULL): n int32, perm[slot] = caller's instance.
 * d_info (may be NULL): 4 int32 {status, nNodes, depth, n}.
 * status: 0 ok; 1 non-finite transform or BLAS index outside [0, nBlas); 2 tree deeper than SNAIL_INSTANCES_MAX_DEPTH.
 * On status != 0 the handle keeps its previous tree and records untouched (launches after it stay safe); d_perm is then unspecified and
 * d_info holds {status, 0, 0, n}.
 * Returns non-zero, with nothing enqueued, for a null handle, n <= 0, n > 1 << 30 or a null d_xf12. */
int snail_instances_rebuild_dev(SnailInstances *, const float *d_xf12, const int32_t *d_blasIdx, int n,
                                int32_t *d_perm, int32_t *d_info, void *stream);
/* Synchronous read-back of what the handle holds now (after every update / rebuild enqueued so far): for tests, and for hosts that want the tree.
 * nodes32 (nodeCap records), xf12_slots and blasIdx_slots (slotCap instances, builder-slot order) may each be NULL; a capacity that is too
 * small is an error.  *nNodes and *n (may be NULL) are set whenever the handle is valid. */
int snail_instances_read_tree(SnailInstances *, void *nodes32, int nodeCap, int *nNodes, float *xf12_slots,
                              int32_t *blasIdx_slots, int slotCap, int *n);

#ifdef __cplusplus
}
#endif
#endif
