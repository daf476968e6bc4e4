/*
 * snail_instances.h -- C-ABI of libsnailhip.so for two-level instanced scenes: the second model of the reference's AccStruct concept,
 * DBVH (src/dbvh/tree.h, tree.cpp, traverse.cpp), on top of the SnailScene handles of snail_hip.h (whose conventions -- status codes,
 * snail_last_error(), `*_dev` entry points on device pointers and a stream, Context / ShadowContext layouts -- hold here as well).
 */
#ifndef SNAIL_INSTANCES_H
#define SNAIL_INSTANCES_H
#include "snail_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- two-level instanced scenes: the second model of the AccStruct concept, DBVH (src/dbvh/tree.h, tree.cpp, traverse.cpp) ------------
 * A top-level tree over rigid instances; each instance = rotation rows r0, r1, r2, a translation t and one BLAS (bottom-level tree = an
 * ordinary SnailScene).  xf12 = n x {r0.xyz, r1.xyz, r2.xyz, t.xyz}; world = R * object + t (ObjectInstance::TransformPoint, tree.h:28-32).
 *
 * Build (host, snail_instances_build; DBVH::Construct / FindSplit, tree.cpp:23-172):
 *   - instance box = ObjectInstance::ComputeBBox (tree.cpp:4-21) over the BLAS root box (blasBBox6 = nBlas x {min.xyz, max.xyz}):
 *     y*r.y + z*r.z, then x*r.x added, min / max over the 8 corners, then + t;
 *   - split axis = MaxAxis of the node box; binned SAH with 8 bins when count < 8, else 16; mul = nBins*(1 - 0.0001f)/extent,
 *     bin = int((c - sub)*mul); cost = BoxSA(left)*nLeft + BoxSA(right)*nRight as written (empty sides cost 0); leaf when count <= 1
 *     or count*BoxSA(node) < min cost; the elements are partitioned by std::partition with the TestBoxes predicate in the order that
 *     libstdc++'s bidirectional __partition produces (swap from both ends); a side left empty -> median split; firstNode = the second
 *     assignment of tree.cpp:141-143 only; depth <= SNAIL_INSTANCES_MAX_DEPTH (DBVH::maxDepth = 64) or an error.
 *   - DEVIATION (defined where the reference is undefined): a bin index that is NaN or < 0 is 0 and one past the last bin is the last bin,
 *     so coincident centres (extent 0: 0 * inf) all fall in bin 0 and take the median split.
 *   - nodes32: the 32-byte DBVH::Node (the BVH record: box, sub / first | 0x80000000, axis | firstNode << 16 / count); capacity 2n.
 *     perm[slot] = the caller's instance at builder slot `slot`; the id a hit reports is that SLOT (DBVH::elements order).
 *   - non-finite transforms or boxes and BLAS indices outside [0, nBlas) are errors.
 *
 * Traversal (one wave per packet; DBVH::TraversePrimary0 / TraverseShadow0, traverse.cpp:14-134 -- TraversePrimary returns
 * TraversePrimary0(c) at once, :136-138, so the split code after it does not exist here):
 *   - stack of maxDepth + 2 (node, firstActive, lastActive); child order firstNode ^ sign[axis], sign from Dir(0) lane 0; every popped
 *     node counts one LoopIteration; BBox::TestInterval over RayInterval(c.rays) (no distances, also for shadows) before BBox::Test,
 *     on leaves too; a leaf whose box passed counts Intersection(last - first + 1) per instance whatever the inner walk does;
 *   - an instance leaf (ObjectInstance::CollidePrimary / CollideShadow, tree.h:47-175): the active quads first..last are transformed
 *     with ITransformVec / ITransformPoint (origin - t, then R^T, left to right, no contraction), idir = SafeInv(dir) = Inv(dir + 1e-8)
 *     in the handle's arithmetic, and BVH::TraversePrimary / TraverseShadow runs on a RayGroup of exactly count = last - first + 1 quads
 *     with distance + first (so its RayInterval, ranges and TreeStats are those of a count-quad packet; it runs in the exact mode of the
 *     generic walk).  A hit inside the instance (objects[n] != ~0) writes object = instance slot, element = triId;
 *   - DEVIATION: the reference passes c.barycentric without + firstActive (tree.h:73), so u / v of inner quad n would land on outer
 *     quad n; here they are stored at the hit's own quad first + n;
 *   - shadows: shared origin only, no early out at the top level; occluded lanes end at -inf as for a BVH.
 * Layouts are the Context / ShadowContext layouts of snail_trace_rays / snail_trace_shadow; `object` receives the instance slot and
 * `element` the triId (both IN/OUT: lanes without a hit keep the caller's values); bary may be NULL.  A primary frame's miss is
 * (t = +inf, u = v = 0, instance = 0, triId = 0), as for snail_trace_primary.
 * The arithmetic is the BLAS scenes' (snail_scene_set_arith) at the launch; BLASes in different arithmetics are an error.
 * Concurrency: as for SnailScene -- any number of host threads may use one handle at once; snail_instances_update is ordered on its
 * stream after every launch enqueued before it (on any stream) and before every launch enqueued after it. */
#define SNAIL_INSTANCES_MAX_DEPTH 64
typedef struct SnailInstances SnailInstances;
int snail_instances_build(const float *xf12, const int32_t *blasIdx, int n, const float *blasBBox6, int nBlas, void *nodes32,
                          int *nNodes, int *depth, int32_t *perm);
/* A tree that is already built (the reference's own DBVH::nodes, or snail_instances_build's), with xf12 / blasIdx in builder-slot order.
 * Validated before any kernel can read it: children inside the array and after their parent, leaf ranges inside [0, n),
 * depth <= 64 (measured, not taken from `depth`), finite transforms, BLAS indices in range, all BLASes on one device.  The node boxes are
 * not checked: a non-finite box only makes its box test fail, as in the reference.
 * Lifetime: the handle keeps the BLAS scenes' device records, not copies -- every SnailScene in `blas` must outlive the SnailInstances
 * handle (destroy the instances first), and the BLAS list is fixed for the handle's life (snail_instances_update changes transforms,
 * BLAS indices and the tree only). */
SnailInstances *snail_instances_create(SnailScene *const *blas, int nBlas, const void *nodes32, int nNodes, const float *xf12,
                                       const int32_t *blasIdx, int n, int depth);
int snail_instances_update(SnailInstances *, const void *nodes32, int nNodes, const float *xf12, const int32_t *blasIdx, int n, int depth,
                           void *stream);
void snail_instances_destroy(SnailInstances *);
/* Primary frame: the packets, layout and TracingRays accounting of snail_trace_primary_dev; d_inst = instance slot. */
int snail_instances_trace_primary_dev(SnailInstances *, const float cam[13], int resx, int resy, int x0, int y0, int w, int h, float *d_t,
                                      float *d_u, float *d_v, int32_t *d_inst, int32_t *d_triId, uint64_t *d_stats, void *stream);
/* ... over an explicit packet list (int2 (x, y) pixel origins), packet-major [nPackets][256] outputs (for snail_shade_depth_dev). */
int snail_instances_trace_packets_dev(SnailInstances *, const float cam[13], int resx, int resy, const int32_t *d_packetXY, int nPackets,
                                      float *d_t, float *d_u, float *d_v, int32_t *d_inst, int32_t *d_triId, uint64_t *d_stats, void *stream);
int snail_instances_trace_rays_dev(SnailInstances *, int nPackets, int size, int sharedOrigin, const float *d_origin, const float *d_dir,
                                   const float *d_idir, const uint8_t *d_mask, float *d_distance, int32_t *d_object, int32_t *d_element,
                                   float *d_bary, uint64_t *d_stats, void *stream);
int snail_instances_trace_shadow_dev(SnailInstances *, int nPackets, int size, const float *d_origin3, const float *d_dir, const float *d_idir,
                                     float *d_distance, uint64_t *d_stats, void *stream);
/* host-pointer forms: staged through device memory of the call, return when the results are in the host buffers */
/* The whole frame's primary packets (row-major over the 16x16 packet grid, packet-major records [packet][256]: the reference's quad order)
 * into host buffers of pw*ph*256 entries each; stats[4] += the frame's TreeStats.  The frame prefetch of the C++ adapter (HipDBVH). */
int snail_instances_trace_frame_packets(SnailInstances *, const float cam[13], int resx, int resy, float *t, float *u, float *v,
                                        int32_t *inst, int32_t *triId, uint64_t stats[4]);
/* The gVals[1] depth-shaded frame (src/scene_trace.cpp:128-137, ConvColor of src/render.cpp:11-17) into a host image of 3 bytes (B, G, R)
 * per pixel and `pitch` bytes per row, in the BLASes' arithmetic; stats[4] += the frame's TreeStats. */
int snail_instances_render_depth(SnailInstances *, const float cam[13], int resx, int resy, uint8_t *image, int pitch, uint64_t stats[4]);
int snail_instances_trace_rays(SnailInstances *, int nPackets, int size, int sharedOrigin, const float *origin, const float *dir,
                               const float *idir, const uint8_t *mask, float *distance, int32_t *object, int32_t *element, float *bary,
                               uint64_t stats[4]);
int snail_instances_trace_shadow(SnailInstances *, int nPackets, int size, const float *origin3, const float *dir, const float *idir,
                                 float *distance, uint64_t stats[4]);

#ifdef __cplusplus
}
#endif
/* lit frames of instanced scenes (lights, shadow packets, one mirrored bounce): declared in a header of their own, part of this one */
#include "snail_instances_shade.h"
/* the tile renderer of instanced scenes (tile list with planar store, 4x antialiasing, rank tint): likewise */
#include "snail_instances_tiles.h"
/* the top-level tree rebuilt on the device from transforms in device memory, byte-equal to the host builder's: likewise */
#include "snail_instances_build.h"
#endif
