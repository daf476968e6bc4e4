/*
 * snail_wide.h -- rays that form no packets: BVH::WideTrace (src/bvh/traverse.cpp:197-225) with ONE RAY PER LANE, and the photon pass of
 * TracePhotons (src/photons.cpp:197-250) on top of it.  Every other walk of this library is a packet walk -- one 16x16 packet per
 * wavefront, every visit testing all 64 quads; a host with scattered rays (photons from a light, occlusion probes, any list of
 * independent queries) would pad them into 256-ray groups and every group would visit the union of its rays' paths.  A header of its own:
 * every other header and its symbol list stay as they are.  Plain C.
 *
 * THE WALK, per ray r (the reference's index lists only batch rays; for one ray its recursion is fixed, so each ray's result and visit
 * counts are the reference's, whatever the other rays do):
 *   - start at startNode WITHOUT testing that node's box;
 *   - leaf: for t = 0 .. count - 1 in order, d = Collide0(tris[first + t]); dist = dist < d ? dist : d (the select: a NaN d replaces
 *     dist, a NaN dist is replaced by the next d);
 *   - inner node with children c, c + 1: if WideTest(box[c], dist) passes, walk c to its end; then, if WideTest(box[c + 1], dist) passes
 *     with the distance as it is THEN, walk c + 1.  The left child always first; axis / firstNode are not used.
 *   WideTest (src/bounding_box.cpp:258-326), per axis x, y, z: l1 = idir * (bmin - o), l2 = idir * (bmax - o); lmin = Max(Min(l1, l2), lmin),
 *   lmax = Min(Max(l1, l2), lmax); passes when lmax >= 0 && lmin <= Min(lmax, dist).  Min(a, b) = a < b ? a : b, Max(a, b) = a > b ? a : b:
 *   the second operand on NaN and on +-0 (minps / maxps, and the scalar tail alike).
 *   Collide0 = Triangle::Collide<0> (src/triangle.h:139-164): edges (ba + a) - a and (ca + a) - a -- recomputed, not the stored ba / ca --,
 *   normal = their cross product times 1 / its length (the stored plane / t0 are not read), det = dir . n, tvec = o - a, u = dir . (ba' x
 *   tvec), v = dir . (tvec x ca'); the distance -(tvec . n) / det where Min(u, v) >= 0 && u + v <= det * t0, else +inf.  THERE IS NO
 *   t > 0 TEST: a triangle behind the origin in a visited leaf gives a negative distance and the select keeps it.
 *   All of it separately rounded IEEE fp32, divide and square root correctly rounded, denormals kept: the results do not depend on the
 *   scene's SNAIL_ARITH_* mode.
 * RAYS: origin / dir / idir are nRays x 3 floats.  idir is used as given (TracePhotons passes VInv(dir)); NULL = 1.0f / dir per
 * component.  dist (nRays floats) is IN/OUT: the walk prunes against what it finds there.  indices (nIndices int32 ray numbers) selects
 * the rays to trace, NULL = all nRays (nIndices is then ignored); rays not listed keep their dist bytes; a number outside 0 .. nRays - 1
 * is skipped.  The entries are expected to be DISTINCT: with duplicates the distances are still correct, the per-ray counters undefined.
 * COUNTERS (optional): d_visits2 = per ray {box tests, triangle tests} as two int32 -- WideTest evaluations (two per inner node visited)
 * and Collide0 evaluations; d_stats = uint64[2], their sums ADDED.
 * WORKS ON handles of snail_scene_create, snail_scene_create_fast_dev (the committed tree; ordered against rebuilds like every launch)
 * and snail_scene_create_lbvh.  Launches are booked under the scene's lock like every other launch; the `_dev` forms never wait for
 * the device, except that a photon launch larger than any before grows the handle's scratch synchronously.
 * REFUSED with non-zero and nothing enqueued (snail_last_error() says which), the arguments judged before the handle is looked at:
 * negative counts, null required buffers, a negative startNode, nLights outside 0 .. SNAIL_MAX_LIGHTS; then an invalid handle, a
 * startNode outside the tree, a handle deeper than SNAIL_MAX_DEPTH = 64 levels.  nRays == 0 returns 0; a photon call without rays
 * (nLights * count == 0) still needs a valid handle and writes a count of 0.
 *
 * PHOTONS (TracePhotons:239-249, struct Photon src/photons.h:7-24): ray l * count + n is photon n of light l.  The distances start at
 * +inf, the rays are traced with idir = 1 / dir, and every ray whose distance is not +inf leaves one SnailPhoton, in ray order (the
 * reference's remove_if is stable): position = origin + dir * dist (multiply, then add), direction = dir, color[k] =
 * (uint8)Min(Max(c[k] * 255, 0), 255) in the select forms above (NaN -> 0; truncated), color[3] = 0 (the reference leaves it unset),
 * temp = 1.  lights7 (HOST, nLights x {pos[3], color[3], radius}) is read for the colours only.  d_photons32 must hold nLights * count
 * records; only the first *d_nPhotons are written, the rest of the buffer is not touched.
 *
 * NOT here: the emission loop (mt19937, libm's sin / cos and a rejection loop -- not bit-reproducible on a device; rays are an INPUT
 * of this header, snail_amd/photons.py has a NumPy stand-in), MakePhotonTree / GatherPhotons (nth_element's order is not reproducible
 * and nothing in the reference consumes the gather), a hit's triangle id (the reference returns none), instanced scenes.
 * Conventions are those of snail_hip.h: 0 = success, otherwise snail_last_error() holds the message.
 */
#ifndef SNAIL_WIDE_H
#define SNAIL_WIDE_H
#include "snail_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* struct Photon, 32 bytes */
typedef struct { float position[3]; float direction[3]; uint8_t color[4]; uint32_t temp; } SnailPhoton;

int snail_wide_trace_dev(SnailScene *scene, int nRays, const float *d_origin3, const float *d_dir3, const float *d_idir3,
                         const int32_t *d_indices, int nIndices, float *d_dist, int startNode, int32_t *d_visits2, uint64_t *d_stats,
                         void *stream);
/* the same on HOST pointers (stats2 = uint64[2], added to); returns after the results are in the host buffers */
int snail_wide_trace(SnailScene *scene, int nRays, const float *origin3, const float *dir3, const float *idir3, const int32_t *indices,
                     int nIndices, float *dist, int startNode, int32_t *visits2, uint64_t *stats2);

int snail_photons_trace_dev(SnailScene *scene, int nLights, int count, const float *d_origin3, const float *d_dir3, const float *lights7,
                            SnailPhoton *d_photons32, int32_t *d_nPhotons, uint64_t *d_stats, void *stream);
/* the same on HOST pointers: photons32 holds nLights * count records, *nPhotons receives the number written */
int snail_photons_trace(SnailScene *scene, int nLights, int count, const float *origin3, const float *dir3, const float *lights7,
                        SnailPhoton *photons32, int32_t *nPhotons, uint64_t *stats2);

#ifdef __cplusplus
}
#endif
#endif
