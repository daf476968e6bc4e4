// bvh_fast.inc -- BVH::Construct(scene, fastBuild) on the device (include/snail_bvh_fast.h): the reference's 16-bin builder BVH::FindSplit
// (src/bvh/tree.cpp:161-287) over vertices already in device memory, into a scene handle that stays on the device.  Byte-equal to
// snail_tris_from_verts + snail_bvh_build_fast (bvh_build.cpp), whose fp32 operation order every expression repeats (plain fp32,
// -ffp-contract=off, IEEE divide / sqrt, denormals kept; neither Inv nor RSqrt, so it exists once and not per arithmetic).
//
// BVH::FindSplit is DBVH::FindSplit over triangle boxes: a leaf at <= 4 elements instead of 1, always 16 bins, the same epsilon.  The
// split is therefore the one of build_common.inc under the policy SplitBvh -- ordered min / max keys, closed-form partition order,
// pre-order numbering from a scan + chain counts: all explained at the top of instances_build.inc -- and this file adds what surrounds it.
//
// PHASES (kernel boundaries on one stream) for n = 10^5 .. 10^6 triangles:
//   k_fast_init    counters, per-slot inner-node counts := 0
//   k_fast_boxes   one thread per triangle: vertices finite (before a value indexes anything), Triangle::GetBBox from a, ba + a, ca + a, the
//                  sanity conditions of the fast arithmetic paths, root box keys (global 64-bit atomics, pre-checked by a plain read)
//   k_build_root   temporary node 0
//   k_build_big    level L splits the nodes of depth L with more than 64 triangles, one 256-thread workgroup per node and up to 2048
//                  workgroups per launch that stride over the level's list: bins in LDS under 64-bit integer-key atomics, the partition as
//                  ballot prefix counts + a swap list.  One launch per level for levels 0..27 (a balanced tree over 10^6 triangles has
//                  such nodes down to level 14; a launch on an empty level returns at once), then one single-workgroup launch for the tail.
//                  The top levels are few workgroups over many triangles (level 0 is ONE workgroup over all of them): they bound the
//                  build time at this scale -- the instance builder's plan carried over, not one tuned for 10^6 triangles: splitting the top
//                  levels' binning over several workgroups (global key atomics) is the next step once tools/build_time.py has numbers
//   k_build_small  hand-off at <= 64 triangles: one wave finishes that subtree, stack in LDS
//   k_build_scan   exclusive prefix sum of the inner-node counts by first slot
//   k_fast_commit  the ONLY writer of the handle, and only on status 0: nodes under their final numbers (+ the node loop's re-encoded copy),
//                  the 64-byte triangle records computed ONCE from the vertices through the final permutation (36 bytes read per triangle
//                  instead of a 64-byte gather per level), perm, info, and {nNodes, depth} for the host to read later
// Sizes: n <= 4 (root leaf), 5..64 (root straight onto the small list), > 64 (big levels, then small subtrees).
namespace devf {

using devb::BuildHdr;
using devb::TNode;
static_assert(SNAIL_MAX_DEPTH == devb::kMaxDepth, "BuildHdr::qCount and the small kernel's stack are sized for DBVH::maxDepth == BVH::maxDepth");

struct FastArgs : devb::SplitArgs {
	const float *verts;
	uint4 *nodes, *pf, *tris;       // the handle's: node records, the node loop's copy (null: none), triangle records
	unsigned trisOff;
	int needSane;                   // the handle's launches take the fast arithmetic paths: a tree that may not is status 3
	int *cur;                       // {nNodes, depth, sane, 0} of the tree the handle holds
	int *perm, *info;
};

// (bodies as functions of the record and a block index, the commit's as text in bvh_fast_commit_body.inc: bvh_fast_batch.inc runs them for one
// tree of several per launch)
__device__ __forceinline__ void fastInitBody(const FastArgs &A, unsigned block) {
	const int i = block * blockDim.x + threadIdx.x;
	if(i < A.n) A.startCnt[i] = 0;
	if(i == 0) devb::hdrInit(*A.hdr);
}
__global__ void k_fast_init(FastArgs A) { fastInitBody(A, blockIdx.x); }

__device__ __forceinline__ void fastBoxesBody(const FastArgs &A, unsigned block) {
	const int i = block * blockDim.x + threadIdx.x;
	if(i >= A.n) return;
	float p[9], rec[16];
	bool ok = true;
	for(int k = 0; k < 9; k++) { p[k] = A.verts[(size_t)i * 9 + k]; ok = ok && devb::finiteBits(p[k]); }
	if(!ok) { atomicMax(&A.hdr->status, 1); return; }
	bool sane = dev::lbvh::triRecord(p, rec);
	// Triangle::GetBBox (src/triangle.h:35-37,62-70) from the record, as bvh_build.cpp's boundsOf
	float lo[3], hi[3];
	for(int k = 0; k < 3; k++) {
		const float p1 = rec[k], p2 = rec[3 + k] + rec[k], p3 = rec[6 + k] + rec[k];
		lo[k] = devb::fmin2(p1, devb::fmin2(p2, p3));
		hi[k] = devb::fmax2(p1, devb::fmax2(p2, p3));
		sane = sane && fabsf(lo[k]) <= 1.0e9f && fabsf(hi[k]) <= 1.0e9f && lo[k] <= hi[k];
	}
	if(!sane) A.hdr->insane = 1;
	float *o = A.box + (size_t)i * 6;
	for(int k = 0; k < 3; k++) { o[k] = lo[k]; o[3 + k] = hi[k]; }
	A.src[i] = i;
	// the root box: box[0] grown by 1..n-1 in the caller's order
	for(int k = 0; k < 3; k++) { devb::keyMin(&A.hdr->rootMin[k], lo[k], i); devb::keyMax(&A.hdr->rootMax[k], hi[k], i); }
}
__global__ void k_fast_boxes(FastArgs A) { fastBoxesBody(A, blockIdx.x); }

__global__ void k_fast_commit(FastArgs A) {
#define SNAIL_BODY_BLOCK blockIdx.x
#define SNAIL_BODY_GRID gridDim.x
#include "bvh_fast_commit_body.inc"
#undef SNAIL_BODY_BLOCK
#undef SNAIL_BODY_GRID
}

} // namespace devf

// ---- host side ----
// What a handle of snail_scene_create_fast_dev carries besides the scene: the builder's scratch (one allocation, sized at creation: a
// rebuild keeps nTris), {nNodes, depth, sane} of the tree as the DEVICE knows them once a rebuild has been enqueued, and the ordering of
// rebuilds against launches -- snail_instances_update's scheme: the rebuild's stream waits for one event per stream that launched, every
// later launch waits for `ready` (SceneUse, in every launch path of snail_hip.hip and instances_host.inc).
struct SnailSceneFast {
	char *base = nullptr;
	int *dCur = nullptr;
	int cur[4] = {0, 0, 0, 0};
	bool curOnDevice = false;
	int depthLimit = SNAIL_MAX_DEPTH;   // what the stack form chosen at creation takes (useDeep): 62, or SNAIL_MAX_DEPTH for a handle created deeper
	hipEvent_t ready = nullptr;
	bool hasReady = false;
	unsigned long long rebuilds = 0;   // builds enqueued on the handle so far (under mu): what a set of snail_materials_create_dev compares its own count with
	struct Use { hipStream_t stream; hipEvent_t ev; };
	std::vector<Use> uses;
};

namespace {

void fastFree(SnailSceneFast *f) {
	if(!f) return;
	if(f->base) (void)hipFree(f->base);
	if(f->dCur) (void)hipFree(f->dCur);
	if(f->ready) (void)hipEventDestroy(f->ready);
	for(auto &u : f->uses) (void)hipEventDestroy(u.ev);
	delete f;
}

int fastSceneBegin(SnailScene *s, hipStream_t stream) {
	SnailSceneFast *f = s->fast;
	if(f->hasReady) HIP_TRY(hipStreamWaitEvent(stream, f->ready, 0));
	return 0;
}
void fastSceneEnd(SnailScene *s, hipStream_t stream) {
	SnailSceneFast *f = s->fast;
	for(auto &u : f->uses)
		if(u.stream == stream) { (void)hipEventRecord(u.ev, stream); return; }
	SnailSceneFast::Use u;
	u.stream = stream;
	if(hipEventCreateWithFlags(&u.ev, hipEventDisableTiming) != hipSuccess) return;
	(void)hipEventRecord(u.ev, stream);
	f->uses.push_back(u);
}

// the whole build on `st` (mu held, or the handle not yet published)
int fastEnqueue(SnailScene *s, const float *dVerts, int32_t *dPerm, int32_t *dInfo, int needSane, hipStream_t st) {
	SnailSceneFast *f = s->fast;
	const int n = s->nTris;
	devf::FastArgs A;
	memset((void *)&A, 0, sizeof(A));
	buildCarve(f->base, n, A);
	A.n = n; A.maxDepth = f->depthLimit;
	A.verts = dVerts;
	A.nodes = s->dNodes; A.tris = s->dTris; A.pf = s->pfOKButNesting ? (uint4 *)s->dPF : nullptr; A.trisOff = (unsigned)s->trisOff;
	A.needSane = needSane; A.cur = f->dCur; A.perm = dPerm; A.info = dInfo;
	const devb::SplitArgs &SA = A;
	typedef devb::SplitBvh P;
	const int perN = (n + 255) / 256;
	hipLaunchKernelGGL(devf::k_fast_init, dim3(perN), dim3(256), 0, st, A);
	hipLaunchKernelGGL(devf::k_fast_boxes, dim3(perN), dim3(256), 0, st, A);
	hipLaunchKernelGGL(devb::k_build_root<P>, dim3(1), dim3(64), 0, st, SA);
	if(n > devb::kSmall) {
		// level L holds at most min(2^L, n / 65) nodes of more than 64 triangles; how many it does hold only the device knows: sized for the
		// worst case (capped; the workgroups stride), the surplus leaves at once
		const int most = n / (devb::kSmall + 1) + 1;
		const int wide = 28;
		for(int level = 0; level < wide; level++) {
			const int grid = std::min(level < 11 ? (1 << level) : 2048, most);
			hipLaunchKernelGGL(devb::k_build_big<P>, dim3(grid), dim3(256), 0, st, SA, level, level + 1);
		}
		hipLaunchKernelGGL(devb::k_build_big<P>, dim3(1), dim3(256), 0, st, SA, wide, (int)devb::kLevels);
	}
	if(n >= P::minSplit) hipLaunchKernelGGL(devb::k_build_small<P>, dim3(std::min(n / 2 + 1, 8192)), dim3(64), 0, st, SA);
	hipLaunchKernelGGL(devb::k_build_scan, dim3(1), dim3(1024), 0, st, SA);
	hipLaunchKernelGGL(devf::k_fast_commit, dim3((unsigned)std::min((2 * (long long)n + 255) / 256, 4096LL)), dim3(256), 0, st, A);
	HIP_TRY(hipGetLastError());
	if(!f->ready) HIP_TRY(hipEventCreateWithFlags(&f->ready, hipEventDisableTiming));
	HIP_TRY(hipEventRecord(f->ready, st));
	f->hasReady = true;
	f->curOnDevice = true;
	f->rebuilds++;
	return 0;
}

// What comes before anything that rewrites what the handle's launches read (mu held): `st` waits for every launch enqueued since the previous
// rebuild (they read what the commit writes) and for that rebuild itself (one scratch area)
int fastWaitUsers(SnailScene *s, hipStream_t st) {
	SnailSceneFast *f = s->fast;
	for(auto &u : f->uses) HIP_TRY(hipStreamWaitEvent(st, u.ev, 0));
	if(f->hasReady) HIP_TRY(hipStreamWaitEvent(st, f->ready, 0));
	return 0;
}

// snail_scene_rebuild_fast_dev after its arguments were judged (mu held); snail_materials_rebuild_dev's first half
int fastRebuildLocked(SnailScene *s, const float *dVerts, int32_t *dPerm, int32_t *dInfo, hipStream_t st) {
	if(int rc = fastWaitUsers(s, st)) return rc;
	// the origin-relative copies of the node slots describe the old tree: a later launch fills its own again (relFor waits for an array's
	// previous fill and its last readers before it overwrites it)
	for(auto &e : s->rel) e.valid = false;
	return fastEnqueue(s, dVerts, dPerm, dInfo, s->fastOK, st);
}

// {nNodes, depth, sane} of the tree the handle holds, waiting for a rebuild in flight if there is one
int fastCurrent(const SnailScene *cs, int cur[4]) {
	SnailScene *s = const_cast<SnailScene *>(cs);
	SnailSceneFast *f = s->fast;
	DeviceGuard guard(s->device);
	std::lock_guard<std::mutex> lock(s->mu);
	if(f->curOnDevice) {
		if(f->hasReady) HIP_TRY(hipEventSynchronize(f->ready));
		HIP_TRY(hipMemcpy(f->cur, f->dCur, sizeof(f->cur), hipMemcpyDeviceToHost));
		f->curOnDevice = false;
	}
	memcpy(cur, f->cur, sizeof(f->cur));
	return 0;
}

} // namespace

extern "C" {

SnailScene *snail_scene_create_fast_dev(const float *d_verts9, int nTris, int device, int32_t *d_perm, int32_t *d_info, void *stream) {
	const char *fn = "snail_scene_create_fast_dev";
	if(!d_verts9 || nTris <= 0 || nTris > (1 << 29)) { snail_set_error("%s: bad arguments", fn); return nullptr; }
	DeviceGuard guard(device);
	if(!guard.ok) { snail_set_error("%s: hipSetDevice(%d) failed", fn, device); return nullptr; }
	hipStream_t st = (hipStream_t)stream;
	SnailScene *s = new SnailScene();
	s->fast = new SnailSceneFast();
	SnailSceneFast *f = s->fast;
	// the node arrays have room for the largest tree over nTris triangles; the slots past the current tree are empty leaves nobody refers to
	const int cap = 2 * nTris - 1;
	s->device = device; s->nNodes = cap; s->nTris = nTris;
	const size_t trisOff = pfTrisOffset(cap), pfBytes = trisOff + (size_t)nTris * 64;
	const bool fits = pfFits((size_t)cap + 1, (size_t)nTris);
	s->trisOff = (int)(fits ? trisOff : 0);
	s->pfOKButNesting = fits ? 1 : 0;   // (children are numbered in pairs from 1 on)
	hipError_t e;
	if((e = hipMalloc((void **)&s->dNodes, (size_t)cap * 32)) != hipSuccess || (e = hipMalloc((void **)&s->dPF, fits ? pfBytes : (size_t)nTris * 64)) != hipSuccess ||
	   (e = hipMalloc((void **)&f->base, buildScratchBytes(nTris))) != hipSuccess || (e = hipMalloc((void **)&f->dCur, 4 * sizeof(int))) != hipSuccess ||
	   (fits && (e = hipMemset(s->dPF, 0, ((size_t)cap + 1) * 32)) != hipSuccess) || (e = hipMemset(f->dCur, 0, 4 * sizeof(int))) != hipSuccess) {
		snail_set_error("%s: %s", fn, hipGetErrorString(e));
		snail_scene_destroy(s);
		return nullptr;
	}
	s->dTris = (uint4 *)(s->dPF + s->trisOff);
	hipLaunchKernelGGL(dev::lbvh::k_fill_empty, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, 0, (float *)s->dNodes, cap);
	int cur[4] = {0, 0, 0, 0}, status[8] = {0};
	if((e = hipDeviceSynchronize()) != hipSuccess || fastEnqueue(s, d_verts9, d_perm, d_info, 0, st) != 0 || (e = hipStreamSynchronize(st)) != hipSuccess ||
	   (e = hipMemcpy(status, f->base, sizeof(status), hipMemcpyDeviceToHost)) != hipSuccess || fastCurrent(s, cur) != 0) {
		if(e != hipSuccess) snail_set_error("%s: %s", fn, hipGetErrorString(e));
		snail_scene_destroy(s);
		return nullptr;
	}
	if(status[0] != 0) {   // BuildHdr::status
		if(status[0] == 1) snail_set_error("%s: a vertex is not finite", fn);
		else snail_set_error("%s: the tree is deeper than BVH::maxDepth = %d", fn, SNAIL_MAX_DEPTH);
		snail_scene_destroy(s);
		return nullptr;
	}
	// the finishing steps of snail_scene_create: the stack form from the depth, the arithmetic paths from the records' sanity; the tree is nested
	// by construction (every box is an ordered fold over a subset of its parent's triangles)
	s->depth = cur[1]; s->fastOK = cur[2]; s->nestedOK = 1; s->pfOK = s->pfOKButNesting;
	f->depthLimit = s->depth > 62 ? SNAIL_MAX_DEPTH : 62;
	return s;
}

int snail_scene_rebuild_fast_dev(SnailScene *s, const float *d_verts9, int nTris, int32_t *d_perm, int32_t *d_info, void *stream) {
	const char *fn = "snail_scene_rebuild_fast_dev";
	if(int rc = checkScene(s, fn)) return rc;
	if(!s->fast) { snail_set_error("%s: the handle was not made by snail_scene_create_fast_dev", fn); return 1; }
	if(!d_verts9 || nTris != s->nTris) { snail_set_error("%s: %d triangles, the handle holds %d (or null vertices)", fn, nTris, s->nTris); return 1; }
	hipStream_t st = (hipStream_t)stream;
	DeviceGuard guard(s->device);
	SNAIL_LOCK(s);
	return fastRebuildLocked(s, d_verts9, d_perm, d_info, st);
}

} // extern "C"
