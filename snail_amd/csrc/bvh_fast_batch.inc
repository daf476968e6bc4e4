// bvh_fast_batch.inc -- the fast builder of bvh_fast.inc over SEVERAL handles in one pass (include/snail_bvh_fast_batch.h).  An animated
// instanced scene rebuilds a handful of small BLASes per frame; one build is about 35 dependent launches, most of them a few workgroups over
// a small mesh, and k builds in a row pay that chain k times.  Here the same chain is enqueued ONCE for up to kFastBatchMax trees: every phase
// is one launch whose workgroups are dealt to the trees, each workgroup working for one of them.
//
// Nothing of the build exists twice.  Each kernel below finds its tree and runs the body the single-tree kernel runs (build_common.inc,
// bvh_fast.inc: a function, or text in a *_body.inc file) with that tree's argument record and the workgroup's index and grid size WITHIN THE TREE'S SHARE.  A tree's share of every
// launch is the grid fastEnqueue gives it, its scratch is its handle's own, and the result of a build does not depend on which workgroup did
// what (ordered 64-bit keys, closed-form partition, numbering from (first, chain)): each handle ends byte-equal to a rebuild of its own.
// The early returns of the bodies -- status 1, an empty level, a tree of <= 64 triangles -- are per tree: a workgroup serves one tree only.
//
// THE TABLE goes by value in the kernel argument, as instances_materials_dynamic.inc's: kFastBatchMax records of devf::FastArgs (160 bytes
// each), the prefix of per-tree workgroup counts of THIS launch and the count: 16 * 160 + 17 * 4 + 4 = 2632 bytes, 2640 with the two level
// numbers of k_bfast_big, of HIP's 4096.  The tree is found from blockIdx by compares of scalars, and its record is read with scalar loads:
// no device table to fill, no staging, no allocation per call.  A longer list takes several passes.
namespace devf {

enum { kFastBatchMax = 16 };

struct FastBatch {
	FastArgs e[kFastBatchMax];
	int first[kFastBatchMax + 1];   // first[k] = the workgroups of the trees before k in this launch; first[count] = the grid
	int count;
};
static_assert(sizeof(FastArgs) == 160 && sizeof(FastBatch) == 2632 && sizeof(FastBatch) + 2 * sizeof(int) <= 4096, "the table must fit the kernel argument");

// the tree of workgroup g (g < first[count]): the last one that starts at or before g (first is non-decreasing; a tree without a share of this
// launch starts where the next one does and is passed over)
__device__ __forceinline__ int batchEntry(const FastBatch &T, int g) {
	int k = 0;
	for(int q = 1; q < kFastBatchMax; q++)
		if(q < T.count && g >= T.first[q]) k = q;
	return k;
}

__global__ void __launch_bounds__(256) k_bfast_init(FastBatch T) {
	const int g = blockIdx.x;
	if(g >= T.first[T.count]) return;
	const int k = batchEntry(T, g);
	fastInitBody(T.e[k], (unsigned)(g - T.first[k]));
}

__global__ void __launch_bounds__(256) k_bfast_boxes(FastBatch T) {
	const int g = blockIdx.x;
	if(g >= T.first[T.count]) return;
	const int k = batchEntry(T, g);
	fastBoxesBody(T.e[k], (unsigned)(g - T.first[k]));
}

// one workgroup of one wave per tree
__global__ void __launch_bounds__(64) k_bfast_root(FastBatch T) {
	const int k = blockIdx.x;
	if(k >= T.count) return;
	devb::buildRootBody<devb::SplitBvh>(T.e[k], 0);
}

// The batched kernels' policy: SplitBvh under a name of its own, so that splitNode<T, P> is instantiated for them apart from the single-tree
// kernels' instance.  With one instance and two callers the compiler stops inlining it into k_build_big / k_build_small, whose code -- the
// shipped path of every single build -- would then no longer be what it was.
struct SplitBvhBatch : devb::SplitBvh {};

// (the three bodies that are text: the tree's record under the name A, its share of the launch as the two macros)
#define SNAIL_BODY_BLOCK (wg - T.first[k])
#define SNAIL_BODY_GRID (T.first[k + 1] - T.first[k])

// levels [level0, level1) of every tree that has a share (level1 > level0 + 1 only with one workgroup per tree, as k_build_big)
__global__ void __launch_bounds__(256) k_bfast_big(FastBatch T, int level0, int level1) {
	using namespace devb;
	typedef SplitBvhBatch P;
	__shared__ SplitLds S;
	__shared__ int levelCount;
	const int wg = blockIdx.x;
	if(wg >= T.first[T.count]) return;
	const int k = batchEntry(T, wg);
	const FastArgs &A = T.e[k];
#include "build_big_body.inc"
}

__global__ void __launch_bounds__(64) k_bfast_small(FastBatch T) {
	using namespace devb;
	typedef SplitBvhBatch P;
	__shared__ SplitLds S;
	__shared__ int stack[kLevels + 8];
	const int wg = blockIdx.x;
	if(wg >= T.first[T.count]) return;
	const int k = batchEntry(T, wg);
	const FastArgs &A = T.e[k];
#include "build_small_body.inc"
}

// one workgroup of 1024 threads per tree
__global__ void __launch_bounds__(1024) k_bfast_scan(FastBatch T) {
	__shared__ int s[1024];
	const int k = blockIdx.x;
	if(k >= T.count) return;
	devb::buildScanBody(T.e[k], s);
}

__global__ void __launch_bounds__(256) k_bfast_commit(FastBatch T) {
	const int wg = blockIdx.x;
	if(wg >= T.first[T.count]) return;
	const int k = batchEntry(T, wg);
	const FastArgs &A = T.e[k];
#include "bvh_fast_commit_body.inc"
}

#undef SNAIL_BODY_BLOCK
#undef SNAIL_BODY_GRID

} // namespace devf

// ---- host side ----
namespace {

// one handle of a batch, after its arguments were judged
struct FastBatchItem { SnailScene *s; const float *dVerts; int32_t *dPerm, *dInfo; };

// fastRebuildLocked for several handles (every mu held, all on the current device, no handle twice): `st` waits for every handle's users and
// previous rebuild, then ONE chain of launches builds them all, kFastBatchMax per pass, and every handle's `ready` is recorded behind it
int fastRebuildBatchLocked(const FastBatchItem *items, int nItems, hipStream_t st) {
	for(int k = 0; k < nItems; k++) {
		if(int rc = fastWaitUsers(items[k].s, st)) return rc;
		for(auto &e : items[k].s->rel) e.valid = false;   // (as fastRebuildLocked: the origin-relative copies describe the old tree)
	}
	typedef devb::SplitBvh P;
	for(int at = 0; at < nItems; at += devf::kFastBatchMax) {
		devf::FastBatch T;
		memset((void *)&T, 0, sizeof(T));
		const int count = std::min(nItems - at, (int)devf::kFastBatchMax);
		T.count = count;
		int n[devf::kFastBatchMax], maxN = 0;
		for(int k = 0; k < count; k++) {
			SnailScene *s = items[at + k].s;
			SnailSceneFast *f = s->fast;
			devf::FastArgs &A = T.e[k];
			n[k] = s->nTris;
			maxN = std::max(maxN, n[k]);
			buildCarve(f->base, n[k], A);
			A.n = n[k]; A.maxDepth = f->depthLimit;
			A.verts = items[at + k].dVerts;
			A.nodes = s->dNodes; A.tris = s->dTris; A.pf = s->pfOKButNesting ? (uint4 *)s->dPF : nullptr; A.trisOff = (unsigned)s->trisOff;
			A.needSane = s->fastOK; A.cur = f->dCur; A.perm = items[at + k].dPerm; A.info = items[at + k].dInfo;
		}
		// the launch's shares: share(k) workgroups for tree k (fastEnqueue's grids), the trees side by side; nothing is launched when no tree has one
		auto deal = [&](auto share) {
			for(int k = 0; k < count; k++) T.first[k + 1] = T.first[k] + share(k);
			for(int k = count + 1; k <= devf::kFastBatchMax; k++) T.first[k] = T.first[count];
			return (unsigned)T.first[count];
		};
		unsigned grid = deal([&](int k) { return (n[k] + 255) / 256; });
		hipLaunchKernelGGL(devf::k_bfast_init, dim3(grid), dim3(256), 0, st, T);
		hipLaunchKernelGGL(devf::k_bfast_boxes, dim3(grid), dim3(256), 0, st, T);
		hipLaunchKernelGGL(devf::k_bfast_root, dim3((unsigned)count), dim3(64), 0, st, T);
		if(maxN > devb::kSmall) {
			const int wide = 28;
			for(int level = 0; level < wide; level++) {
				grid = deal([&](int k) { return n[k] > devb::kSmall ? std::min(level < 11 ? (1 << level) : 2048, n[k] / (devb::kSmall + 1) + 1) : 0; });
				hipLaunchKernelGGL(devf::k_bfast_big, dim3(grid), dim3(256), 0, st, T, level, level + 1);
			}
			grid = deal([&](int k) { return n[k] > devb::kSmall ? 1 : 0; });
			hipLaunchKernelGGL(devf::k_bfast_big, dim3(grid), dim3(256), 0, st, T, wide, (int)devb::kLevels);
		}
		grid = deal([&](int k) { return n[k] >= P::minSplit ? std::min(n[k] / 2 + 1, 8192) : 0; });
		if(grid) hipLaunchKernelGGL(devf::k_bfast_small, dim3(grid), dim3(64), 0, st, T);
		hipLaunchKernelGGL(devf::k_bfast_scan, dim3((unsigned)count), dim3(1024), 0, st, T);
		grid = deal([&](int k) { return (int)std::min((2 * (long long)n[k] + 255) / 256, 4096LL); });
		hipLaunchKernelGGL(devf::k_bfast_commit, dim3(grid), dim3(256), 0, st, T);
	}
	HIP_TRY(hipGetLastError());
	for(int k = 0; k < nItems; k++) {
		SnailSceneFast *f = items[k].s->fast;
		if(!f->ready) HIP_TRY(hipEventCreateWithFlags(&f->ready, hipEventDisableTiming));
		HIP_TRY(hipEventRecord(f->ready, st));
		f->hasReady = true;
		f->curOnDevice = true;
		f->rebuilds++;
	}
	return 0;
}

} // namespace

extern "C" {

int snail_scenes_rebuild_fast_dev(const SnailFastRebuild *list, int nList, void *stream) {
	const char *fn = "snail_scenes_rebuild_fast_dev";
	if(!list || nList <= 0) { snail_set_error("%s: no handle listed (a null list or nList <= 0)", fn); return 1; }
	// the whole list is judged before any handle is touched
	for(int k = 0; k < nList; k++) {
		SnailScene *s = list[k].scene;
		if(!s || !s->dNodes || !s->dPF || !s->dTris) { snail_set_error("%s: entry %d: invalid scene handle", fn, k); return 1; }
		if(!s->fast) { snail_set_error("%s: entry %d: the handle was not made by snail_scene_create_fast_dev", fn, k); return 1; }
		if(!list[k].d_verts9 || list[k].nTris != s->nTris) {
			snail_set_error("%s: entry %d: %d triangles, the handle holds %d (or null vertices)", fn, k, list[k].nTris, s->nTris);
			return 1;
		}
		for(int j = 0; j < k; j++)
			if(list[j].scene == s) { snail_set_error("%s: entry %d: the handle is listed twice (entry %d)", fn, k, j); return 1; }
		if(s->device != list[0].scene->device) {
			snail_set_error("%s: entry %d: the handle is on device %d, entry 0 on device %d (one batch, one device)", fn, k, s->device, list[0].scene->device);
			return 1;
		}
	}
	hipStream_t st = (hipStream_t)stream;
	DeviceGuard guard(list[0].scene->device);
	// the locks in ADDRESS order (snail_render_tiles_multi's rule): two threads with the same handles in different orders cannot wait for each other
	std::vector<SnailScene *> byAddr((size_t)nList);
	for(int k = 0; k < nList; k++) byAddr[k] = list[k].scene;
	std::sort(byAddr.begin(), byAddr.end());
	std::vector<std::unique_lock<std::mutex>> locks;
	for(SnailScene *s : byAddr) locks.emplace_back(s->mu);
	std::vector<FastBatchItem> items((size_t)nList);
	for(int k = 0; k < nList; k++) items[k] = FastBatchItem{list[k].scene, list[k].d_verts9, list[k].d_perm, list[k].d_info};
	return fastRebuildBatchLocked(items.data(), nList, st);
}

#ifdef SNAIL_DEBUG_API
// The workbench build only, for the tests: the builds enqueued on a handle of snail_scene_create_fast_dev so far (a refused call leaves it alone).
int snail_scene_debug_rebuilds(SnailScene *s, uint64_t *out) {
	const char *fn = "snail_scene_debug_rebuilds";
	if(int rc = checkScene(s, fn)) return rc;
	if(!s->fast || !out) { snail_set_error("%s: not a handle of snail_scene_create_fast_dev, or a null result", fn); return 1; }
	SNAIL_LOCK(s);
	*out = s->fast->rebuilds;
	return 0;
}
#endif

} // extern "C"
