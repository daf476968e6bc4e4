// build_common.inc -- what the two device tree builders share (instances_build.inc: DBVH::FindSplit over instance boxes; bvh_fast.inc:
// BVH::FindSplit over triangle boxes): ordered min / max as 64-bit integer keys, the binned split of one node with the closed form of
// libstdc++'s partition order, the per-level and per-subtree kernels, and the scan behind the pre-order numbering.  The two builders differ
// in a Policy (the smallest node that is split, the number of bins) and in what surrounds the split: element boxes before, commit after.
// The reasoning behind the keys, the phases and the numbering is at the top of instances_build.inc.
namespace devb {

typedef unsigned long long u64;
enum { kSmall = 64, kMaxDepth = SNAIL_INSTANCES_MAX_DEPTH, kLevels = SNAIL_INSTANCES_MAX_DEPTH + 1 };

struct TNode {                      // a node under construction, 64 bytes
	float lo[3], hi[3];
	int first, count;
	int aux;                        // leaf: count; inner: axis | firstNode << 16
	int inner;
	int chain;                      // inner ancestors with the same first slot
	int pfirst, pchain, side;       // the parent's (first, chain) and which child this is
	int sdepth;
	int pad;
};

struct BuildHdr {
	int status, depth, nTemp, nSmall, totalInner;
	int insane;                     // bvh_fast.inc: a record outside the range of the fast arithmetic paths
	int pad[2];
	u64 rootMin[3], rootMax[3];
	int qCount[kLevels + 3];
};

// what the split kernels read and write: the elements' boxes and source indices (permuted in place), per-element scratch, the nodes under
// construction and the work lists; each builder's argument record starts with it
struct SplitArgs {
	int n, maxDepth;                // elements; a split that would put children below maxDepth sets status 2
	float *box; int *src, *binE, *tmpA, *tmpB, *startCnt;
	TNode *tn; int *queue[2]; int *small;
	BuildHdr *hdr;
};
// DBVH::FindSplit (src/dbvh/tree.cpp:46-152): a node of one instance is a leaf; 8 bins below 8 instances
struct SplitDbvh {
	enum { minSplit = 2 };
	static __device__ __forceinline__ int bins(int count) { return count < 8 ? 8 : 16; }
};
// BVH::FindSplit (src/bvh/tree.cpp:161-287): a node of up to 4 triangles is a leaf; always 16 bins
struct SplitBvh {
	enum { minSplit = 5 };
	static __device__ __forceinline__ int bins(int) { return 16; }
};

__device__ __forceinline__ float fmin2(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float fmax2(float a, float b) { return a > b ? a : b; }

__device__ __forceinline__ unsigned mono(float x) {
	unsigned u = __float_as_uint(x);
	if(u == 0x80000000u) u = 0;
	return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unmono(unsigned m, unsigned sign) {
	unsigned u = (m & 0x80000000u) ? (m ^ 0x80000000u) : ~m;
	if(u == 0 && sign) u = 0x80000000u;
	return __uint_as_float(u);
}
__device__ __forceinline__ u64 minKey(float x, int pos) {
	return ((u64)mono(x) << 32) | ((u64)(unsigned)(0x7fffffff - pos) << 1) | (u64)(__float_as_uint(x) >> 31);
}
__device__ __forceinline__ u64 maxKey(float x, int pos) {
	return ((u64)mono(x) << 32) | ((u64)(unsigned)pos << 1) | (u64)(__float_as_uint(x) >> 31);
}
__device__ __forceinline__ float keyValue(u64 k) { return unmono((unsigned)(k >> 32), (unsigned)(k & 1)); }
#define SNAIL_KEY_MIN_INIT 0xff800000fffffffeull   /* minKey(+inf, 0) */
#define SNAIL_KEY_MAX_INIT 0x007fffff00000001ull   /* maxKey(-inf, 0) */
// (the plain read only spares atomics that cannot win: the cell moves one way, so a stale value never hides a winner.  The cells are
// 8-byte aligned and read with one ds_read_b64 / global_load_dwordx2: a single access, never two halves of different values)
__device__ __forceinline__ void keyMin(u64 *p, float x, int pos) {
	const u64 k = minKey(x, pos);
	if(k < *(volatile u64 *)p) atomicMin(p, k);
}
__device__ __forceinline__ void keyMax(u64 *p, float x, int pos) {
	const u64 k = maxKey(x, pos);
	if(k > *(volatile u64 *)p) atomicMax(p, k);
}

// BoxSA (src/dbvh/tree.cpp:40-42)
__device__ __forceinline__ float boxArea(const float *lo, const float *hi) {
	const float w = hi[0] - lo[0], h = hi[1] - lo[1], d = hi[2] - lo[2];
	return (w * (d + h) + d * h) * 2.0f;
}
// int((c - sub) * mul) with the defined deviation of dbvh_build.cpp
__device__ __forceinline__ int binOf(float c, float sub, float mul, int nBins) {
	const float v = (c - sub) * mul;
	if(!(v >= 0.0f)) return 0;
	if(!(v < (float)nBins)) return nBins - 1;
	return (int)v;
}
__device__ __forceinline__ bool finiteBits(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ void hdrInit(BuildHdr &H) {
	H.status = 0; H.depth = 0; H.nTemp = 0; H.nSmall = 0; H.totalInner = 0; H.insane = 0;
	for(int k = 0; k < 3; k++) { H.rootMin[k] = SNAIL_KEY_MIN_INIT; H.rootMax[k] = SNAIL_KEY_MAX_INIT; }
	for(int k = 0; k < kLevels + 3; k++) H.qCount[k] = 0;
}

// The kernels' bodies are functions of the argument record (and, where they use them, a block index and a grid size), or text in a file of
// their own (build_big_body.inc, build_small_body.inc: see there), so that the batched builder (bvh_fast_batch.inc) runs the same code for
// one tree of several per launch, with the block index and grid size of that tree's share
template <class P>
__device__ __forceinline__ void buildRootBody(const SplitArgs &A, int block) {
	BuildHdr &H = *A.hdr;
	if(threadIdx.x != 0 || block != 0 || H.status != 0) return;
	TNode r;
	for(int k = 0; k < 3; k++) { r.lo[k] = keyValue(H.rootMin[k]); r.hi[k] = keyValue(H.rootMax[k]); }
	r.first = 0; r.count = A.n; r.aux = A.n; r.inner = 0; r.chain = 0; r.pfirst = 0; r.pchain = 0; r.side = 0; r.sdepth = 0; r.pad = 0;
	A.tn[0] = r;
	H.nTemp = 1;
	if(A.n > kSmall) { A.queue[0][0] = 0; H.qCount[0] = 1; }
	else if(A.n >= P::minSplit) { A.small[0] = 0; H.nSmall = 1; }
}
template <class P>
__global__ void k_build_root(SplitArgs A) { buildRootBody<P>(A, (int)blockIdx.x); }

struct SplitLds {
	u64 bmin[16][3], bmax[16][3];
	u64 mmin[2][3], mmax[2][3];
	float lbox[16][6], rbox[16][6];
	int bcnt[16], lcnt[16], rcnt[16];
	int wsum[4];
	int minIdx, leaf, m;
	int child, cL, cR;       // the children made (child < 0: none) and their counts
};

// FindSplit for the node tn[t] of at least P::minSplit elements, by the T threads of one workgroup (T = 64: one wave)
template <int T, class P>
__device__ void splitNode(const SplitArgs &A, int t, SplitLds &S) {
	const int tid = threadIdx.x;
	const TNode nd = A.tn[t];
	const int first = nd.first, count = nd.count;
	float size[3];
	for(int k = 0; k < 3; k++) size[k] = nd.hi[k] - nd.lo[k];
	const int axis = size[1] > size[0] ? (size[2] > size[1] ? 2 : 1) : (size[2] > size[0] ? 2 : 0);
	const int nBins = P::bins(count);
	const float ndLo = axis == 0 ? nd.lo[0] : axis == 1 ? nd.lo[1] : nd.lo[2];
	const float ndHi = axis == 0 ? nd.hi[0] : axis == 1 ? nd.hi[1] : nd.hi[2];
	const float mul = __fdiv_rn((float)nBins * (1.0f - 0.0001f), ndHi - ndLo);
	const float sub = ndLo;
	for(int k = tid; k < 48; k += T) { (&S.bmin[0][0])[k] = SNAIL_KEY_MIN_INIT; (&S.bmax[0][0])[k] = SNAIL_KEY_MAX_INIT; }
	for(int k = tid; k < 6; k += T) { (&S.mmin[0][0])[k] = SNAIL_KEY_MIN_INIT; (&S.mmax[0][0])[k] = SNAIL_KEY_MAX_INIT; }
	if(tid < 16) S.bcnt[tid] = 0;
	if(tid == 0) { S.child = -1; S.cL = 0; S.cR = 0; S.m = 0; }
	__syncthreads();
	// bins accumulate their members in element order: the keys carry the element's position
	for(int i = tid; i < count; i += T) {
		const float *b = A.box + (size_t)(first + i) * 6;
		const float c = (b[3 + axis] + b[axis]) * 0.5f;
		const int bin = binOf(c, sub, mul, nBins);
		A.binE[first + i] = bin;
		atomicAdd(&S.bcnt[bin], 1);
		for(int k = 0; k < 3; k++) { keyMin(&S.bmin[bin][k], b[k], i); keyMax(&S.bmax[bin][k], b[3 + k], i); }
	}
	__syncthreads();
	// prefix / suffix boxes and counts: the host's serial loops, one lane per box component
	if(tid < 6) {
		const bool isMin = tid < 3;
		const int k = isMin ? tid : tid - 3;
		float acc = isMin ? keyValue(S.bmin[0][k]) : keyValue(S.bmax[0][k]);
		S.lbox[0][tid] = acc;
		for(int b = 1; b < nBins; b++) {
			const float x = isMin ? keyValue(S.bmin[b][k]) : keyValue(S.bmax[b][k]);
			acc = isMin ? fmin2(acc, x) : fmax2(acc, x);
			S.lbox[b][tid] = acc;
		}
		acc = isMin ? keyValue(S.bmin[nBins - 1][k]) : keyValue(S.bmax[nBins - 1][k]);
		S.rbox[nBins - 1][tid] = acc;
		for(int b = nBins - 2; b >= 0; b--) {
			const float x = isMin ? keyValue(S.bmin[b][k]) : keyValue(S.bmax[b][k]);
			acc = isMin ? fmin2(acc, x) : fmax2(acc, x);
			S.rbox[b][tid] = acc;
		}
	} else if(tid == 6) {
		int acc = 0;
		for(int b = 0; b < nBins; b++) { acc += S.bcnt[b]; S.lcnt[b] = acc; }
		acc = 0;
		for(int b = nBins - 1; b >= 0; b--) { acc += S.bcnt[b]; S.rcnt[b] = acc; }
	}
	__syncthreads();
	if(tid == 0) {
		float minCost = INFINITY;
		const float noSplitCost = 1.0f * (float)count * boxArea(nd.lo, nd.hi);
		int minIdx = 1;
		for(int b = 1; b < nBins; b++) {
			const float cost = (S.lcnt[b - 1] ? boxArea(&S.lbox[b - 1][0], &S.lbox[b - 1][3]) * (float)S.lcnt[b - 1] : 0.0f) +
							   (S.rcnt[b] ? boxArea(&S.rbox[b][0], &S.rbox[b][3]) * (float)S.rcnt[b] : 0.0f);
			if(cost < minCost) { minCost = cost; minIdx = b; }
		}
		minCost = 0.0f + 1.0f * minCost;
		S.leaf = noSplitCost < minCost ? 1 : 0;
		S.minIdx = minIdx;
	}
	__syncthreads();
	if(S.leaf) {
		if(tid == 0) {
			A.tn[t].inner = 0; A.tn[t].aux = count;
			atomicMax(&A.hdr->depth, nd.sdepth);
		}
		return;
	}
	const int minIdx = S.minIdx;
	int L = S.lcnt[minIdx - 1], R = S.rcnt[minIdx];
	if(L != 0 && R != 0) {
		// std::partition in libstdc++'s bidirectional form, closed: the k-th (ascending) element before L that fails the predicate swaps
		// with the k-th (descending) element from L on that satisfies it; everything else stays
		int carry = 0;
		for(int base = 0; base < count; base += T) {
			const int i = base + tid;
			const bool p = i < count && A.binE[first + i] < minIdx;
			const u64 bal = __ballot(p);
			int pre = __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0));
			int tot = __popcll(bal);
			if(T > 64) {
				const int w = tid >> 6;
				if((tid & 63) == 0) S.wsum[w] = tot;
				__syncthreads();
				tot = 0;
				for(int ww = 0; ww < T / 64; ww++) { if(ww < w) pre += S.wsum[ww]; tot += S.wsum[ww]; }
				__syncthreads();
			}
			const int Ti = carry + pre;   // elements before i that satisfy the predicate
			if(i < count) {
				if(i == L) S.m = L - Ti;
				if(i < L && !p) A.tmpA[first + (i - Ti)] = i;
				else if(i >= L && p) A.tmpB[first + (L - Ti - 1)] = i;
			}
			carry += tot;
		}
		__syncthreads();
		const int m = S.m;
		for(int k = tid; k < m; k += T) {
			const int a = first + A.tmpA[first + k], b = first + A.tmpB[first + k];
			float *pa = A.box + (size_t)a * 6, *pb = A.box + (size_t)b * 6;
			for(int c = 0; c < 6; c++) { const float v = pa[c]; pa[c] = pb[c]; pb[c] = v; }
			const int s = A.src[a]; A.src[a] = A.src[b]; A.src[b] = s;
		}
		__syncthreads();
	} else {
		// median split over the (unmoved) order: [0, mid) and [mid, count), each an in-order union
		const int mid = count / 2;
		for(int i = tid; i < count; i += T) {
			const float *b = A.box + (size_t)(first + i) * 6;
			const int s = i >= mid ? 1 : 0;
			for(int k = 0; k < 3; k++) { keyMin(&S.mmin[s][k], b[k], i); keyMax(&S.mmax[s][k], b[3 + k], i); }
		}
		__syncthreads();
		L = mid; R = count - mid;
	}
	if(tid == 0) {
		float lb[6], rb[6];
		if(S.lcnt[minIdx - 1] != 0 && S.rcnt[minIdx] != 0) {
			for(int k = 0; k < 6; k++) { lb[k] = S.lbox[minIdx - 1][k]; rb[k] = S.rbox[minIdx][k]; }
		} else {
			for(int k = 0; k < 3; k++) {
				lb[k] = keyValue(S.mmin[0][k]); lb[3 + k] = keyValue(S.mmax[0][k]);
				rb[k] = keyValue(S.mmin[1][k]); rb[3 + k] = keyValue(S.mmax[1][k]);
			}
		}
		if(nd.sdepth + 1 > A.maxDepth) atomicMax(&A.hdr->status, 2);   // a leaf below would be deeper than maxDepth
		else {
			const int firstNode = lb[axis] == rb[axis] ? (lb[3 + axis] < rb[3 + axis] ? 0 : 1) : 0;   // the second assignment only
			const int c = atomicAdd(&A.hdr->nTemp, 2);
			for(int s = 0; s < 2; s++) {
				TNode ch;
				for(int k = 0; k < 3; k++) { ch.lo[k] = s ? rb[k] : lb[k]; ch.hi[k] = s ? rb[3 + k] : lb[3 + k]; }
				ch.first = s ? first + L : first;
				ch.count = s ? R : L;
				ch.aux = ch.count; ch.inner = 0;
				ch.chain = s ? 0 : nd.chain + 1;
				ch.pfirst = first; ch.pchain = nd.chain; ch.side = s;
				ch.sdepth = nd.sdepth + 1; ch.pad = 0;
				A.tn[c + s] = ch;
				if(ch.count < P::minSplit) atomicMax(&A.hdr->depth, ch.sdepth);
			}
			A.tn[t].inner = 1;
			A.tn[t].aux = (int)((unsigned)axis | ((unsigned)firstNode << 16));
			atomicAdd(&A.startCnt[first], 1);
			S.child = c; S.cL = L; S.cR = R;
		}
	}
	__syncthreads();
}

// levels [level0, level1) of the nodes of more than 64 elements.  One level per launch while a level can be wide; the deep tail, where
// only degenerate fields still have such nodes, is ONE workgroup that takes the remaining levels in turn (level1 > level0 + 1 only with
// a grid of 1: the barrier between levels is the workgroup's own)
template <class P>
__global__ void __launch_bounds__(256) k_build_big(SplitArgs A, int level0, int level1) {
	__shared__ SplitLds S;
	__shared__ int levelCount;
#define SNAIL_BODY_BLOCK blockIdx.x
#define SNAIL_BODY_GRID gridDim.x
#include "build_big_body.inc"
#undef SNAIL_BODY_BLOCK
#undef SNAIL_BODY_GRID
}

template <class P>
__global__ void __launch_bounds__(64) k_build_small(SplitArgs A) {
	__shared__ SplitLds S;
	__shared__ int stack[kLevels + 8];
#define SNAIL_BODY_BLOCK blockIdx.x
#define SNAIL_BODY_GRID gridDim.x
#include "build_small_body.inc"
#undef SNAIL_BODY_BLOCK
#undef SNAIL_BODY_GRID
}

// startCnt[i] := number of inner nodes whose first slot is < i; totalInner (one workgroup of 1024 threads per tree)
__device__ __forceinline__ void buildScanBody(const SplitArgs &A, int *s) {
	BuildHdr &H = *A.hdr;
	if(H.status != 0) return;
	const int tid = threadIdx.x;
	int carry = 0;
	for(int base = 0; base < A.n; base += 1024) {
		const int i = base + tid;
		const int v = i < A.n ? A.startCnt[i] : 0;
		s[tid] = v;
		__syncthreads();
		for(int off = 1; off < 1024; off <<= 1) {
			const int x = tid >= off ? s[tid - off] : 0;
			__syncthreads();
			s[tid] += x;
			__syncthreads();
		}
		if(i < A.n) A.startCnt[i] = carry + s[tid] - v;
		carry += s[1023];
		__syncthreads();
	}
	if(tid == 0) H.totalInner = carry;
}
__global__ void __launch_bounds__(1024) k_build_scan(SplitArgs A) {
	__shared__ int s[1024];
	buildScanBody(A, s);
}

} // namespace devb

// ---- host side ----
namespace {

size_t buildScratchBytes(int cap) {
	const size_t N = (size_t)cap;
	return 256 * 12 + sizeof(devb::BuildHdr) + N * 24 + 5 * N * 4 + 2 * N * sizeof(devb::TNode) + 2 * (N / 65 + 2) * 4 + (N / 2 + 2) * 4;
}

// the scratch of a build over up to `cap` elements, carved out of the handle's allocation of buildScratchBytes(cap)
void buildCarve(char *base, int cap, devb::SplitArgs &A) {
	const size_t N = (size_t)cap;
	auto take = [&](size_t bytes) { char *p = base; base += (bytes + 255) & ~(size_t)255; return p; };
	A.hdr = (devb::BuildHdr *)take(sizeof(devb::BuildHdr));
	A.tn = (devb::TNode *)take(2 * N * sizeof(devb::TNode));
	A.box = (float *)take(N * 24);
	A.src = (int *)take(N * 4);
	A.binE = (int *)take(N * 4);
	A.tmpA = (int *)take(N * 4);
	A.tmpB = (int *)take(N * 4);
	A.startCnt = (int *)take(N * 4);
	A.queue[0] = (int *)take((N / 65 + 2) * 4);
	A.queue[1] = (int *)take((N / 65 + 2) * 4);
	A.small = (int *)take((N / 2 + 2) * 4);
}

} // namespace
