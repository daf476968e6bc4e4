// instances_build.inc -- DBVH::Construct on the device (include/snail_instances_build.h): the kernels behind snail_instances_rebuild_dev.
// Bit-equal to dbvh_build.cpp, whose fp32 operation order every expression here repeats (plain fp32, -ffp-contract=off, IEEE division,
// denormals kept); it uses neither Inv nor RSqrt, so it exists once and not per arithmetic.  Host side: instances_host.inc.
//
// ORDERED MIN / MAX.  fmin2(a, b) = a < b ? a : b returns its SECOND operand on a tie, so the fold acc = fmin2(acc, x_i) over i = 0..k ends at
// x_j with j the LARGEST index among the numerically smallest values (the first of them replaces acc, every later equal one replaces it
// again, nothing larger does); +0 and -0 are such equal values with different bytes.  That is the lexicographic minimum of (value with
// -0 == +0, index descending), which fits one 64-bit integer: [monotone image of the value : 32][0x7fffffff - index : 31][sign bit : 1].
// An integer minimum over those keys does not depend on the order in which it is taken, so it may be taken with integer atomics;
// fmax2 likewise with [value][index][sign] and an integer maximum.  (A float atomic min or an unordered float reduction would lose
// exactly the index.)  Bins start at (+inf, -inf), which is the key of an element that loses to every finite value and ties with an
// infinite one to the same bytes.  The equivalence holds for boxes without NaN; finite transforms over finite BLAS boxes give those
// unless a product overflows to inf - inf, which the host builder does not define either.
//
// PHASES (kernel boundaries on one stream; inside a kernel only workgroup barriers):
//   k_build_init   counters, per-slot inner-node counts := 0
//   k_build_boxes  validation (before an input value indexes anything), ObjectInstance::ComputeBBox per instance, root box keys
//   k_build_root   temporary node 0
//   k_build_big    level L splits the nodes of depth L that hold more than 64 instances, one 256-thread workgroup per node; children of
//                  <= 64 instances go on the small list.  One launch per level for levels 0..15, then one single-workgroup launch that
//                  takes levels 16..64 in turn (only degenerate fields have such nodes that deep)
//   k_build_small  one wave per small-list entry finishes that whole subtree with a stack in LDS
//   k_build_scan   exclusive prefix sum of the inner-node counts by first slot
//   k_build_commit final numbering + the packed instance records into the handle's buffers, only when status == 0
// Sizes: n == 1 (root leaf), 2..64 (root straight onto the small list), > 64 (big levels, then small subtrees).
//
// NUMBERING.  The host numbers children when their parent is split and finishes the left subtree first, so an inner node's `sub` is
// 1 + 2 * (its rank among the inner nodes in pre-order).  Inner nodes have nested or disjoint slot ranges and both children non-empty, so
// pre-order is (first slot ascending, then depth): rank = (inner nodes whose first slot is smaller) + (inner ancestors with the same first
// slot).  The second term (`chain`) is known when the node is made: a left child continues its parent's chain, a right child starts one.
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
	int status, depth, nTemp, nSmall, totalInner, pad[3];
	u64 rootMin[3], rootMax[3];
	int qCount[kLevels + 3];
};

struct BuildArgs {
	const float *xf; const int *blasIdx; int n, nBlas; const float *blasBox;
	float *box; int *src, *binE, *tmpA, *tmpB, *startCnt;
	TNode *tn; int *queue[2]; int *small;
	BuildHdr *hdr;
	uint4 *top, *inst; int *cur; int *perm, *info;
	int seed, seedNodes, seedN;
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

__global__ void k_build_init(BuildArgs A) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if(i < A.n) A.startCnt[i] = 0;
	if(i == 0) {
		BuildHdr &H = *A.hdr;
		H.status = 0; H.depth = 0; H.nTemp = 0; H.nSmall = 0; H.totalInner = 0;
		for(int k = 0; k < 3; k++) { H.rootMin[k] = SNAIL_KEY_MIN_INIT; H.rootMax[k] = SNAIL_KEY_MAX_INIT; }
		for(int k = 0; k < kLevels + 3; k++) H.qCount[k] = 0;
		if(A.seed) { A.cur[0] = A.seedNodes; A.cur[1] = A.seedN; }   // what the host's last snail_instances_update left
	}
}

// ObjectInstance::ComputeBBox (src/dbvh/tree.cpp:4-21) as dbvh_build.cpp's instanceBox has it
__global__ void k_build_boxes(BuildArgs A) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= A.n) return;
	float x[12];
	bool ok = true;
	for(int k = 0; k < 12; k++) { x[k] = A.xf[(size_t)i * 12 + k]; ok = ok && finiteBits(x[k]); }
	const int bi = A.blasIdx ? A.blasIdx[i] : 0;
	ok = ok && bi >= 0 && bi < A.nBlas;
	if(!ok) { atomicMax(&A.hdr->status, 1); return; }
	float b6[6];
	for(int k = 0; k < 6; k++) b6[k] = A.blasBox[(size_t)bi * 6 + k];
	const float x0 = b6[0], x1 = b6[3];
	const float y[4] = {b6[1], b6[1], b6[4], b6[4]}, z[4] = {b6[2], b6[5], b6[2], b6[5]};
	float lo[3], hi[3];
	for(int c = 0; c < 3; c++) {
		const float *r = x + c * 3;
		float mn[4], mx[4];
		for(int l = 0; l < 4; l++) {
			float p0 = y[l] * r[1] + z[l] * r[2];
			const float p1 = x1 * r[0] + p0;
			p0 = p0 + x0 * r[0];
			mn[l] = fmin2(p0, p1);
			mx[l] = fmax2(p0, p1);
		}
		lo[c] = fmin2(fmin2(mn[0], mn[1]), fmin2(mn[2], mn[3])) + x[9 + c];
		hi[c] = fmax2(fmax2(mx[0], mx[1]), fmax2(mx[2], mx[3])) + x[9 + c];
	}
	float *o = A.box + (size_t)i * 6;
	for(int k = 0; k < 3; k++) { o[k] = lo[k]; o[3 + k] = hi[k]; }
	A.src[i] = i;
	// the root box: box[0] grown by 1..n-1 in the caller's order
	for(int k = 0; k < 3; k++) { keyMin(&A.hdr->rootMin[k], lo[k], i); keyMax(&A.hdr->rootMax[k], hi[k], i); }
}

__global__ void k_build_root(BuildArgs A) {
	BuildHdr &H = *A.hdr;
	if(threadIdx.x != 0 || blockIdx.x != 0 || H.status != 0) return;
	TNode r;
	for(int k = 0; k < 3; k++) { r.lo[k] = keyValue(H.rootMin[k]); r.hi[k] = keyValue(H.rootMax[k]); }
	r.first = 0; r.count = A.n; r.aux = A.n; r.inner = 0; r.chain = 0; r.pfirst = 0; r.pchain = 0; r.side = 0; r.sdepth = 0; r.pad = 0;
	A.tn[0] = r;
	H.nTemp = 1;
	if(A.n > kSmall) { A.queue[0][0] = 0; H.qCount[0] = 1; }
	else if(A.n >= 2) { A.small[0] = 0; H.nSmall = 1; }
}

struct SplitLds {
	u64 bmin[16][3], bmax[16][3];
	u64 mmin[2][3], mmax[2][3];
	float lbox[16][6], rbox[16][6];
	int bcnt[16], lcnt[16], rcnt[16];
	int wsum[4];
	int minIdx, leaf, m;
	int child, cL, cR;       // the children made (child < 0: none) and their counts
};

// DBVH::FindSplit for the node tn[t] of at least two instances, by the T threads of one workgroup (T = 64: one wave)
template <int T>
__device__ void splitNode(const BuildArgs &A, int t, SplitLds &S) {
	const int tid = threadIdx.x;
	const TNode nd = A.tn[t];
	const int first = nd.first, count = nd.count;
	float size[3];
	for(int k = 0; k < 3; k++) size[k] = nd.hi[k] - nd.lo[k];
	const int axis = size[1] > size[0] ? (size[2] > size[1] ? 2 : 1) : (size[2] > size[0] ? 2 : 0);
	const int nBins = count < 8 ? 8 : 16;
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
		if(nd.sdepth + 1 > kMaxDepth) atomicMax(&A.hdr->status, 2);   // a leaf below would be deeper than DBVH::maxDepth
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
				if(ch.count <= 1) atomicMax(&A.hdr->depth, ch.sdepth);
			}
			A.tn[t].inner = 1;
			A.tn[t].aux = (int)((unsigned)axis | ((unsigned)firstNode << 16));
			atomicAdd(&A.startCnt[first], 1);
			S.child = c; S.cL = L; S.cR = R;
		}
	}
	__syncthreads();
}

// levels [level0, level1) of the nodes of more than 64 instances.  One level per launch while a level can be wide; the deep tail, where
// only degenerate fields still have such nodes, is ONE workgroup that takes the remaining levels in turn (level1 > level0 + 1 only with
// a grid of 1: the barrier between levels is the workgroup's own)
__global__ void __launch_bounds__(256) k_build_big(BuildArgs A, int level0, int level1) {
	__shared__ SplitLds S;
	__shared__ int levelCount;
	BuildHdr &H = *A.hdr;
	if(H.status == 1) return;
	for(int level = level0; level < level1; level++) {
		__syncthreads();
		if(threadIdx.x == 0) levelCount = atomicAdd(&H.qCount[level], 0);   // (read where this workgroup's own atomics of the level before landed)
		__syncthreads();
		const int cnt = levelCount;
		if(cnt == 0) return;      // no node of this depth: none deeper either
		const int *in = A.queue[level & 1];
		int *out = A.queue[(level + 1) & 1];
		for(int item = blockIdx.x; item < cnt; item += gridDim.x) {
			__syncthreads();
			splitNode<256>(A, in[item], S);
			if(threadIdx.x == 0 && S.child >= 0) {
				const int id[2] = {S.child, S.child + 1}, c[2] = {S.cL, S.cR};
				for(int s = 0; s < 2; s++) {
					if(c[s] > kSmall) out[atomicAdd(&H.qCount[level + 1], 1)] = id[s];
					else if(c[s] >= 2) A.small[atomicAdd(&H.nSmall, 1)] = id[s];
				}
			}
		}
	}
}

__global__ void __launch_bounds__(64) k_build_small(BuildArgs A) {
	__shared__ SplitLds S;
	__shared__ int stack[kLevels + 8];
	BuildHdr &H = *A.hdr;
	if(H.status == 1) return;
	const int cnt = H.nSmall;
	for(int item = blockIdx.x; item < cnt; item += gridDim.x) {
		__syncthreads();
		if(threadIdx.x == 0) stack[0] = A.small[item];
		int sp = 1;
		while(sp > 0) {
			__syncthreads();
			const int t = stack[--sp];
			__syncthreads();
			splitNode<64>(A, t, S);
			// (the children of a node at depth d sit at d + 1 <= 64 and none is made below that: at most one pending sibling per level)
			const int c = S.child;
			if(c >= 0) {
				if(S.cR >= 2 && sp < kLevels + 6) { if(threadIdx.x == 0) stack[sp] = c + 1; sp++; }
				if(S.cL >= 2 && sp < kLevels + 6) { if(threadIdx.x == 0) stack[sp] = c; sp++; }
			}
		}
	}
}

// startCnt[i] := number of inner nodes whose first slot is < i; totalInner
__global__ void __launch_bounds__(1024) k_build_scan(BuildArgs A) {
	__shared__ int s[1024];
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

// the commit: nodes under their final numbers and the packed 64-byte instance records (packInstances), only for a tree that stands
__global__ void k_build_commit(BuildArgs A) {
	const BuildHdr &H = *A.hdr;
	const int g = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
	if(H.status != 0) {
		if(g == 0 && A.info) { A.info[0] = H.status; A.info[1] = 0; A.info[2] = 0; A.info[3] = A.n; }
		return;
	}
	const int nTemp = H.nTemp;
	for(int t = g; t < nTemp; t += stride) {
		const TNode nd = A.tn[t];
		const int idx = t == 0 ? 0 : 1 + 2 * (A.startCnt[nd.pfirst] + nd.pchain) + nd.side;
		const unsigned sub = nd.inner ? (unsigned)(1 + 2 * (A.startCnt[nd.first] + nd.chain)) : ((unsigned)nd.first | 0x80000000u);
		A.top[(size_t)idx * 2] = make_uint4(__float_as_uint(nd.lo[0]), __float_as_uint(nd.lo[1]), __float_as_uint(nd.lo[2]), __float_as_uint(nd.hi[0]));
		A.top[(size_t)idx * 2 + 1] = make_uint4(__float_as_uint(nd.hi[1]), __float_as_uint(nd.hi[2]), sub, (unsigned)nd.aux);
	}
	for(int i = g; i < A.n; i += stride) {
		const int s = A.src[i];
		const unsigned *x = (const unsigned *)A.xf + (size_t)s * 12;
		const unsigned bi = A.blasIdx ? (unsigned)A.blasIdx[s] : 0u;
		uint4 *o = A.inst + (size_t)i * 4;
		o[0] = make_uint4(x[0], x[1], x[2], bi);
		o[1] = make_uint4(x[3], x[4], x[5], 0);
		o[2] = make_uint4(x[6], x[7], x[8], 0);
		o[3] = make_uint4(x[9], x[10], x[11], 0);
		if(A.perm) A.perm[i] = s;
	}
	if(g == 0) {
		const int nNodes = 1 + 2 * H.totalInner;
		A.cur[0] = nNodes; A.cur[1] = A.n;
		if(A.info) { A.info[0] = 0; A.info[1] = nNodes; A.info[2] = H.depth; A.info[3] = A.n; }
	}
}

} // namespace devb
