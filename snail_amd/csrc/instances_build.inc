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
// The split itself (keys, splitNode, k_build_root / big / small / scan) is shared with the triangle builder: build_common.inc.
namespace devb {

struct BuildArgs : SplitArgs {
	const float *xf; const int *blasIdx; int nBlas; const float *blasBox;
	uint4 *top, *inst; int *cur; int *perm, *info;
	int seed, seedNodes, seedN;
};


__global__ void k_build_init(BuildArgs A) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if(i < A.n) A.startCnt[i] = 0;
	if(i == 0) {
		hdrInit(*A.hdr);
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
