// wide.inc -- BVH::WideTrace (src/bvh/traverse.cpp:197-225) with one ray per lane, and the photon records of TracePhotons
// (src/photons.cpp:242-249) with their stable compaction.  The C-ABI is include/snail_wide.h, the host side wide_host.inc.
//
// Everything here is scalar IEEE fp32 -- BBox::WideTest (src/bounding_box.cpp:258-326) and Triangle::Collide<0> (src/triangle.h:139-164)
// use mul, sub, the selects a < b ? a : b / a > b ? a : b, one 1 / x, one sqrt and one divide -- so the file is compiled ONCE, outside
// the two arithmetic namespaces: what it computes does not depend on SNAIL_ARITH_*.  (The build's -ffp-contract=off keeps every mul and
// add separately rounded; divide and sqrt are correctly rounded; denormals are kept.)
//
// The reference's index lists only batch rays: for ONE ray the recursion is fixed -- left child's box, the left subtree to its end, the
// right child's box against the distance as it is then, the right subtree -- so a lane that keeps the right siblings still to be tested
// on a private stack walks exactly what the reference walks for that ray, whatever its neighbours do.  The stack lives in dynamic LDS as
// [slot][lane]: byte address (slot * 64 + lane) * 4, bank lane % 32 whatever slot each lane is on.
namespace devw {

struct WideArgs {
	const uint4 *nodes, *tris;          // the handle's own 32 B / 64 B records
	int nNodes, nTris;
	const float *origin, *dir, *idir;   // [nRays][3]; idir null = 1 / dir
	const int *indices;                 // n ray numbers, or null: ray i
	int n, nRays;
	float *dist;                        // [nRays], in / out
	int startNode, slots;               // slots = stack entries per lane (the tree's depth)
	int *visits;                        // [nRays][2] {box tests, triangle tests} or null
	unsigned long long *stats;          // [2] += the same, or null
};

// veclib's Min / Max (veclib/vecbase.h:75-76), which is also what minps / maxps compute: the SECOND operand on NaN and on +-0
__device__ __forceinline__ float selMin(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float selMax(float a, float b) { return a > b ? a : b; }

// BBox::WideTest for one ray (the 4-wide body and the scalar tail are the same operations)
__device__ __forceinline__ bool wideTest(const uint4 n0, const uint4 n1, float ox, float oy, float oz, float ix, float iy, float iz, float dist) {
	const float bminx = __uint_as_float(n0.x), bminy = __uint_as_float(n0.y), bminz = __uint_as_float(n0.z);
	const float bmaxx = __uint_as_float(n0.w), bmaxy = __uint_as_float(n1.x), bmaxz = __uint_as_float(n1.y);
	float l1 = ix * (bminx - ox), l2 = ix * (bmaxx - ox);
	float lmin = selMin(l1, l2), lmax = selMax(l1, l2);
	l1 = iy * (bminy - oy); l2 = iy * (bmaxy - oy);
	lmin = selMax(selMin(l1, l2), lmin); lmax = selMin(selMax(l1, l2), lmax);
	l1 = iz * (bminz - oz); l2 = iz * (bmaxz - oz);
	lmin = selMax(selMin(l1, l2), lmin); lmax = selMin(selMax(l1, l2), lmax);
	return lmax >= 0.0f && lmin <= selMin(lmax, dist);
}

// Triangle::Collide<0>: the edges are P2() - P1() = (ba + a) - a and P3() - P1(), NOT the stored ba / ca (the locals of that name hide the
// members from their declaration to the end of the function: the normal AND the two cross products of u, v take them); the normal and
// its length are recomputed, the stored plane / t0 are not read.  No t > 0 test: a triangle behind the origin gives a negative distance.
__device__ __forceinline__ float collide0(const uint4 q0, const uint4 q1, const uint4 q2, float ox, float oy, float oz, float dx, float dy, float dz) {
	const float ax = __uint_as_float(q0.x), ay = __uint_as_float(q0.y), az = __uint_as_float(q0.z);
	const float bx = (__uint_as_float(q0.w) + ax) - ax, by = (__uint_as_float(q1.x) + ay) - ay, bz = (__uint_as_float(q1.y) + az) - az;
	const float cx = (__uint_as_float(q1.z) + ax) - ax, cy = (__uint_as_float(q1.w) + ay) - ay, cz = (__uint_as_float(q2.x) + az) - az;
	float nx = by * cz - bz * cy, ny = bz * cx - bx * cz, nz = bx * cy - by * cx;
	const float t0 = sqrtf(nx * nx + ny * ny + nz * nz);
	const float inv = 1.0f / t0;
	nx *= inv; ny *= inv; nz *= inv;
	const float det = dx * nx + dy * ny + dz * nz;
	const float tx = ox - ax, ty = oy - ay, tz = oz - az;
	const float u = dx * (by * tz - bz * ty) + dy * (bz * tx - bx * tz) + dz * (bx * ty - by * tx);
	const float v = dx * (ty * cz - tz * cy) + dy * (tz * cx - tx * cz) + dz * (tx * cy - ty * cx);
	const bool test = selMin(u, v) >= 0.0f && u + v <= det * t0;
	const float d = -(tx * nx + ty * ny + tz * nz) / det;
	return test ? d : __uint_as_float(0x7f800000u);
}

__device__ __forceinline__ unsigned long long waveSum(unsigned long long v) {
	for(int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
	return v;
}

// One ray per lane, one wave per workgroup; a wave ends when its last lane does.  No communication between workgroups.
__global__ __launch_bounds__(64) void k_wide_trace(const WideArgs A) {
	extern __shared__ __attribute__((aligned(16))) int wideStack[];   // [A.slots][64]
	const int lane = threadIdx.x;
	const long long i = (long long)blockIdx.x * 64 + lane;
	int ray = -1;
	if(i < A.n) {
		ray = A.indices ? A.indices[i] : (int)i;
		if((unsigned)ray >= (unsigned)A.nRays) ray = -1;   // (a number outside the ray arrays names no ray)
	}
	int nBox = 0, nTri = 0;
	if(ray >= 0) {
		const float ox = A.origin[3 * (size_t)ray], oy = A.origin[3 * (size_t)ray + 1], oz = A.origin[3 * (size_t)ray + 2];
		const float dx = A.dir[3 * (size_t)ray], dy = A.dir[3 * (size_t)ray + 1], dz = A.dir[3 * (size_t)ray + 2];
		float ix, iy, iz;
		if(A.idir) { ix = A.idir[3 * (size_t)ray]; iy = A.idir[3 * (size_t)ray + 1]; iz = A.idir[3 * (size_t)ray + 2]; }
		else { ix = 1.0f / dx; iy = 1.0f / dy; iz = 1.0f / dz; }
		float dist = A.dist[ray];
		int sp = 0;
		unsigned next = (unsigned)A.startNode;
		bool test = false;   // the start node's own box is not tested
		for(;;) {
			if(next >= (unsigned)A.nNodes) break;   // (records that point outside the arrays are not followed)
			const uint4 n0 = A.nodes[2 * (size_t)next], n1 = A.nodes[2 * (size_t)next + 1];
			bool pass = true;
			if(test) { nBox++; pass = wideTest(n0, n1, ox, oy, oz, ix, iy, iz, dist); }
			test = true;
			if(pass) {
				if(n1.z & 0x80000000u) {
					const unsigned first = n1.z & 0x7fffffffu;
					unsigned count = (int)n1.w > 0 ? n1.w : 0u;
					if(first >= (unsigned)A.nTris) count = 0;
					else if(count > (unsigned)A.nTris - first) count = (unsigned)A.nTris - first;
					for(unsigned t = 0; t < count; t++) {
						const uint4 *T = A.tris + 4 * (size_t)(first + t);
						const float d = collide0(T[0], T[1], T[2], ox, oy, oz, dx, dy, dz);
						dist = dist < d ? dist : d;   // the select: a NaN d replaces dist, a NaN dist is replaced by the next d
						nTri++;
					}
				} else if(sp < A.slots) {
					wideStack[sp * 64 + lane] = (int)(n1.z + 1u);   // the right sibling waits for the left subtree
					sp++;
					next = n1.z;
					continue;
				} else break;   // (deeper than the depth the handle declared: cannot happen in a tree snail_scene_create accepted)
			}
			if(sp == 0) break;
			sp--;
			next = (unsigned)wideStack[sp * 64 + lane];
		}
		A.dist[ray] = dist;
		if(A.visits) { A.visits[2 * (size_t)ray] = nBox; A.visits[2 * (size_t)ray + 1] = nTri; }
	}
	if(A.stats) {
		const unsigned long long b = waveSum((unsigned long long)nBox), t = waveSum((unsigned long long)nTri);
		if(lane == 0) { atomicAdd(A.stats, b); atomicAdd(A.stats + 1, t); }
	}
}

// ---- photon records ----
// struct Photon (src/photons.h:7-24), 32 bytes: position, direction, colour bytes, temp
struct PhotonArgs {
	const float *origin, *dir, *dist;   // [n][3], [n][3], [n]
	int n, count;                       // n = nLights * count rays, light-major
	unsigned colour[8];                 // per light: the three colour bytes (byte 3 = 0), converted on the host
	unsigned *blockCount;               // [blocks + 1]: counts, then (after the scan) exclusive offsets
	int nBlocks;
	unsigned *photons;                  // [..][8] words
	int *nPhotons;
};

enum { kPhotonBlock = 256 };

// temp = dist == +inf ? 0 : 1 (a NaN distance keeps its record, as in the reference)
__device__ __forceinline__ bool photonKept(const PhotonArgs &A, int i) { return i < A.n && !(A.dist[i] == __uint_as_float(0x7f800000u)); }

// stage 1: how many records each block of 256 rays keeps
__global__ __launch_bounds__(kPhotonBlock) void k_photon_flag(const PhotonArgs A) {
	const int i = blockIdx.x * kPhotonBlock + threadIdx.x;
	const int kept = __syncthreads_count(photonKept(A, i) ? 1 : 0);
	if(threadIdx.x == 0) A.blockCount[blockIdx.x] = (unsigned)kept;
}

// stage 2: ONE workgroup turns the block counts into exclusive offsets, 1024 at a time with a running carry, and writes the total
__global__ __launch_bounds__(1024) void k_photon_scan(const PhotonArgs A) {
	__shared__ unsigned waveTotal[16];
	__shared__ unsigned carryS;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	if(tid == 0) carryS = 0;
	__syncthreads();
	for(int base = 0; base < A.nBlocks; base += 1024) {
		const int b = base + tid;
		const unsigned own = b < A.nBlocks ? A.blockCount[b] : 0u;
		unsigned incl = own;
		for(int off = 1; off < 64; off <<= 1) {
			const unsigned up = __shfl_up(incl, off, 64);
			if(lane >= off) incl += up;
		}
		if(lane == 63) waveTotal[wave] = incl;
		__syncthreads();
		unsigned before = carryS;
		for(int w = 0; w < wave; w++) before += waveTotal[w];
		if(b < A.nBlocks) A.blockCount[b] = before + incl - own;
		__syncthreads();
		if(tid == 1023) carryS = before + incl;
		__syncthreads();
	}
	if(tid == 0) *A.nPhotons = (int)carryS;
}

// stage 3: every kept ray writes its record at its block's offset + its rank among the block's kept rays (ray order: remove_if is stable)
__global__ __launch_bounds__(kPhotonBlock) void k_photon_scatter(const PhotonArgs A) {
	__shared__ unsigned waveKept[kPhotonBlock / 64];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int i = blockIdx.x * kPhotonBlock + tid;
	const bool kept = photonKept(A, i);
	const unsigned long long mask = __ballot(kept);
	if(lane == 0) waveKept[wave] = (unsigned)__popcll(mask);
	__syncthreads();
	if(!kept) return;
	unsigned at = A.blockCount[blockIdx.x] + (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
	for(int w = 0; w < wave; w++) at += waveKept[w];
	const float d = A.dist[i];
	const float ox = A.origin[3 * (size_t)i], oy = A.origin[3 * (size_t)i + 1], oz = A.origin[3 * (size_t)i + 2];
	const float dx = A.dir[3 * (size_t)i], dy = A.dir[3 * (size_t)i + 1], dz = A.dir[3 * (size_t)i + 2];
	unsigned *P = A.photons + 8 * (size_t)at;
	P[0] = __float_as_uint(ox + dx * d); P[1] = __float_as_uint(oy + dy * d); P[2] = __float_as_uint(oz + dz * d);   // origin + dir * dist
	P[3] = __float_as_uint(dx); P[4] = __float_as_uint(dy); P[5] = __float_as_uint(dz);
	P[6] = A.colour[i / A.count];
	P[7] = 1u;
}

} // namespace devw
