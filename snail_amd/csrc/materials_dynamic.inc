// materials_dynamic.inc -- the ShTriangle records of a material set written on the device (include/snail_materials_dynamic.h): what
// snail_shtris_pack computes on the host, one thread per record, from input-order data in device memory through the permutation of the
// tree the handle holds.  Plain fp32 (this TU: -ffp-contract=off, IEEE divide / sqrt, denormals kept), so it exists once and not per
// arithmetic, as bvh_fast.inc.  HBM-bound gathers: <= 65 bytes read (24 uv + 36 normals or vertices + 4 + 1) and 64 written per triangle.
//   k_shd_check   creation only: uv finite and below 2^20, matIdx inside the map, perm inside the triangles -> the first offender
//   k_shd_pack    record i <- input triangle perm[i]; under a rebuild only when the build's status word (k_fast_commit's info) is 0
//   k_shd_info    the caller's info words, after the pack (one thread)
// The per-record body and the info words are __device__ functions: the batched kernels of instances_materials_dynamic.inc call the same ones.
namespace devshd {

struct PackArgs {
	const float *uv6;              // the set's copies, input order
	const int *matIdx;
	const unsigned char *flat;     // (null: none flat)
	const float *nrm9, *verts9;    // the caller's: per-vertex normals, or (nrm9 null) the vertices face normals come from
	const int *perm;               // slot -> input triangle
	const int *build;              // k_fast_commit's {status, nNodes, depth, n} (null: there was no build -- always commit)
	uint4 *shtris;
	int *permOut;                  // (null: none) [n], receives perm whether or not the records are committed
	int *zeroed;                   // += triangles whose normals were replaced by zeros
	int *check;                    // k_shd_check: {code, first offender}
	int *info;                     // k_shd_info: the caller's words (null: none)
	int n, nMap;
};

__device__ __forceinline__ bool finiteBits(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__global__ void k_shd_check(PackArgs A) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= A.n) return;
	int code = 0;
	for(int k = 0; k < 6; k++)
		if(!(fabsf(A.uv6[(size_t)i * 6 + k]) < 1048576.0f)) code = 1;
	const int mi = A.matIdx[i];
	if(!code && (mi < 0 || mi >= A.nMap)) code = 2;
	if(!code && (unsigned)A.perm[i] >= (unsigned)A.n) code = 3;
	if(code) { atomicMax(&A.check[0], code); atomicMin(&A.check[1], i); }
}

// record i of one set (i < A.n): the ONE body of k_shd_pack and of the batched devshd::k_ishd_pack (instances_materials_dynamic.inc)
__device__ __forceinline__ void shdPackRecord(const PackArgs &A, const int i) {
	const int src = A.perm[i];
	if(A.permOut) A.permOut[i] = src;
	if(A.build && A.build[0] != 0) return;   // the tree was not committed: neither are the records
	uint4 *o = A.shtris + (size_t)i * 4;
	if((unsigned)src >= (unsigned)A.n) {
		atomicAdd(A.zeroed, 1);
		for(int q = 0; q < 4; q++) o[q] = make_uint4(0u, 0u, 0u, 0u);
		return;
	}
	float nr[9];
	if(A.nrm9) {
		for(int k = 0; k < 9; k++) nr[k] = A.nrm9[(size_t)src * 9 + k];
	} else {
		// BaseScene::Object::GetTriangle (src/base_scene.cpp:313-314): fnrm = (p1 - p0) ^ (p2 - p0); fnrm *= RSqrt(fnrm | fnrm)
		float p[9];
		for(int k = 0; k < 9; k++) p[k] = A.verts9[(size_t)src * 9 + k];
		const float bx = p[3] - p[0], by = p[4] - p[1], bz = p[5] - p[2], cx = p[6] - p[0], cy = p[7] - p[1], cz = p[8] - p[2];
		float fx = by * cz - bz * cy, fy = bz * cx - bx * cz, fz = bx * cy - by * cx;
		const float r = 1.0f / __builtin_sqrtf(fx * fx + fy * fy + fz * fz);
		fx *= r; fy *= r; fz *= r;
		for(int v = 0; v < 3; v++) { nr[v * 3] = fx; nr[v * 3 + 1] = fy; nr[v * 3 + 2] = fz; }
	}
	bool fin = true;
	for(int k = 0; k < 9; k++) fin = fin && finiteBits(nr[k]);
	if(!fin) {
		atomicAdd(A.zeroed, 1);
		for(int k = 0; k < 9; k++) nr[k] = 0.0f;
	}
	float uv[6];
	for(int k = 0; k < 6; k++) uv[k] = A.uv6[(size_t)src * 6 + k];
	// the ShTriangle constructor (src/triangle.h:188-208), as snail_shtris_pack: elements 1 and 2 minus element 0
	float r[15];
	r[0] = uv[0]; r[1] = uv[1];
	r[2] = uv[2] - uv[0]; r[3] = uv[3] - uv[1];
	r[4] = uv[4] - uv[0]; r[5] = uv[5] - uv[1];
	for(int c = 0; c < 3; c++) { r[6 + c] = nr[c]; r[9 + c] = nr[3 + c] - nr[c]; r[12 + c] = nr[6 + c] - nr[c]; }
	const unsigned id = (unsigned)A.matIdx[src] | ((A.flat && A.flat[src]) ? 0x80000000u : 0u);
	for(int q = 0; q < 3; q++) o[q] = make_uint4(__float_as_uint(r[q * 4]), __float_as_uint(r[q * 4 + 1]), __float_as_uint(r[q * 4 + 2]), __float_as_uint(r[q * 4 + 3]));
	o[3] = make_uint4(__float_as_uint(r[12]), __float_as_uint(r[13]), __float_as_uint(r[14]), id);
}

__global__ void k_shd_pack(PackArgs A) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= A.n) return;
	shdPackRecord(A, i);
}

// rebuild (build given): {status, nNodes, depth, n, committed, zeroed}; update: {1, zeroed}
__device__ __forceinline__ void shdInfoWords(const PackArgs &A) {
	if(!A.info) return;
	if(A.build) {
		for(int k = 0; k < 4; k++) A.info[k] = A.build[k];
		A.info[4] = A.build[0] == 0 ? 1 : 0;
		A.info[5] = *A.zeroed;
	} else {
		A.info[0] = 1;
		A.info[1] = *A.zeroed;
	}
}
__global__ void k_shd_info(PackArgs A) {
	if(blockIdx.x != 0 || threadIdx.x != 0) return;
	shdInfoWords(A);
}

} // namespace devshd
