// lbvh.inc -- GPU tree builder option (SURVEY.md section 8 f3), included by snail_hip.hip.
//
// A linear BVH in the reference's record formats (32-B BVH::Node, src/bvh/tree.h:60-72; 64-B Triangle, src/triangle.h:133-135), built
// and kept on the device: triangle records + Morton keys of the triangle-box centres (30 bits, index in the low word so that keys are
// unique), one device radix sort (rocPRIM), Karras' binary radix tree over the sorted keys (T. Karras, "Maximizing parallelism in the
// construction of BVHs, octrees and k-d trees", HPG 2012), bottom-up refit, subtrees of <= maxLeafTris triangles collapsed into leaves.
// It is NOT the parity tree: triangle order (= triId) and shape differ from BVH::Construct's SAH sweep, so it is reported separately;
// the traversal kernels are the same.
//
// Layout trick: the reference needs the two children of a node adjacent (subNode, subNode+1; src/bvh/tree.cpp:153-157).  Karras'
// internal node i (0 = root) gets its children at output slots 1+2i and 2+2i, so no re-layout pass is needed: the output array has
// 2n-1 slots, the root in slot 0; slots below a collapsed subtree stay unused (never referenced).
#include <rocprim/rocprim.hpp>

namespace dev {
namespace lbvh {

typedef unsigned long long u64;

struct Box { float mn[3], mx[3]; };

// order-preserving map float -> uint for atomicMin/atomicMax
__device__ __forceinline__ unsigned orderKey(float f) { unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float orderVal(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__global__ void k_scene_bounds(const float *verts, int n, unsigned *bounds /*6: min xyz, max xyz as order keys*/) {
	const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	float mn[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, mx[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
	if(i < n) {
		const float *p = verts + (size_t)i * 9;
		for(int v = 0; v < 3; v++)
			for(int c = 0; c < 3; c++) { mn[c] = fminf(mn[c], p[v * 3 + c]); mx[c] = fmaxf(mx[c], p[v * 3 + c]); }
	}
	for(int c = 0; c < 3; c++) { // wave reduction, then one atomic per wave
		for(int o = 32; o > 0; o >>= 1) { mn[c] = fminf(mn[c], __shfl_xor(mn[c], o)); mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], o)); }
		if((threadIdx.x & 63) == 0) { atomicMin(&bounds[c], orderKey(mn[c])); atomicMax(&bounds[3 + c], orderKey(mx[c])); }
	}
}

__device__ __forceinline__ unsigned spread10(unsigned v) { // 10 bits -> every third bit
	v = (v | (v << 16)) & 0x030000ffu;
	v = (v | (v << 8)) & 0x0300f00fu;
	v = (v | (v << 4)) & 0x030c30c3u;
	v = (v | (v << 2)) & 0x09249249u;
	return v;
}

__global__ void k_morton(const float *verts, int n, const unsigned *bounds, u64 *keys) {
	const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	if(i >= n) return;
	const float *p = verts + (size_t)i * 9;
	unsigned q[3];
	for(int c = 0; c < 3; c++) {
		const float lo = orderVal(bounds[c]), hi = orderVal(bounds[3 + c]);
		const float mn = fminf(p[c], fminf(p[3 + c], p[6 + c])), mx = fmaxf(p[c], fmaxf(p[3 + c], p[6 + c]));
		const float ext = hi - lo;
		float t = ext > 0.0f ? ((mn + mx) * 0.5f - lo) / ext : 0.0f;
		t = fminf(fmaxf(t, 0.0f), 1.0f);
		q[c] = (unsigned)fminf(t * 1024.0f, 1023.0f);
	}
	const unsigned code = (spread10(q[0]) << 2) | (spread10(q[1]) << 1) | spread10(q[2]);
	keys[i] = ((u64)code << 32) | (unsigned)i;
}

// one triangle record: the formulas of Triangle::Triangle + ComputeData (src/triangle.h:16-21,123-131), as in snail_tris_from_verts (this
// TU is built without FMA contraction, IEEE divide / sqrt); p = 9 floats of vertices, t = 16 floats.  Returns the sanity conditions of
// snail_scene_create (fast arithmetic modes need finite records of sane magnitude).  Shared with bvh_fast.inc
__device__ __forceinline__ bool triRecord(const float *p, float *t) {
	float a[3], ba[3], ca[3];
	for(int k = 0; k < 3; k++) { a[k] = p[k]; ba[k] = p[3 + k] - p[k]; ca[k] = p[6 + k] - p[k]; }
	float nx = ba[1] * ca[2] - ba[2] * ca[1];
	float ny = ba[2] * ca[0] - ba[0] * ca[2];
	float nz = ba[0] * ca[1] - ba[1] * ca[0];
	const float len = __builtin_sqrtf(nx * nx + ny * ny + nz * nz);
	const float inv = 1.0f / len;
	nx *= inv; ny *= inv; nz *= inv;
	t[0] = a[0]; t[1] = a[1]; t[2] = a[2]; t[3] = ba[0]; t[4] = ba[1]; t[5] = ba[2]; t[6] = ca[0]; t[7] = ca[1]; t[8] = ca[2];
	t[9] = len; t[10] = 1.0f / len; t[11] = 0.0f;
	t[12] = nx; t[13] = ny; t[14] = nz; t[15] = nx * a[0] + ny * a[1] + nz * a[2];
	bool ok = len > 0.0f && t[10] <= 1.0e12f && t[10] > 0.0f;
	for(int k = 0; k < 9; k++) ok = ok && fabsf(t[k]) <= 1.0e9f;
	for(int k = 12; k < 16; k++) ok = ok && fabsf(t[k]) <= 1.0e18f;
	return ok;
}

// triangle records in sorted order
__global__ void k_records(const float *verts, int n, const u64 *keys, float *tris /*16 floats each*/, int *perm, Box *leafBox, int *flags) {
	const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	if(j >= n) return;
	const int src = (int)(unsigned)(keys[j] & 0xffffffffull);
	const float *p = verts + (size_t)src * 9;
	Box b;
	for(int k = 0; k < 3; k++) { b.mn[k] = fminf(p[k], fminf(p[3 + k], p[6 + k])); b.mx[k] = fmaxf(p[k], fmaxf(p[3 + k], p[6 + k])); }
	const bool ok = triRecord(p, tris + (size_t)j * 16);
	perm[j] = src;
	leafBox[j] = b;
	if(!ok) atomicAnd(flags, 0);
}

__device__ __forceinline__ int delta(const u64 *keys, int n, int i, int j) {
	if(j < 0 || j >= n) return -1;
	return __clzll((long long)(keys[i] ^ keys[j]));
}

// Karras 2012, Algorithm 1.  child >= 0: internal node index; child < 0: leaf ~child
__global__ void k_topology(const u64 *keys, int n, int2 *children, int2 *range, int *parentInt, int *parentLeaf) {
	const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	if(i >= n - 1) return;
	const int d = delta(keys, n, i, i + 1) - delta(keys, n, i, i - 1) >= 0 ? 1 : -1;
	const int dmin = delta(keys, n, i, i - d);
	int lmax = 2;
	while(delta(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
	int l = 0;
	for(int t = lmax / 2; t >= 1; t /= 2)
		if(delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
	const int j = i + l * d;
	const int dnode = delta(keys, n, i, j);
	int s = 0;
	for(int t = (l + 1) / 2;; t = (t + 1) / 2) {
		if(delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
		if(t <= 1) break;
	}
	const int g = i + s * d + (d < 0 ? -1 : 0);
	const int lo = i < j ? i : j, hi = i < j ? j : i;
	const int left = (lo == g) ? ~g : g, right = (hi == g + 1) ? ~(g + 1) : g + 1;
	children[i] = make_int2(left, right);
	range[i] = make_int2(lo, hi);
	if(left >= 0) parentInt[left] = i; else parentLeaf[~left] = i;
	if(right >= 0) parentInt[right] = i; else parentLeaf[~right] = i;
	if(i == 0) parentInt[0] = -1;
}

// a box another thread of this launch has just written (ordered by its __threadfence + atomic on the parent's counter): read it
// past the CU's non-coherent L1
__device__ __forceinline__ Box loadBoxCoherent(const Box *p) {
	Box b;
	const float *f = (const float *)p;
	for(int k = 0; k < 3; k++) {
		b.mn[k] = __hip_atomic_load(f + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		b.mx[k] = __hip_atomic_load(f + 3 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
	return b;
}

__global__ void k_refit(int n, const int2 *children, const int *parentInt, const int *parentLeaf, const Box *leafBox, Box *intBox, int *visits) {
	const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	if(j >= n) return;
	int cur = parentLeaf[j];
	while(cur >= 0) {
		__threadfence();
		if(atomicAdd(&visits[cur], 1) == 0) return; // the second arrival owns the node
		const int2 c = children[cur];
		const Box a = c.x >= 0 ? loadBoxCoherent(intBox + c.x) : leafBox[~c.x];
		const Box b = c.y >= 0 ? loadBoxCoherent(intBox + c.y) : leafBox[~c.y];
		Box u;
		for(int k = 0; k < 3; k++) { u.mn[k] = fminf(a.mn[k], b.mn[k]); u.mx[k] = fmaxf(a.mx[k], b.mx[k]); }
		intBox[cur] = u;
		cur = parentInt[cur];
	}
}

// every slot starts as an empty leaf (no triangles, the zero box): the slots below a collapsed subtree are never referenced, but the
// array stays a valid input for snail_scene_create should a caller download and re-upload it
__global__ void k_fill_empty(float *nodes, int nSlots) {
	const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	if(i >= nSlots) return;
	float4 *o = (float4 *)(nodes + (size_t)i * 8);
	o[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	o[1] = make_float4(0.0f, 0.0f, __uint_as_float(0x80000000u), __int_as_float(0));
}

// the conditions snail_scene_create puts on a node's box before it allows the fast arithmetic modes: every emitted record passes through here
__host__ __device__ __forceinline__ bool boxSane(const Box &b) {
	bool ok = true;
	for(int k = 0; k < 3; k++) ok = ok && fabsf(b.mn[k]) <= 1.0e9f && fabsf(b.mx[k]) <= 1.0e9f && b.mn[k] <= b.mx[k];
	return ok;
}

__device__ __forceinline__ void writeNode(float *nodes, int slot, const Box &b, unsigned sub, int aux) {
	float4 *o = (float4 *)(nodes + (size_t)slot * 8);
	o[0] = make_float4(b.mn[0], b.mn[1], b.mn[2], b.mx[0]);
	o[1] = make_float4(b.mx[1], b.mx[2], __uint_as_float(sub), __int_as_float(aux));
}

// one thread per Karras node: an internal node with more than maxLeaf triangles becomes an inner output node and also emits those of
// its children that are leaves (single triangles, or collapsed subtrees); everything below a collapsed subtree is left unused
__global__ void k_emit(int n, int maxLeaf, const int2 *children, const int2 *range, const int *parentInt, const Box *leafBox, const Box *intBox,
					   float *nodes, int *flags, int *depthOut) {
	const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	if(i >= n - 1) return;
	const int2 r = range[i];
	const int size = r.y - r.x + 1;
	if(size <= maxLeaf) {
		if(i == 0) { // the whole scene is one leaf
			writeNode(nodes, 0, intBox[0], 0x80000000u | (unsigned)r.x, size); *depthOut = 0;
			if(!boxSane(intBox[0])) atomicAnd(flags, 0);
		}
		return;
	}
	// slot and depth of this node: walk up (inner ancestors only by construction)
	int depth = 0;
	for(int p = parentInt[i]; p >= 0; p = parentInt[p]) depth++;
	const int pi = parentInt[i];
	const int slot = i == 0 ? 0 : 1 + 2 * pi + (children[pi].y == i ? 1 : 0);
	const int2 c = children[i];
	const Box bl = c.x >= 0 ? intBox[c.x] : leafBox[~c.x], br = c.y >= 0 ? intBox[c.y] : leafBox[~c.y];
	// axis = largest separation of the children's centres; firstNode = which child comes first along +axis
	int axis = 0; float best = -1.0f, sep[3];
	for(int k = 0; k < 3; k++) {
		sep[k] = (br.mn[k] + br.mx[k]) - (bl.mn[k] + bl.mx[k]);
		if(fabsf(sep[k]) > best) { best = fabsf(sep[k]); axis = k; }
	}
	const int firstNode = sep[axis] >= 0.0f ? 0 : 1;
	const Box &bi = intBox[i];
	writeNode(nodes, slot, bi, (unsigned)(1 + 2 * i), axis | (firstNode << 16));
	bool ok = boxSane(bi);
	for(int side = 0; side < 2; side++) {
		const int ch = side ? c.y : c.x;
		const Box &cb = side ? br : bl;
		bool leaf = false; int first = 0, count = 0;
		if(ch < 0) { leaf = true; first = ~ch; count = 1; }
		else {
			const int2 cr = range[ch];
			if(cr.y - cr.x + 1 <= maxLeaf) { leaf = true; first = cr.x; count = cr.y - cr.x + 1; }
		}
		if(leaf) {
			writeNode(nodes, 1 + 2 * i + side, cb, 0x80000000u | (unsigned)first, count);
			ok = ok && boxSane(cb);
			atomicMax(depthOut, depth + 1);
		}
	}
	if(!ok) atomicAnd(flags, 0);
}

} // namespace lbvh
} // namespace dev

namespace {

struct Scratch {
	std::vector<void *> p;
	~Scratch() { for(void *q : p) if(q) (void)hipFree(q); }
	template <class T> int get(T **out, size_t count) {
		void *q = nullptr;
		if(hipMalloc(&q, (count ? count : 1) * sizeof(T)) != hipSuccess) return 1;
		p.push_back(q);
		*out = (T *)q;
		return 0;
	}
};

// builds nodes (2n-1 slots) and tris (n) into freshly allocated device arrays owned by the caller on success
int buildLbvhDevice(const float *hostVerts, int n, int maxLeaf, uint4 **outNodes, uint4 **outTris, int32_t *permHost, int *depth, int *fastOK,
					float *buildMs) {
	using namespace dev::lbvh;
	Scratch S;
	float *dVerts; unsigned *dBounds; u64 *dKeys, *dKeysSorted; int *dPerm, *dParentInt, *dParentLeaf, *dVisits, *dFlags;
	int2 *dChildren, *dRange; Box *dLeafBox, *dIntBox;
	const size_t nInt = (size_t)(n > 1 ? n - 1 : 1);
	if(S.get(&dVerts, (size_t)n * 9) || S.get(&dBounds, 6) || S.get(&dKeys, n) || S.get(&dKeysSorted, n) || S.get(&dPerm, n) || S.get(&dParentInt, nInt) ||
	   S.get(&dParentLeaf, n) || S.get(&dVisits, nInt) || S.get(&dFlags, 2) || S.get(&dChildren, nInt) || S.get(&dRange, nInt) || S.get(&dLeafBox, n) ||
	   S.get(&dIntBox, nInt)) {
		snail_set_error("snail_scene_create_lbvh: device allocation failed");
		return 2;
	}
	uint4 *dNodes = nullptr, *dTris = nullptr;
	const size_t nSlots = (size_t)2 * n - 1;
	if(hipMalloc((void **)&dNodes, nSlots * 32) != hipSuccess || hipMalloc((void **)&dTris, (size_t)n * 64) != hipSuccess) {
		if(dNodes) (void)hipFree(dNodes);
		snail_set_error("snail_scene_create_lbvh: device allocation failed");
		return 2;
	}
	auto fail = [&](int rc) { (void)hipFree(dNodes); (void)hipFree(dTris); return rc; };
#define LBVH_TRY(expr) do { hipError_t e_ = (expr); if(e_ != hipSuccess) { snail_set_error("%s failed: %s", #expr, hipGetErrorString(e_)); return fail(100 + (int)e_); } } while(0)
	LBVH_TRY(hipMemcpy(dVerts, hostVerts, (size_t)n * 36, hipMemcpyHostToDevice));
	hipEvent_t e0, e1;
	LBVH_TRY(hipEventCreate(&e0)); LBVH_TRY(hipEventCreate(&e1));
	const unsigned initBounds[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
	const int initFlags[2] = {1, 0};
	LBVH_TRY(hipMemcpy(dBounds, initBounds, sizeof(initBounds), hipMemcpyHostToDevice));
	LBVH_TRY(hipMemcpy(dFlags, initFlags, sizeof(initFlags), hipMemcpyHostToDevice));
	LBVH_TRY(hipMemset(dVisits, 0, nInt * sizeof(int)));
	hipLaunchKernelGGL(k_fill_empty, dim3((unsigned)((nSlots + 255) / 256)), dim3(256), 0, 0, (float *)dNodes, (int)nSlots);
	LBVH_TRY(hipEventRecord(e0, 0));
	const int T = 256, B = (n + T - 1) / T;
	hipLaunchKernelGGL(k_scene_bounds, dim3(B), dim3(T), 0, 0, dVerts, n, dBounds);
	hipLaunchKernelGGL(k_morton, dim3(B), dim3(T), 0, 0, dVerts, n, dBounds, dKeys);
	size_t tmpBytes = 0;
	LBVH_TRY(rocprim::radix_sort_keys(nullptr, tmpBytes, dKeys, dKeysSorted, (size_t)n, 0, 64, 0));
	char *dTmp;
	if(S.get(&dTmp, tmpBytes)) { snail_set_error("snail_scene_create_lbvh: device allocation failed"); return fail(2); }
	LBVH_TRY(rocprim::radix_sort_keys(dTmp, tmpBytes, dKeys, dKeysSorted, (size_t)n, 0, 64, 0));
	hipLaunchKernelGGL(k_records, dim3(B), dim3(T), 0, 0, dVerts, n, dKeysSorted, (float *)dTris, dPerm, dLeafBox, dFlags);
	bool rootOK = true;
	if(n == 1) { // a single leaf
		Box b;
		LBVH_TRY(hipMemcpy(&b, dLeafBox, sizeof(Box), hipMemcpyDeviceToHost));
		rootOK = boxSane(b);
		float node[8] = {b.mn[0], b.mn[1], b.mn[2], b.mx[0], b.mx[1], b.mx[2], 0.0f, 0.0f};
		const unsigned sub = 0x80000000u; const int aux = 1;
		memcpy(&node[6], &sub, 4); memcpy(&node[7], &aux, 4);
		LBVH_TRY(hipMemcpy(dNodes, node, 32, hipMemcpyHostToDevice));
	} else {
		const int Bi = (n - 1 + T - 1) / T;
		hipLaunchKernelGGL(k_topology, dim3(Bi), dim3(T), 0, 0, dKeysSorted, n, dChildren, dRange, dParentInt, dParentLeaf);
		hipLaunchKernelGGL(k_refit, dim3(B), dim3(T), 0, 0, n, dChildren, dParentInt, dParentLeaf, dLeafBox, dIntBox, dVisits);
		hipLaunchKernelGGL(k_emit, dim3(Bi), dim3(T), 0, 0, n, maxLeaf, dChildren, dRange, dParentInt, dLeafBox, dIntBox, (float *)dNodes, dFlags, dFlags + 1);
	}
	LBVH_TRY(hipEventRecord(e1, 0));
	LBVH_TRY(hipDeviceSynchronize());
	LBVH_TRY(hipGetLastError());
	float ms = 0.0f;
	(void)hipEventElapsedTime(&ms, e0, e1);
	(void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
	int flags[2];
	LBVH_TRY(hipMemcpy(flags, dFlags, sizeof(flags), hipMemcpyDeviceToHost));
	if(permHost) LBVH_TRY(hipMemcpy(permHost, dPerm, (size_t)n * 4, hipMemcpyDeviceToHost));
#undef LBVH_TRY
	*outNodes = dNodes; *outTris = dTris; *fastOK = flags[0] && rootOK; *depth = flags[1];
	if(buildMs) *buildMs = ms;
	return 0;
}

} // namespace
