// instances.inc -- device side of the two-level instanced scenes (DBVH, include/snail_instances.h).
// Included once per arithmetic right after snail_dev.inc, into the same namespace (dev / dev_sse).
//
// One wave per packet, as everywhere else.  The top-level walk is plain C++ (it is small: a few nodes per packet); its stack lives in
// VGPR lanes of its own (tStkNode / tStkFL), apart from the inner walk's.  At an instance leaf the active quads first..last are
// transformed in registers, moved down to lanes 0..count-1 (ds_bpermute) and handed to the generic walk (walk<...> of snail_dev.inc)
// as a packet of exactly count quads -- the RayGroup of ObjectInstance::CollidePrimary / CollideShadow (src/dbvh/tree.h:47-175) --
// then its distances, triIds and barycentrics are moved back.  The outer packet's own directions stay in registers for the next
// instance.  The inner walk runs in M_EXACT, the mode that restates the reference's operations for any input.
namespace SNAIL_DEV_NS {

struct InstBlas { const uint4 *nodes, *tris; };

struct InstArgs {
	const unsigned *hostTab; // FIRST: as PrimaryArgs::hostTab (dev_sse::hostTab() reads the kernel-argument segment's first 8 bytes)
	const uint4 *top;        // top-level node records (DBVH::Node)
	const uint4 *inst;       // per builder slot 4 x 16 B: {r0.xyz, BLAS index}, {r1.xyz, 0}, {r2.xyz, 0}, {t.xyz, 0}
	const InstBlas *blas;
	// primary frames (rect or packet list)
	GenConst g;
	int resx, resy, x0, y0, w, h, pw, nPackets;
	const int2 *packetXY;
	float *t, *u, *v;
	int *instOut, *triOut;
	// generic / shadow packets (Context / ShadowContext layouts of RaysArgs)
	int size;
	const float *origin, *dir, *idir;
	const unsigned char *mask;
	float *distance;
	int *object, *element;
	float *bary;
	u64 *stats;
	unsigned *pstats; // per-packet TreeStats [nPackets][4] (bookPacket: k_inst_frame, k_inst_trace<.., PSTATS>; the heat-map launches) or null
};

__device__ __forceinline__ float instShfl(float x, int src) { return __int_as_float(__builtin_amdgcn_ds_bpermute(src << 2, __float_as_int(x))); }
__device__ __forceinline__ int instShfl(int x, int src) { return __builtin_amdgcn_ds_bpermute(src << 2, x); }

// BBox::TestInterval + BBox::Test (src/bounding_box.cpp:208-236, :61-200) of a top-level node: the M_EXACT test of walk<> on the same
// 32-byte record, the quads with a passing lane (before clipping to [first,last])
template <bool SHARED, bool SHADOW>
__device__ __forceinline__ u64 instBoxPass(const Node &n, const Interval &iv, const float (&org)[3][4], const float (&id)[3][4], const float (&dist)[4]) {
	bool anyPass = false;
	if(boxTestInterval(n, iv)) {
		float tmn[3], tmx[3];
		if(SHARED) {
#pragma unroll
			for(int k = 0; k < 3; k++) { tmn[k] = n.bmin[k] - org[k][0]; tmx[k] = n.bmax[k] - org[k][0]; }
		}
#pragma unroll
		for(int l = 0; l < 4; l++) {
			float lmin = 0.0f, lmax = 0.0f;
#pragma unroll
			for(int k = 0; k < 3; k++) {
				float l1 = id[k][l] * (SHARED ? tmn[k] : n.bmin[k] - org[k][l]);
				float l2 = id[k][l] * (SHARED ? tmx[k] : n.bmax[k] - org[k][l]);
				float lo = Min<M_EXACT>(l1, l2), hi = Max<M_EXACT>(l1, l2);
				if(k == 0) { lmin = lo; lmax = hi; }
				else if(SHADOW) { lmin = Max<M_EXACT>(lo, lmin); lmax = Min<M_EXACT>(hi, lmax); }
				else { lmin = Max<M_EXACT>(lmin, lo); lmax = Min<M_EXACT>(lmax, hi); }
			}
			bool pass = SHADOW ? (lmax >= 0.0f && lmin <= Min<M_EXACT>(lmax, dist[l])) : !(lmax < 0.0f || lmin > Min<M_EXACT>(lmax, dist[l]));
			anyPass |= pass;
		}
	}
	return __builtin_amdgcn_ballot_w64(anyPass);
}

// ObjectInstance::CollidePrimary / CollideShadow (src/dbvh/tree.h:47-175) of builder slot `slot` on the outer quads [first,last]
template <bool SHARED, bool MASK, bool SHADOW, bool BARY, bool DEEP>
__device__ __forceinline__ void instCollide(const InstArgs &A, int slot, int first, int last, int lane, const float (&org)[3][4], const float (&d)[3][4],
											unsigned mask4, float (&dist)[4], int (&obj)[4], int (&elem)[4], float (&bu)[4], float (&bv)[4], float *lds,
											Counters &st) {
	float R[3][3], T[3];
	int b;
	{
		scalar_ptr p = (scalar_ptr)(unsigned long long)(A.inst + (size_t)slot * 4);
		const u32x4 q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3];
		R[0][0] = asf(q0.x); R[0][1] = asf(q0.y); R[0][2] = asf(q0.z); b = (int)q0.w;
		R[1][0] = asf(q1.x); R[1][1] = asf(q1.y); R[1][2] = asf(q1.z);
		R[2][0] = asf(q2.x); R[2][1] = asf(q2.y); R[2][2] = asf(q2.z);
		T[0] = asf(q3.x); T[1] = asf(q3.y); T[2] = asf(q3.z);
	}
	const uint4 *bn, *bt;
	{
		scalar_ptr p = (scalar_ptr)(unsigned long long)(A.blas + b);
		const u32x4 q = p[0];
		bn = (const uint4 *)(((unsigned long long)q.y << 32) | q.x);
		bt = (const uint4 *)(((unsigned long long)q.w << 32) | q.z);
	}
	const int count = last - first + 1;
	const int src = first + (lane < count ? lane : 0);

	// inner RayGroup of `count` quads: lane i <- outer quad first + i; ITransformVec, SafeInv, ITransformPoint (src/dbvh/tree.h:34-45,:52-58)
	Quad IQ;
	float iorg[3][4];
	float sd[3][4];
#pragma unroll
	for(int c = 0; c < 3; c++)
#pragma unroll
		for(int l = 0; l < 4; l++) sd[c][l] = instShfl(d[c][l], src);
#pragma unroll
	for(int l = 0; l < 4; l++) {
#pragma unroll
		for(int c = 0; c < 3; c++) IQ.d[c][l] = sd[0][l] * R[0][c] + sd[1][l] * R[1][c] + sd[2][l] * R[2][c];
#pragma unroll
		for(int c = 0; c < 3; c++) IQ.id[c][l] = Inv(IQ.d[c][l] + 0.00000001f); // SafeInv (src/rtbase.h:117-120)
		IQ.dist[l] = instShfl(dist[l], src);
	}
	if(SHARED) {
		const float p0 = org[0][0] - T[0], p1 = org[1][0] - T[1], p2 = org[2][0] - T[2];
#pragma unroll
		for(int c = 0; c < 3; c++) {
			const float o = p0 * R[0][c] + p1 * R[1][c] + p2 * R[2][c];
#pragma unroll
			for(int l = 0; l < 4; l++) iorg[c][l] = o;
		}
	} else {
#pragma unroll
		for(int l = 0; l < 4; l++) {
			const float p0 = instShfl(org[0][l], src) - T[0], p1 = instShfl(org[1][l], src) - T[1], p2 = instShfl(org[2][l], src) - T[2];
#pragma unroll
			for(int c = 0; c < 3; c++) iorg[c][l] = p0 * R[0][c] + p1 * R[1][c] + p2 * R[2][c];
		}
	}
	const unsigned imask = MASK ? (unsigned)instShfl((int)mask4, src) : 15u;
	int itid[4] = {-1, -1, -1, -1}; // objects[n] = i32x4(~0)
	float ibu[4] = {0, 0, 0, 0}, ibv[4] = {0, 0, 0, 0};
	walk<SHARED, MASK, SHADOW, M_EXACT, BARY, DEEP, false>(bn, bt, count, lane, iorg, IQ, imask, itid, ibu, ibv, lds, st);

	// back to the outer quads: lane first + i <- lane i
	const bool mine = lane >= first && lane <= last;
	const int back = mine ? lane - first : 0;
#pragma unroll
	for(int l = 0; l < 4; l++) {
		const float nd = instShfl(IQ.dist[l], back);
		if(mine) dist[l] = nd;
		if(!SHADOW) {
			const int tid = instShfl(itid[l], back);
			float nu = 0.0f, nv = 0.0f;
			if(BARY) { nu = instShfl(ibu[l], back); nv = instShfl(ibv[l], back); }
			if(mine && tid != -1) { // (objects[n] != ~0: a hit inside this instance)
				obj[l] = slot; elem[l] = tid;
				if(BARY) { bu[l] = nu; bv[l] = nv; } // (deviation: at the hit's own quad, see include/snail_instances.h)
			}
		}
	}
}

// DBVH::TraversePrimary0 / TraverseShadow0 (src/dbvh/traverse.cpp:14-134) of one packet of `size` quads
template <bool SHARED, bool MASK, bool SHADOW, bool BARY, bool DEEP>
__device__ __forceinline__ void instWalk(const InstArgs &A, int size, int lane, const float (&org)[3][4], const float (&d)[3][4], const float (&id)[3][4],
										 unsigned mask4, float (&dist)[4], int (&obj)[4], int (&elem)[4], float (&bu)[4], float (&bv)[4], float *lds,
										 Counters &st) {
	Interval iv;
	{ // RayInterval(c.rays) (src/ray_group.h:296-333): no distances, also for shadow packets (traverse.cpp:93)
		const unsigned act4 = lane < size ? (MASK ? (mask4 & 15u) : 15u) : 0u;
		computeMinMax<true, MASK>(d, act4, size, lane, lds, iv.minDir, iv.maxDir);
		computeMinMax<true, MASK>(id, act4, size, lane, lds, iv.minIDir, iv.maxIDir);
		if(SHARED) {
#pragma unroll
			for(int k = 0; k < 3; k++) iv.minOrg[k] = iv.maxOrg[k] = org[k][0];
		} else computeMinMax<true, MASK>(org, act4, size, lane, lds, iv.minOrg, iv.maxOrg);
	}
	const int signBits = __builtin_amdgcn_readfirstlane((d[0][0] < 0.0f ? 1 : 0) | (d[1][0] < 0.0f ? 2 : 0) | (d[2][0] < 0.0f ? 4 : 0));
	int tStkNode = 0, tStkFL = 0, tStkNode2 = 0, tStkFL2 = 0; // slot i = lane i (slots 64.. in the second pair)
	int sp = 0;
	int first = 0, last = size - 1;
	Node n = loadNode(A.top, 0);
	for(;;) {
		st.iters++; // LoopIteration
		const bool isLeaf = (n.sub & 0x80000000u) != 0;
		const u64 alive = instBoxPass<SHARED, SHADOW>(n, iv, org, id, dist) & __builtin_amdgcn_ballot_w64((unsigned)(lane - first) <= (unsigned)(last - first));
		if(alive != 0) {
			first = __builtin_ctzll(alive);
			last = 63 - __builtin_clzll(alive);
			if(!isLeaf) {
				const int axis = n.aux & 0xffff;
				const int firstNode = ((n.aux >> 16) ^ (signBits >> axis)) & 1;
				const int fl = first | (last << 8);
				const int farIdx = (int)n.sub + (firstNode ^ 1);
				if(sp < 64) writeLane2(tStkNode, farIdx, tStkFL, fl, sp);
				else writeLane2(tStkNode2, farIdx, tStkFL2, fl, sp - 64);
				sp++;
				n = loadNode(A.top, (int)n.sub + firstNode);
				continue;
			}
			const int count = n.aux, firstInst = (int)(n.sub & 0x7fffffffu);
			for(int k = 0; k < count; k++) {
				instCollide<SHARED, MASK, SHADOW, BARY, DEEP>(A, firstInst + k, first, last, lane, org, d, mask4, dist, obj, elem, bu, bv, lds, st);
				st.intersects += (unsigned)(last - first + 1);
			}
		}
		if(sp == 0) break;
		sp--;
		int cur, fl;
		if(sp < 64) { cur = __builtin_amdgcn_readlane(tStkNode, sp); fl = __builtin_amdgcn_readlane(tStkFL, sp); }
		else { cur = __builtin_amdgcn_readlane(tStkNode2, sp - 64); fl = __builtin_amdgcn_readlane(tStkFL2, sp - 64); }
		first = fl & 0xff; last = fl >> 8;
		n = loadNode(A.top, cur);
	}
}

// ---- primary frames: RayGenerator::Generate + SafeInv + DBVH::TraversePrimary<1,0> (same packets and layouts as k_primary) ----
template <bool DEEP>
__global__ __launch_bounds__(64) void k_inst_frame(InstArgs A) {
	__shared__ float lds[LDS_FLOATS_PER_WAVE];
	const int lane = threadIdx.x & 63;
	const int p = (int)blockIdx.x;
	if(p >= A.nPackets) return;
	int px, py;
	if(A.packetXY) {
		const int2 xy = A.packetXY[p];
		px = __builtin_amdgcn_readfirstlane(xy.x);
		py = __builtin_amdgcn_readfirstlane(xy.y);
	} else {
		px = A.x0 + (p % A.pw) * 16;
		py = A.y0 + (p / A.pw) * 16;
	}
	const GenConst &G = A.g;
	float d[3][4], id[3][4], dist[4];
	const int ty = lane >> 2, k4 = lane & 3;
	// RayGenerator::Generate, level 3 (src/ray_generator.cpp:23-47): quad ty*4+k, lane j -> pixel (x+4k+j, y+ty) -- the operations of primaryPacket
#if SNAIL_ARITH_SSE
	{
		float pt[3][4], pp[4], rs[4], dn[12], idn[12];
#pragma unroll
		for(int l = 0; l < 4; l++) {
			const float xoff = (float)(px + (l >= 2 ? 2 : 0));
			const float yoff = (float)(py - (l >= 2 ? 1 : 0));
			const float tposx = (float)(4 * k4) + xoff;
			const float tposy = (float)ty + yoff;
#pragma unroll
			for(int c = 0; c < 3; c++) pt[c][l] = G.tright[c] * tposx + (G.tup[c] * tposy + G.txyz[c][l]);
			pp[l] = pt[0][l] * pt[0][l] + pt[1][l] * pt[1][l] + pt[2][l] * pt[2][l];
		}
		RSqrtN<4>(pp, rs);
#pragma unroll
		for(int l = 0; l < 4; l++)
#pragma unroll
			for(int c = 0; c < 3; c++) { d[c][l] = pt[c][l] * rs[l]; dn[c * 4 + l] = d[c][l] + 0.00000001f; }
		InvN<12>(dn, idn);
#pragma unroll
		for(int l = 0; l < 4; l++) {
#pragma unroll
			for(int c = 0; c < 3; c++) id[c][l] = idn[c * 4 + l];
			dist[l] = __builtin_inff();
		}
	}
#else
#pragma unroll
	for(int l = 0; l < 4; l++) {
		const float xoff = (float)(px + (l >= 2 ? 2 : 0));
		const float yoff = (float)(py - (l >= 2 ? 1 : 0));
		const float tposx = (float)(4 * k4) + xoff;
		const float tposy = (float)ty + yoff;
		const float p0 = G.tright[0] * tposx + (G.tup[0] * tposy + G.txyz[0][l]);
		const float p1 = G.tright[1] * tposx + (G.tup[1] * tposy + G.txyz[1][l]);
		const float p2 = G.tright[2] * tposx + (G.tup[2] * tposy + G.txyz[2][l]);
		const float rs = RSqrt(p0 * p0 + p1 * p1 + p2 * p2);
		d[0][l] = p0 * rs; d[1][l] = p1 * rs; d[2][l] = p2 * rs;
#pragma unroll
		for(int c = 0; c < 3; c++) id[c][l] = Inv(d[c][l] + 0.00000001f);
		dist[l] = __builtin_inff();
	}
#endif
	float org[3][4];
#pragma unroll
	for(int c = 0; c < 3; c++)
#pragma unroll
		for(int l = 0; l < 4; l++) org[c][l] = G.org[c];
	int obj[4] = {0, 0, 0, 0}, elem[4] = {0, 0, 0, 0};
	float bu[4] = {0, 0, 0, 0}, bv[4] = {0, 0, 0, 0};
	Counters st = {0, 0, 0, 0, 0};
	instWalk<true, false, false, true, DEEP>(A, 64, lane, org, d, id, 15u, dist, obj, elem, bu, bv, lds, st);
	flushStats(A.stats, st, 256u, lane);
	bookPacket(A.pstats, (size_t)p, st, 256u, lane);

	if(A.packetXY) { // packet-major (Context layout)
		const size_t o = (size_t)p * 256 + (size_t)lane * 4;
		if(A.t) *(float4 *)(A.t + o) = make_float4(dist[0], dist[1], dist[2], dist[3]);
		if(A.u) *(float4 *)(A.u + o) = make_float4(bu[0], bu[1], bu[2], bu[3]);
		if(A.v) *(float4 *)(A.v + o) = make_float4(bv[0], bv[1], bv[2], bv[3]);
		if(A.instOut) *(int4 *)(A.instOut + o) = make_int4(obj[0], obj[1], obj[2], obj[3]);
		if(A.triOut) *(int4 *)(A.triOut + o) = make_int4(elem[0], elem[1], elem[2], elem[3]);
	} else {
		const int yy = py + ty, xx = px + k4 * 4;
		const int xlim = min(A.resx, A.x0 + A.w), ylim = min(A.resy, A.y0 + A.h);
		if(yy < ylim) {
			const size_t o = (size_t)yy * A.resx + xx;
#pragma unroll
			for(int l = 0; l < 4; l++)
				if(xx + l < xlim) {
					if(A.t) A.t[o + l] = dist[l];
					if(A.u) A.u[o + l] = bu[l];
					if(A.v) A.v[o + l] = bv[l];
					if(A.instOut) A.instOut[o + l] = obj[l];
					if(A.triOut) A.triOut[o + l] = elem[l];
				}
		}
	}
}

// ---- generic packets: DBVH::TraversePrimary<SHARED,MASK>(Context&) ----
// PSTATS: the heat-map launches' instantiation, which also books per packet (a template argument as in snail_dev.inc: a pointer test here cost the
// other launches' kernel scalar spills and, in one instantiation, a wave; for the same reason the walk under an order list is a kernel of its
// own, k_imat_trace_level in instances_materials_transparency.inc, which repeats the <false, true, DEEP, true> body: a change here belongs there too)
template <bool SHARED, bool MASK, bool DEEP, bool BARY, bool PSTATS = false>
__global__ __launch_bounds__(64) void k_inst_trace(InstArgs A) {
	__shared__ float lds[LDS_FLOATS_PER_WAVE];
	const int lane = threadIdx.x & 63;
	const int p = (int)blockIdx.x;
	if(p >= A.nPackets) return;
	const int size = A.size;
	const bool live = lane < size;
	const size_t q = (size_t)p * size + (live ? lane : 0);
	float d[3][4], id[3][4], org[3][4];
	loadQuad3(A.dir, q, d);
	loadQuad3(A.idir, q, id);
	if(SHARED) {
		scalar_ptr op = (scalar_ptr)(unsigned long long)(A.origin + (size_t)p * 12);
		const u32x4 ox = op[0], oy = op[1], oz = op[2];
#pragma unroll
		for(int l = 0; l < 4; l++) { org[0][l] = asf(ox.x); org[1][l] = asf(oy.x); org[2][l] = asf(oz.x); } // ExtractN(Origin(0), 0)
	} else loadQuad3(A.origin, q, org);
	const unsigned mask4 = MASK ? (A.mask[q] & 15u) : 15u;
	const float4 dv = *(const float4 *)(A.distance + q * 4);
	const int4 ov = *(const int4 *)(A.object + q * 4), ev = *(const int4 *)(A.element + q * 4);
	float dist[4] = {dv.x, dv.y, dv.z, dv.w};
	int obj[4] = {ov.x, ov.y, ov.z, ov.w}, elem[4] = {ev.x, ev.y, ev.z, ev.w};
	float bu[4] = {0, 0, 0, 0}, bv[4] = {0, 0, 0, 0};
	if(BARY) {
		const float4 b0 = *(const float4 *)(A.bary + q * 8), b1 = *(const float4 *)(A.bary + q * 8 + 4);
		bu[0] = b0.x; bu[1] = b0.y; bu[2] = b0.z; bu[3] = b0.w;
		bv[0] = b1.x; bv[1] = b1.y; bv[2] = b1.z; bv[3] = b1.w;
	}
	Counters st = {0, 0, 0, 0, 0};
	instWalk<SHARED, MASK, false, BARY, DEEP>(A, size, lane, org, d, id, mask4, dist, obj, elem, bu, bv, lds, st);
	flushStats(A.stats, st, 0u, lane);
	if(PSTATS) bookPacket(A.pstats, (size_t)p, st, 0u, lane);
	if(live) {
		*(float4 *)(A.distance + q * 4) = make_float4(dist[0], dist[1], dist[2], dist[3]);
		*(int4 *)(A.object + q * 4) = make_int4(obj[0], obj[1], obj[2], obj[3]);
		*(int4 *)(A.element + q * 4) = make_int4(elem[0], elem[1], elem[2], elem[3]);
		if(BARY) {
			*(float4 *)(A.bary + q * 8) = make_float4(bu[0], bu[1], bu[2], bu[3]);
			*(float4 *)(A.bary + q * 8 + 4) = make_float4(bv[0], bv[1], bv[2], bv[3]);
		}
	}
}

// ---- shadow packets: DBVH::TraverseShadow(ShadowContext&) ----
template <bool DEEP>
__global__ __launch_bounds__(64) void k_inst_occl(InstArgs A) {
	__shared__ float lds[LDS_FLOATS_PER_WAVE];
	const int lane = threadIdx.x & 63;
	const int p = (int)blockIdx.x;
	if(p >= A.nPackets) return;
	const int size = A.size;
	const bool live = lane < size;
	const size_t q = (size_t)p * size + (live ? lane : 0);
	float d[3][4], id[3][4], org[3][4];
	loadQuad3(A.dir, q, d);
	loadQuad3(A.idir, q, id);
	{
		const float *op = A.origin + (size_t)p * 3;
		const float o0 = firstlanef(op[0]), o1 = firstlanef(op[1]), o2 = firstlanef(op[2]);
#pragma unroll
		for(int l = 0; l < 4; l++) { org[0][l] = o0; org[1][l] = o1; org[2][l] = o2; }
	}
	const float4 dv = *(const float4 *)(A.distance + q * 4);
	float dist[4] = {dv.x, dv.y, dv.z, dv.w};
	int obj[4] = {0, 0, 0, 0}, elem[4] = {0, 0, 0, 0};
	float bu[4] = {0, 0, 0, 0}, bv[4] = {0, 0, 0, 0};
	Counters st = {0, 0, 0, 0, 0};
	instWalk<true, false, true, false, DEEP>(A, size, lane, org, d, id, 15u, dist, obj, elem, bu, bv, lds, st);
	flushStats(A.stats, st, 0u, lane);
	if(live) *(float4 *)(A.distance + q * 4) = make_float4(dist[0], dist[1], dist[2], dist[3]);
}

} // namespace SNAIL_DEV_NS
