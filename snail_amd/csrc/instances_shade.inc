// instances_shade.inc -- Scene<DBVH>::RayTrace, simple-shading configuration, for the two-level instanced scenes (include/snail_instances.h):
// lights, shadow packets and the gVals[7] mirrored bounce around the walks of instances.inc.  Included once per arithmetic right after
// instances.inc, into the same namespace (dev / dev_sse).
//
// The staging is that of the plain scenes' pipeline (snail_dev.inc, "Scene::RayTrace after the traversal"): packet-major intermediates in
// HBM, one wave per packet or per (packet, light), nothing but the shadow packet live across a walk, samples derived again in the final
// pass.  Always over an explicit packet list (packet li = packetXY[li]; intermediates and packet-major output indexed by li):
//   k_inst_frame                               primary hits (t, instance slot, triId)
//   k_inst_light<DEEP, SRC_PRIMARY>            one wave per (packet, light): samples -> light cull -> shadow packet -> DBVH::TraverseShadow
//                                              -> the surviving distances [light][packet][256]        Scene::TraceLight, scene_trace.cpp:523-566
//   k_inst_final<SRC_PRIMARY, DST_FRAME>       samples, the tail of TraceLight per light, colour, ConvColor, B,G,R store   :567-601, :484-512
// and with reflections, between the first two:
//   k_inst_final<SRC_PRIMARY, DST_MIRROR>      samples -> mirrored packets + lane masks                Scene::TraceReflection, :603-618
//   k_inst_trace<false, true, DEEP, false>     DBVH::TraversePrimary<0,1> of the mirrored packets
//   k_inst_light<DEEP, SRC_MIRROR>, k_inst_final<SRC_MIRROR, DST_COLOR>   the nested RayTrace -> a float colour per mirrored ray
// The one difference to a plain scene's sample is the normal: ObjectInstance::GetNormal = TransformVec(blas.GetNormal(elem))
// (src/dbvh/tree.h:21-26,178-181,216-218).  hitBounds / lightCulled / shadowLane / shadeAndStore are the plain pipeline's, on these samples.
// Table arithmetic: every look-up in its fully checked form.
namespace SNAIL_DEV_NS {

struct InstShadeArgs {
	ShadeArgs s;          // FIRST: its hostTab opens the kernel-argument segment.  hitId / rObj hold the triIds; nodes / tris / pf are unused
	InstArgs i;           // top, inst, blas: the tree the walks and the normals read
	const int *hitInst;   // instance slot of the primary hits, packet-major
	int *rInst;           // instance slot of the mirrored hits (zeroed with the mirrored packets, written by k_inst_trace)
};

// the packet's rays and hits, then its samples (loadSamples of snail_dev.inc with the instance's normal)
template <int SRC>
__device__ __forceinline__ void instLoadSamples(const InstShadeArgs &A, const PacketPos &P, int lane, float (&d)[3][4], Samples &S) {
	const size_t quad = P.pidx * 64 + lane;
	const float inf = __builtin_inff();
	float org[3][4], dist[4];
	int tid[4], slot[4];
	unsigned mask4 = 15u;
	if(SRC == SRC_MIRROR) {
		loadQuad3(A.s.rDir, quad, d);
		loadQuad3(A.s.rOrg, quad, org);
		mask4 = A.s.rMask[quad] & 15u;
		const float4 dv = *(const float4 *)(A.s.rDist + quad * 4);
		const int4 ev = *(const int4 *)(A.s.rObj + quad * 4), iv = *(const int4 *)(A.rInst + quad * 4);
		dist[0] = dv.x; dist[1] = dv.y; dist[2] = dv.z; dist[3] = dv.w;
		tid[0] = ev.x; tid[1] = ev.y; tid[2] = ev.z; tid[3] = ev.w;
		slot[0] = iv.x; slot[1] = iv.y; slot[2] = iv.z; slot[3] = iv.w;
	} else {
		const int ty = lane >> 2, k4 = lane & 3;
#pragma unroll
		for(int l = 0; l < 4; l++) { // RayGenerator::Generate, exactly as in k_inst_frame
			const float xoff = (float)(P.px + (l >= 2 ? 2 : 0)), yoff = (float)(P.py - (l >= 2 ? 1 : 0));
			const float tposx = (float)(4 * k4) + xoff, tposy = (float)ty + yoff;
			const float p0 = A.s.g.tright[0] * tposx + (A.s.g.tup[0] * tposy + A.s.g.txyz[0][l]);
			const float p1 = A.s.g.tright[1] * tposx + (A.s.g.tup[1] * tposy + A.s.g.txyz[1][l]);
			const float p2 = A.s.g.tright[2] * tposx + (A.s.g.tup[2] * tposy + A.s.g.txyz[2][l]);
			const float rs = RSqrt(p0 * p0 + p1 * p1 + p2 * p2);
			d[0][l] = p0 * rs; d[1][l] = p1 * rs; d[2][l] = p2 * rs;
#pragma unroll
			for(int c = 0; c < 3; c++) org[c][l] = A.s.g.org[c];
		}
		const float4 dv = *(const float4 *)(A.s.hitT + quad * 4);
		const int4 ev = *(const int4 *)(A.s.hitId + quad * 4), iv = *(const int4 *)(A.hitInst + quad * 4);
		dist[0] = dv.x; dist[1] = dv.y; dist[2] = dv.z; dist[3] = dv.w;
		tid[0] = ev.x; tid[1] = ev.y; tid[2] = ev.z; tid[3] = ev.w;
		slot[0] = iv.x; slot[1] = iv.y; slot[2] = iv.z; slot[3] = iv.w;
	}
#pragma unroll
	for(int l = 0; l < 4; l++) {
		S.hit[l] = dist[l] < inf && ((mask4 >> l) & 1u) != 0;
#pragma unroll
		for(int c = 0; c < 3; c++) S.pos[c][l] = d[c][l] * dist[l] + org[c][l];
		// ObjectInstance::GetNormal (src/dbvh/tree.h:178-181): the instance record and its BLAS as instCollide reads them (per lane here),
		// plane.xyz of the triangle, TransformVec (:21-26: three products added left to right)
		const uint4 *rec = A.i.inst + (size_t)(S.hit[l] ? slot[l] : 0) * 4;
		const uint4 q0 = rec[0], q1 = rec[1], q2 = rec[2];
		const uint4 *bt = A.i.blas[(int)q0.w].tris;
		const float4 pl = *(const float4 *)((const float *)(bt + (size_t)(S.hit[l] ? tid[l] : 0) * 4) + 12);
		const float n0 = pl.x * asf(q0.x) + pl.y * asf(q0.y) + pl.z * asf(q0.z);
		const float n1 = pl.x * asf(q1.x) + pl.y * asf(q1.y) + pl.z * asf(q1.z);
		const float n2 = pl.x * asf(q2.x) + pl.y * asf(q2.y) + pl.z * asf(q2.z);
		S.nrm[0][l] = S.hit[l] ? n0 : 0.0f; S.nrm[1][l] = S.hit[l] ? n1 : 0.0f; S.nrm[2][l] = S.hit[l] ? n2 : 0.0f;
		const float dn = d[0][l] * S.nrm[0][l] + d[1][l] * S.nrm[1][l] + d[2][l] * S.nrm[2][l];
		S.sdn[l] = S.hit[l] ? __builtin_fabsf(dn) : 0.0f;
	}
}

// ---- one (packet, light): the shadow packet (src/scene_trace.cpp:538-558) and DBVH::TraverseShadow ----
template <bool DEEP, int SRC>
__global__ __launch_bounds__(64) void k_inst_light(InstShadeArgs A) {
	__shared__ float lds[LDS_FLOATS_PER_WAVE];
	const int lane = threadIdx.x & 63;
	const int li = (int)blockIdx.x, n = (int)blockIdx.y;
	if(li >= A.s.nPackets || n >= A.s.nLights) return;
	const PacketPos P = packetOf(A.s, li);
	const float lp[3] = {A.s.lights[n][0], A.s.lights[n][1], A.s.lights[n][2]};
	const float radius = A.s.lights[n][6], radSq = radius * radius;
	Quad Q;
	{
		float d[3][4];
		Samples S;
		instLoadSamples<SRC>(A, P, lane, d, S);
		float tMin[3], tMax[3];
		hitBounds(S, tMin, tMax);
		if(lightCulled(tMin, tMax, lp, radSq)) return;   // (wave-uniform; k_inst_final skips the light by the same test)
#pragma unroll
		for(int l = 0; l < 4; l++) {
			float sd[3], distance, dotv;
			shadowLane(S, l, lp, sd, distance, dotv, Q.dist[l]);
#pragma unroll
			for(int c = 0; c < 3; c++) { Q.d[c][l] = sd[c]; Q.id[c][l] = S.hit[l] ? InvDiv(sd[c] + 0.00000001f) : 0.0f; }
		}
	}
	unsigned rays = 0;   // stats.TracingRays(CountMaskBits(ForWhich(mask))), :557
#pragma unroll
	for(int l = 0; l < 4; l++) rays += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(Q.dist[l] > 0.0f));
	float lorg[3][4];
#pragma unroll
	for(int c = 0; c < 3; c++)
#pragma unroll
		for(int l = 0; l < 4; l++) lorg[c][l] = lp[c];
	int obj[4] = {0, 0, 0, 0}, elem[4] = {0, 0, 0, 0};
	float bu[4] = {0, 0, 0, 0}, bv[4] = {0, 0, 0, 0};
	Counters st = {0, 0, 0, 0, 0};
	instWalk<true, false, true, false, DEEP>(A.i, 64, lane, lorg, Q.d, Q.id, 15u, Q.dist, obj, elem, bu, bv, lds, st);
	flushStats(A.s.stats, st, rays, lane);
	*(float4 *)(A.s.sDist + ((size_t)n * (size_t)A.s.nPackets + P.pidx) * 256 + (size_t)lane * 4) = make_float4(Q.dist[0], Q.dist[1], Q.dist[2], Q.dist[3]);
}

// ---- one packet: samples -> mirrored packets (DST_MIRROR), or samples + the lights' surviving distances -> colour (DST_FRAME / DST_COLOR) ----
template <int SRC, int DST>
__global__ __launch_bounds__(64) void k_inst_final(InstShadeArgs A) {
	const int lane = threadIdx.x & 63;
	const int li = (int)blockIdx.x;
	if(li >= A.s.nPackets) return;
	const PacketPos P = packetOf(A.s, li);
	const size_t quad = P.pidx * 64 + lane;
	float d[3][4];
	Samples S;
	instLoadSamples<SRC>(A, P, lane, d, S);
	if(DST == DST_MIRROR) {
		// Scene::TraceReflection (src/scene_trace.cpp:603-618): Reflect (src/rtbase_math.h:54-58) about the world-space normal, origin = position
		// + 0.001 dir, SafeInv; selector = hit lanes.  Masked lanes: zeros, distance -inf (as the plain scenes' mirrored packets).
		const float inf = __builtin_inff();
		float rd[3][4], ro[3][4], ri[3][4], rdist[4];
		unsigned sel = 0;
#pragma unroll
		for(int l = 0; l < 4; l++) {
			const float dt = S.nrm[0][l] * d[0][l] + S.nrm[1][l] * d[1][l] + S.nrm[2][l] * d[2][l];
			const float dt2 = dt + dt;
#pragma unroll
			for(int c = 0; c < 3; c++) {
				const float r = d[c][l] - S.nrm[c][l] * dt2;
				rd[c][l] = S.hit[l] ? r : 0.0f;
				ro[c][l] = S.hit[l] ? S.pos[c][l] + r * 0.001f : 0.0f;
				ri[c][l] = Inv(rd[c][l] + 0.00000001f);
			}
			rdist[l] = S.hit[l] ? inf : -inf; // src/scene_trace.cpp:112-115
			sel |= S.hit[l] ? (1u << l) : 0u;
		}
		float4 *po = (float4 *)(A.s.rOrg + quad * 12), *pd = (float4 *)(A.s.rDir + quad * 12), *pi = (float4 *)(A.s.rIDir + quad * 12);
#pragma unroll
		for(int c = 0; c < 3; c++) {
			po[c] = make_float4(ro[c][0], ro[c][1], ro[c][2], ro[c][3]);
			pd[c] = make_float4(rd[c][0], rd[c][1], rd[c][2], rd[c][3]);
			pi[c] = make_float4(ri[c][0], ri[c][1], ri[c][2], ri[c][3]);
		}
		A.s.rMask[quad] = (unsigned char)sel;
		*(float4 *)(A.s.rDist + quad * 4) = make_float4(rdist[0], rdist[1], rdist[2], rdist[3]);
		*(int4 *)(A.s.rObj + quad * 4) = make_int4(0, 0, 0, 0);
		*(int4 *)(A.rInst + quad * 4) = make_int4(0, 0, 0, 0);
		unsigned cnt = 0;     // stats.TracingRays(CountMaskBits(mask)) of the nested RayTrace (src/scene_trace.cpp:116-117)
#pragma unroll
		for(int l = 0; l < 4; l++) cnt += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(S.hit[l]));
		const Counters none = {0, 0, 0, 0, 0};
		flushStats(A.s.stats, none, cnt, lane);
		return;
	}
	if(DST == DST_FRAME || DST == DST_COLOR) {
		const float none[4] = {0.0f, 0.0f, 0.0f, 0.0f};
		shadeAndStore<SRC, DST, false>(A.s, P, lane, d, S, none);
	}
}

} // namespace SNAIL_DEV_NS
