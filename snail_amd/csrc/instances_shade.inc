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
//
// The tile renderer's switches (include/snail_instances_tiles.h; RenderTask::Work, src/render.cpp:71-190) end in one more pass:
//   k_inst_store<DEPTH, AA, PLANAR>            float colours of k_inst_final (ShadeArgs::colPackets) or the hit distances of k_inst_frame
//                                              -> [2x2 reduction of gVals[9]] -> [rank tint of gVals[8]] -> ConvColor -> packet-major B,G,R
//                                              bytes, or the tile's planes R, G-R, B-R
// and, for the antialiased frames, k_inst_aa_packets lists the four double-resolution packets of every packet of the call.
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
// TWINS: k_imat_light (instances_materials.inc) is this kernel with the samples of full shading (matLoadSamples) in place of instLoadSamples; a
// change to the shadow packet, the walk or the stats flush belongs there too.
template <bool DEEP, int SRC, bool PSTATS = false>
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
	if(PSTATS) bookPacket(A.s.pstats, P.pidx, st, rays, lane);   // (a culled light has returned above: it books nothing)
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
		bookPacket(A.s.pstats, P.pidx, none, cnt, lane);
		return;
	}
	if(DST == DST_FRAME || DST == DST_COLOR) {
		const float none[4] = {0.0f, 0.0f, 0.0f, 0.0f};
		shadeAndStore<SRC, DST, false>(A.s, P, lane, d, S, none);
	}
}

// ---- the tail of RenderTask::Work (src/render.cpp:71-163) for the packets of an instanced scene ----
struct InstStoreArgs {
	const unsigned *hostTab;     // FIRST: as PrimaryArgs::hostTab (DEPTH: Inv of the handle's arithmetic)
	const float *in;             // colours [n][256][3] (r, g, b), DEPTH: hit distances [n][256]; AA: n = 4 nPackets, sub-packet k of packet p at 4 p + k
	int nPackets;                // OUTPUT packets
	int tinted;                  // gVals[8]: c = (c + 0.1) * tint, after the reduction, before ConvColor (src/render.cpp:118-132)
	float tint[3];
	unsigned char *bgrPackets;   // !PLANAR: packet-major B,G,R [nPackets][256][3], 4-byte aligned
	// PLANAR: packet p belongs to tile packetTile[p], whose packets firstPacket[tile] .. are consecutive, row bands outer, columns inner
	const int4 *tiles;
	const int *packetTile, *firstPacket;
	const long long *outOff;
	unsigned char *out;
	int resx, resy;
};

#if !SNAIL_ARITH_SSE
// the packets of the double-resolution frame behind packet p: 4 p + k at (2x + 16 (k & 1), 2y + 16 (k >> 1)) (src/render.cpp:72-77)
__global__ __launch_bounds__(256) void k_inst_aa_packets(const int2 *xy, int nPackets, int2 *xy2) {
	const int i = (int)(blockIdx.x * 256 + threadIdx.x);
	if(i >= nPackets * 4) return;
	const int2 p = xy[i >> 2];
	const int k = i & 3;
	xy2[i] = make_int2(p.x * 2 + ((k & 1) ? 16 : 0), p.y * 2 + ((k & 2) ? 16 : 0));
}
#endif

// One wave per output packet, lane = output quad (row lane >> 2, pixels 4 (lane & 3) .. + 3).  The reduction is k_aa_reduce's: the same quad
// mapping, out = ((a0 + b0) * 0.25) + ((a1 + b1) * 0.25); the depth colour is k_shade_depth's Inv(t) * (20, 250, 2); the planes follow
// k_bgr_to_planar's index rule (byte ty * w + tx of plane k of a w x h tile), clipped to the tile's rect and to the image.
template <bool DEPTH, bool AA, bool PLANAR>
__global__ __launch_bounds__(64) void k_inst_store(InstStoreArgs A) {
	const int p = (int)blockIdx.x, lane = (int)threadIdx.x;
	if(p >= A.nPackets) return;
	const int row = lane >> 2, qc = lane & 3;
	float c[4][3];   // [pixel of the quad][r, g, b]
	if(AA) {
		const int k = (row >= 8 ? 2 : 0) + (qc >= 2 ? 1 : 0);     // the quarter of the packet = the sub-packet it comes from
		const int r = row & 7, h = qc & 1;
#pragma unroll
		for(int j = 0; j < 4; j++) {
			const int i = j >> 1, s2 = (j & 1) * 2;
			const int qa = 8 * r + 2 * h + i, qb = qa + 4;          // the input quads of rows 2r and 2r + 1
			const size_t ia = ((size_t)(4 * p + k) * 64 + qa) * 4 + s2, ib = ((size_t)(4 * p + k) * 64 + qb) * 4 + s2;
			float ta0 = 0.0f, ta1 = 0.0f, tb0 = 0.0f, tb1 = 0.0f;
			if(DEPTH) { ta0 = InvDiv(A.in[ia]); ta1 = InvDiv(A.in[ia + 1]); tb0 = InvDiv(A.in[ib]); tb1 = InvDiv(A.in[ib + 1]); }
#pragma unroll
			for(int ch = 0; ch < 3; ch++) {
				float a0, a1, b0, b1;
				if(DEPTH) {
					const float scale = ch == 0 ? 20.0f : ch == 1 ? 250.0f : 2.0f;
					a0 = ta0 * scale; a1 = ta1 * scale; b0 = tb0 * scale; b1 = tb1 * scale;
				} else { a0 = A.in[ia * 3 + ch]; a1 = A.in[(ia + 1) * 3 + ch]; b0 = A.in[ib * 3 + ch]; b1 = A.in[(ib + 1) * 3 + ch]; }
				c[j][ch] = (a0 + b0) * 0.25f + (a1 + b1) * 0.25f;
			}
		}
	} else {
		const size_t q = ((size_t)p * 64 + (size_t)lane) * 4;
		if(DEPTH) {
			const float4 tv = *(const float4 *)(A.in + q);
			const float tt[4] = {tv.x, tv.y, tv.z, tv.w};
#pragma unroll
			for(int l = 0; l < 4; l++) {
				const float dist = InvDiv(tt[l]);
				c[l][0] = dist * 20.0f; c[l][1] = dist * 250.0f; c[l][2] = dist * 2.0f;
			}
		} else {
			const float4 *s = (const float4 *)(A.in + q * 3);
			const float4 v0 = s[0], v1 = s[1], v2 = s[2];
			const float f[12] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w};
#pragma unroll
			for(int l = 0; l < 4; l++) { c[l][0] = f[l * 3]; c[l][1] = f[l * 3 + 1]; c[l][2] = f[l * 3 + 2]; }
		}
	}
	if(A.tinted) {
#pragma unroll
		for(int l = 0; l < 4; l++)
#pragma unroll
			for(int ch = 0; ch < 3; ch++) c[l][ch] = (c[l][ch] + 0.1f) * A.tint[ch];
	}
	unsigned rr[4], gg[4], bb[4];
#pragma unroll
	for(int l = 0; l < 4; l++) { rr[l] = (unsigned)convChannelW(c[l][0]); gg[l] = (unsigned)convChannelW(c[l][1]); bb[l] = (unsigned)convChannelW(c[l][2]); }
	if(!PLANAR) {
		unsigned bytes[12];
#pragma unroll
		for(int l = 0; l < 4; l++) { bytes[l * 3 + 0] = bb[l]; bytes[l * 3 + 1] = gg[l]; bytes[l * 3 + 2] = rr[l]; }
		unsigned *o = (unsigned *)(A.bgrPackets + ((size_t)p * 256 + (size_t)lane * 4) * 3);
#pragma unroll
		for(int w = 0; w < 3; w++) o[w] = bytes[4 * w] | (bytes[4 * w + 1] << 8) | (bytes[4 * w + 2] << 16) | (bytes[4 * w + 3] << 24);
		return;
	}
	const int tile = A.packetTile[p];
	const int4 T = A.tiles[tile];
	const int ppr = (T.z + 15) >> 4, lp = p - A.firstPacket[tile];
	const int ty = (lp / ppr) * 16 + row, tx = (lp % ppr) * 16 + qc * 4;
	if(ty >= T.w || T.y + ty >= A.resy) return;
	int nIn = T.z - tx;                                        // pixels of the quad inside the tile and the image
	if(A.resx - (T.x + tx) < nIn) nIn = A.resx - (T.x + tx);
	if(nIn <= 0) return;
	const size_t n = (size_t)T.z * (size_t)T.w, i = (size_t)ty * (size_t)T.z + (size_t)tx;
	unsigned char *o = A.out + A.outOff[tile] + i;
	unsigned pl[3][4];
#pragma unroll
	for(int l = 0; l < 4; l++) { pl[0][l] = rr[l]; pl[1][l] = (gg[l] - rr[l]) & 255u; pl[2][l] = (bb[l] - rr[l]) & 255u; }
#pragma unroll
	for(int k = 0; k < 3; k++) {
		unsigned char *d = o + (size_t)k * n;
		if(nIn >= 4 && ((unsigned long long)d & 3) == 0) *(unsigned *)d = pl[k][0] | (pl[k][1] << 8) | (pl[k][2] << 16) | (pl[k][3] << 24);
		else {
#pragma unroll
			for(int l = 0; l < 4; l++)
				if(l < nIn) d[l] = (unsigned char)pl[k][l];
		}
	}
}

} // namespace SNAIL_DEV_NS
