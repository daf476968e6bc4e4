// materials_tree.inc -- the transparency continuation together with the one mirrored bounce of gVals[7] (include/snail_materials_tree.h).  Included
// once per arithmetic after materials_transparency.inc, into the same namespace (dev / dev_sse); one wave per packet, lane q = quad q, as there.
// With gVals[7] every RayTrace call of the A chain (cache.reflections == 0: the primary packets and their continuations) mirrors its own hit
// lanes and blends the nested call's colour into its diffuse BEFORE it continues through its transparent lanes (src/scene_trace.cpp:454-483), and
// the mirrored call (cache.reflections == 1) continues but never mirrors again.  Everything but two stages exists: the sample, generator, light,
// colour, blend and truncation stages of materials.inc / materials_transparency.inc run on the levels of both chains unchanged.  Here:
//   k_mat_mirror_rays      Scene::TraceReflection from a level's GENERIC packets (k_mat_mirror reads the primary ones), + the mirrored walk's order list
//   k_mat_blend_refl / _rays   the reflection blend as a stage of its own: it rewrites the diffuse planes of a level's sample buffer in place, so
//                          that k_mat_blend_transp, the lights and the colour stage run after it unchanged (the primary level: k_mat_final / k_mat_colour)
namespace SNAIL_DEV_NS {

struct TreeArgs {
	TranspArgs t;              // FIRST: its hostTab opens the kernel-argument segment.  t.m.s.rOrg / rDir / rMask (null: every lane selected) / rDist and
	                           // t.m.nSamples are the LEVEL's rays, hits and samples (matLoadSamples<SRC_MIRROR>); t.inOrder is the level's own order list
	float *oOrg, *oDir, *oIDir, *oDist;   // the mirrored packets, in the layout of k_mat_mirror's outputs
	int *oObj;
	unsigned char *oMask;
	int *oOrder;               // [packet]: the packet's index when it is part of the level, -1 otherwise
};

// ---- one packet: a level's generic packets and samples -> its mirrored packets.  Scene::TraceReflection (src/scene_trace.cpp:603-618) called by a
// nested RayTrace with cache.reflections == 0: dir is the level's ray, position = dir * t + origin, the selector is the lanes with their mask bit
// set and t < inf, the normal comes from the level's nested sample buffer.  A packet that is not part of the level writes its order word and
// nothing else; the mirrored call of one that is takes place even when none of its lanes hit (reflSel.Any() is commented out, :454), so such a
// packet stays in the list, as the bounce of the primary packets walks an all-miss packet.
// TWINS: the body -- Reflect, the origin's offset, the layout, zeros for masked lanes, SafeInv one component at a time through InvN<4> in the table
// arithmetic, distance inf / -inf, object 0, one mask byte per quad and the nested call's TracingRays -- is k_mat_mirror's (materials.inc), which
// names this kernel's source as its only difference; a change to either belongs in both.
// PSTATS (k_mat_mirror_rays_heat): the nested call's TracingRays per packet as well, as matMirror's; a packet that is not part of the level books nothing.
template <bool PSTATS>
__device__ __forceinline__ void matMirrorRays(const TreeArgs &G) {
	const TranspArgs &T = G.t;
	const MatArgs &A = T.m;
	const int lane = threadIdx.x & 63;
	const int li = (int)blockIdx.x;
	if(li >= A.s.nPackets) return;
	if(orderSkipped(T.inOrder, li)) {   // (wave-uniform)
		if(lane == 0) G.oOrder[li] = -1;
		return;
	}
	const PacketPos P = matPacket<SRC_MIRROR>(A, li);
	const size_t quad = P.pidx * 64 + lane;
	const float inf = __builtin_inff();
	Samples S;
	float d[3][4];
	loadQuad3(A.s.rDir, quad, d);
	matLoadSamples<SRC_MIRROR>(A, P, lane, S);
	float rd[3][4], ro[3][4], rdist[4];
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
		}
		rdist[l] = S.hit[l] ? inf : -inf;
		sel |= S.hit[l] ? (1u << l) : 0u;
	}
	float4 *po = (float4 *)(G.oOrg + quad * 12), *pd = (float4 *)(G.oDir + quad * 12), *pi = (float4 *)(G.oIDir + quad * 12);
#pragma unroll
	for(int c = 0; c < 3; c++) {
		po[c] = make_float4(ro[c][0], ro[c][1], ro[c][2], ro[c][3]);
		pd[c] = make_float4(rd[c][0], rd[c][1], rd[c][2], rd[c][3]);
	}
#pragma unroll
	for(int c = 0; c < 3; c++) {   // SafeInv (src/rtbase.h:117-120); table arithmetic: a component's four look-ups in one batch
		float x4[4], r4[4];
#pragma unroll
		for(int l = 0; l < 4; l++) x4[l] = rd[c][l] + 0.00000001f;
#if SNAIL_ARITH_SSE
		InvN<4>(x4, r4);
#else
#pragma unroll
		for(int l = 0; l < 4; l++) r4[l] = Inv(x4[l]);
#endif
		pi[c] = make_float4(r4[0], r4[1], r4[2], r4[3]);
	}
	G.oMask[quad] = (unsigned char)sel;
	*(float4 *)(G.oDist + quad * 4) = make_float4(rdist[0], rdist[1], rdist[2], rdist[3]);
	*(int4 *)(G.oObj + quad * 4) = make_int4(0, 0, 0, 0);
	if(lane == 0) G.oOrder[li] = li;
	unsigned cnt = 0;
#pragma unroll
	for(int l = 0; l < 4; l++) cnt += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(S.hit[l]));
	const Counters none = {0, 0, 0, 0, 0};
	flushStats(A.s.stats, none, cnt, lane);
	if(PSTATS) bookPacketLate<ShadeArgs>(P.pidx, none, cnt, lane);
}
__global__ __launch_bounds__(64) void k_mat_mirror_rays(TreeArgs G) { matMirrorRays<false>(G); }
__global__ __launch_bounds__(64) void k_mat_mirror_rays_heat(TreeArgs G) { matMirrorRays<true>(G); }

// ---- one packet: samples[q].diffuse += (reflColor - diffuse) * 0.3 on the hit lanes (= reflSel), specular untouched (src/scene_trace.cpp:462-465),
// in place in the level's sample buffer T.bSamples, the nested call's outColor in T.bCol (floats [packet][256][3]).  It comes BEFORE
// k_mat_blend_transp, as :462-465 precedes :479-481.  SRC_PRIMARY: a hit = t < inf of the primary hits; SRC_MIRROR: t < inf and the lane's mask
// bit.  Buffers are indexed by the list position (the note at k_mat_blend_transp).
// TWINS: the expression and its rounding -- df + (refl - df) * 0.3f, three separately rounded operations -- are matFinal<SRC_PRIMARY, BLEND>'s
// (materials.inc), which blends in registers on its way to the colour; a change to either belongs in both.
template <int SRC>
__device__ __forceinline__ void matBlendRefl(const TranspArgs &T) {
	const MatArgs &A = T.m;
	const int lane = threadIdx.x & 63;
	const int li = (int)blockIdx.x;
	if(li >= A.s.nPackets || orderSkipped(T.inOrder, li)) return;
	const size_t quad = (size_t)li * 64 + lane;
	const float inf = __builtin_inff();
	const float4 tv = *(const float4 *)((SRC == SRC_MIRROR ? A.s.rDist : A.s.hitT) + quad * 4);
	const float t[4] = {tv.x, tv.y, tv.z, tv.w};
	unsigned mask4 = 15u;
	if(SRC == SRC_MIRROR && A.s.rMask) mask4 = A.s.rMask[quad] & 15u;
	bool hit[4];
#pragma unroll
	for(int l = 0; l < 4; l++) hit[l] = t[l] < inf && ((mask4 >> l) & 1u) != 0;
	if(!(hit[0] || hit[1] || hit[2] || hit[3])) return;
	float4 *sm = (float4 *)(T.bSamples + (size_t)li * (9 * 256)) + lane;
#pragma unroll
	for(int c = 0; c < 3; c++) {
		const float4 dv = sm[(3 + c) * 64];
		float df[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
		for(int l = 0; l < 4; l++) {
			const float refl = T.bCol[(quad * 4 + l) * 3 + c];
			if(hit[l]) df[l] = df[l] + (refl - df[l]) * 0.3f;
		}
		sm[(3 + c) * 64] = make_float4(df[0], df[1], df[2], df[3]);
	}
}
__global__ __launch_bounds__(64) void k_mat_blend_refl(TranspArgs T) { matBlendRefl<SRC_PRIMARY>(T); }
__global__ __launch_bounds__(64) void k_mat_blend_refl_rays(TranspArgs T) { matBlendRefl<SRC_MIRROR>(T); }

} // namespace SNAIL_DEV_NS
