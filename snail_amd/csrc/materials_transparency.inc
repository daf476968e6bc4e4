// materials_transparency.inc -- transparent materials under full shading (include/snail_materials_transparency.h).  Included once per arithmetic
// after materials.inc, into the same namespace (dev / dev_sse); one wave per packet, lane q = quad q, the reference's block of 4 quads = lanes
// 4b .. 4b + 3 (a DPP quad), as there.
//   k_mat_sample_transp / k_mat_sample_transp_rays   the sample stage of k_mat_sample / k_mat_sample_rays with the kinds that can select a transparent
//                          lane (TransparentMaterial<NDotR>, src/shading/transparent_material.h; UberMaterial's dissFactor), Sample::opacity per ray
//                          and the transSel selector after the opacity < 1 filter (src/scene_trace.cpp:190, :306, :347-349, :472)
//   k_mat_light_transp / k_mat_colour_transp / k_mat_blend_transp / k_mat_truncated   the frames' way back up, at the end of this file
//   k_mat_continue / k_mat_continue_rays   Scene::TraceTransparency's packets (:620-634) from a level's rays, hits and selector, in the layout of
//                          k_mat_mirror, + the order word under which launchRays leaves out a packet without a selected lane (orderedSlot)
// Kernels of their own: the existing sample kernels stay the code they are, and a set they can be given never holds these kinds
// (checkMaterials).  The sample stage is matSample (materials.inc) with its [T] lines compiled in; the planes of a set without these kinds are
// k_mat_sample's / k_mat_sample_rays' byte for byte.
namespace SNAIL_DEV_NS {

struct TranspArgs {
	MatArgs m;                 // FIRST: its hostTab opens the kernel-argument segment
	float *opacity;            // sample stage: Sample::opacity [packet][256]
	unsigned char *sel;        // sample stage: transSel after the opacity filter, one byte per quad [packet][64]
	// generator: the level's rays (null: the camera's, generated again), hits and selector; outputs are m.s.rOrg / rDir / rIDir / rMask / rDist / rObj
	const float *cOrg, *cDir, *cIDir;
	const float *cT;
	const unsigned char *cSel;
	int *order;                // [packet]: the packet's index when any lane is selected, -1 otherwise
	// frames (level iteration): the level's OWN order list -- a packet whose word is negative is not part of the level's nested call and is
	// skipped by every stage of that level (null: the primary level, every packet) -- and the blend / truncation stages' buffers
	const int *inOrder;
	float *bSamples;           // blend: the level's sample buffer [packet][9][64][4], its diffuse planes are rewritten in place
	const float *bOpacity;     // ... its opacity [packet][256] and selector [packet][64]
	const unsigned char *bSel;
	const float *bCol;         // ... and the deeper level's outColor = transColor, floats [packet][256][3]
	unsigned long long *trunc; // truncation: += the lanes the deepest level would still select
};

// the sample stage with the [T] additions: matSample (materials.inc) with TRANSP on, behind the level's order list
__global__ __launch_bounds__(64) void k_mat_sample_transp(TranspArgs T) { matSample<SRC_PRIMARY, true, MatKey>(T.m, nullptr, T.inOrder, T.opacity, T.sel); }
__global__ __launch_bounds__(64) void k_mat_sample_transp_rays(TranspArgs T) { matSample<SRC_MIRROR, true, MatKey>(T.m, nullptr, T.inOrder, T.opacity, T.sel); }

// ---- one packet: a level's rays, hits and selector -> the next level's packets.  Scene::TraceTransparency (src/scene_trace.cpp:620-634): origin =
// dir * (distance + 0.001) + origin per ray, dir and idir as the caller's RayGroup carries them (the primary one: idir = SafeInv(dir)); the
// packet goes as RayGroup<0, 0> when all 256 lanes are selected, else as RayGroup<0, 1>: the mask byte says which.
// TWINS: the output -- layout, zeros for masked lanes (SafeInv(0) in idir), distance inf / -inf (:112-115), object 0, one mask byte per quad, the
// nested call's TracingRays(CountMaskBits(mask)) (:116-117) -- is k_mat_mirror's (materials.inc) and k_final<SRC_PRIMARY, DST_CONTINUE>'s (snail_dev.inc).
// PSTATS (k_mat_continue_heat / _rays_heat): the nested call's TracingRays per packet as well (matLight's note, materials.inc); a packet that makes
// no nested call -- none of its lanes selected, or absent from its level -- books nothing.
template <int SRC, bool PSTATS = false>
__device__ __forceinline__ void matContinue(const TranspArgs &T) {
	const MatArgs &A = T.m;
	const int lane = threadIdx.x & 63;
	const int li = (int)blockIdx.x;
	if(li >= A.s.nPackets) return;
	const PacketPos P = matPacket<SRC>(A, li);
	const size_t quad = P.pidx * 64 + lane;
	const float inf = __builtin_inff();
	float d[3][4], org[3][4], id[3][4];
	if(SRC == SRC_MIRROR) {
		loadQuad3(T.cDir, quad, d);
		loadQuad3(T.cOrg, quad, org);
		loadQuad3(T.cIDir, quad, id);
	} else {
		matRays(A.s, P, lane, d);
#pragma unroll
		for(int c = 0; c < 3; c++)
#pragma unroll
			for(int l = 0; l < 4; l++) { org[c][l] = A.s.g.org[c]; id[c][l] = 0.0f; }
	}
	const float4 tv = *(const float4 *)(T.cT + quad * 4);
	const float tt[4] = {tv.x, tv.y, tv.z, tv.w};
	const unsigned selq = orderSkipped(T.inOrder, li) ? 0u : (T.cSel[quad] & 15u);   // (a packet outside its level's call selected nothing: its buffers were never written)
	float ro[3][4], rd[3][4], ri[3][4], rdist[4];
	unsigned sel = 0;
#pragma unroll
	for(int l = 0; l < 4; l++) {
		const bool on = tt[l] < inf && ((selq >> l) & 1u) != 0;
		const float tl = tt[l] + 0.001f;
#pragma unroll
		for(int c = 0; c < 3; c++) {
			rd[c][l] = on ? d[c][l] : 0.0f;
			ro[c][l] = on ? d[c][l] * tl + org[c][l] : 0.0f;
			const float si = Inv(rd[c][l] + 0.00000001f);   // SafeInv (src/rtbase.h:117-120)
			ri[c][l] = (SRC == SRC_MIRROR && on) ? id[c][l] : si;
		}
		rdist[l] = on ? inf : -inf;
		sel |= on ? (1u << l) : 0u;
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
	unsigned cnt = 0;
#pragma unroll
	for(int l = 0; l < 4; l++) cnt += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64((sel >> l) & 1u));
	// a packet without a selected lane makes NO nested call (:474): its word takes it out of the walk's order list
	if(lane == 0) T.order[P.pidx] = cnt ? li : -1;
	const Counters none = {0, 0, 0, 0, 0};
	flushStats(A.s.stats, none, cnt, lane);
	if(PSTATS && cnt) bookPacketLate<ShadeArgs>(P.pidx, none, cnt, lane);
}
__global__ __launch_bounds__(64) void k_mat_continue(TranspArgs T) { matContinue<SRC_PRIMARY>(T); }
__global__ __launch_bounds__(64) void k_mat_continue_rays(TranspArgs T) { matContinue<SRC_MIRROR>(T); }
__global__ __launch_bounds__(64) void k_mat_continue_heat(TranspArgs T) { matContinue<SRC_PRIMARY, true>(T); }
__global__ __launch_bounds__(64) void k_mat_continue_rays_heat(TranspArgs T) { matContinue<SRC_MIRROR, true>(T); }

// ---- the way back up (include/snail_materials_transparency.h, frames).  The nested call's lights and outColor are matLight / matFinal of
// materials.inc on the level's generic packets (SRC_MIRROR: rays, masks, hits, samples and shadow distances of that level), left out for a packet
// that is not part of the level's call; the blend samples[q].diffuse = VLerp(transColor, diffuse, opacity) on the selected lanes (:479-481,
// veclib/vecbase.h:81: a + (b - a) * x) happens BEFORE the lights and touches nothing else, so it is a stage of its own that rewrites the
// diffuse planes of the level's sample buffer, after which the existing light and colour stages run unchanged.
template <bool DEEP>
__global__ __launch_bounds__(64) void k_mat_light_transp(TranspArgs T) {
	__shared__ float lds[LDS_FLOATS_PER_WAVE];
	if((int)blockIdx.x >= T.m.s.nPackets || orderSkipped(T.inOrder, (int)blockIdx.x)) return;
	matLight<DEEP, SRC_MIRROR>(T.m, lds);
}
template <bool DEEP>
__global__ __launch_bounds__(64) void k_mat_light_transp_heat(TranspArgs T) {
	__shared__ float lds[LDS_FLOATS_PER_WAVE];
	if((int)blockIdx.x >= T.m.s.nPackets || orderSkipped(T.inOrder, (int)blockIdx.x)) return;
	matLight<DEEP, SRC_MIRROR, true>(T.m, lds);
}
__global__ __launch_bounds__(64) void k_mat_colour_transp(TranspArgs T) {
	if((int)blockIdx.x >= T.m.s.nPackets || orderSkipped(T.inOrder, (int)blockIdx.x)) return;
	matFinal<SRC_MIRROR, false>(T.m);
}
// (this stage and k_mat_truncated index the level's buffers by the list position li, as matPacket<SRC_MIRROR> does: the frames always run over a
// packet list -- frameSet takes the whole frame's when the caller brings none -- so the primary level's P.pidx is li as well)
__global__ __launch_bounds__(64) void k_mat_blend_transp(TranspArgs T) {
	const int lane = threadIdx.x & 63;
	const int li = (int)blockIdx.x;
	if(li >= T.m.s.nPackets || orderSkipped(T.inOrder, li)) return;
	const size_t quad = (size_t)li * 64 + lane;
	const unsigned sel = T.bSel[quad] & 15u;
	if(!sel) return;
	const float4 ov = *(const float4 *)(T.bOpacity + quad * 4);
	const float op[4] = {ov.x, ov.y, ov.z, ov.w};
	float4 *sm = (float4 *)(T.bSamples + (size_t)li * (9 * 256)) + lane;
#pragma unroll
	for(int c = 0; c < 3; c++) {
		const float4 dv = sm[(3 + c) * 64];
		float df[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
		for(int l = 0; l < 4; l++) {
			const float tc = T.bCol[(quad * 4 + l) * 3 + c];
			if((sel >> l) & 1u) df[l] = tc + (df[l] - tc) * op[l];
		}
		sm[(3 + c) * 64] = make_float4(df[0], df[1], df[2], df[3]);
	}
}
// the lanes that the deepest level asked for would still select: counted, and treated as not selected (no generator and no blend follows)
__global__ __launch_bounds__(64) void k_mat_truncated(TranspArgs T) {
	const int lane = threadIdx.x & 63;
	const int li = (int)blockIdx.x;
	if(li >= T.m.s.nPackets || orderSkipped(T.inOrder, li)) return;
	const unsigned sel = T.bSel[(size_t)li * 64 + lane] & 15u;
	unsigned cnt = 0;
#pragma unroll
	for(int l = 0; l < 4; l++) cnt += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64((sel >> l) & 1u));
	if(lane == 0 && cnt) atomicAdd(T.trunc, (unsigned long long)cnt);
}

} // namespace SNAIL_DEV_NS
