// materials_transparency.inc -- transparent materials under full shading (include/snail_materials_transparency.h).  Included once per arithmetic
// after materials.inc, into the same namespace (dev / dev_sse); one wave per packet, lane q = quad q, the reference's block of 4 quads = lanes
// 4b .. 4b + 3 (a DPP quad), as there.
//   k_mat_sample_transp / k_mat_sample_transp_rays   the sample stage of k_mat_sample / k_mat_sample_rays with the kinds that can select a transparent
//                          lane (TransparentMaterial<NDotR>, src/shading/transparent_material.h; UberMaterial's dissFactor), Sample::opacity per ray
//                          and the transSel selector after the opacity < 1 filter (src/scene_trace.cpp:190, :306, :347-349, :472)
//   k_mat_light_transp / k_mat_colour_transp / k_mat_blend_transp / k_mat_truncated   the frames' way back up, at the end of this file
//   k_mat_continue / k_mat_continue_rays   Scene::TraceTransparency's packets (:620-634) from a level's rays, hits and selector, in the layout of
//                          k_mat_mirror, + the order word under which launchRays leaves out a packet without a selected lane (orderedSlot)
// Kernels of their own: the existing sample kernels stay as they are, and a set they can be given never holds these kinds (checkMaterials).
// TWINS: matSampleTransp is k_mat_sample / k_mat_sample_rays (materials.inc) with the additions marked [T]; a change to the branches, the kinds
// or the nine planes there belongs here too -- the planes of a set without these kinds are theirs byte for byte.  imatSampleTransp
// (instances_materials_transparency.inc) carries the same [T] additions for instanced scenes: a change to them belongs there too.
namespace SNAIL_DEV_NS {

enum { MAT_TRANSPARENT = 3 };
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
__device__ __forceinline__ bool transpSkipped(const TranspArgs &T, int li) { return T.inOrder && __builtin_amdgcn_readfirstlane(T.inOrder[li]) < 0; }

// broadcast of lane I of the block (quad_perm [I, I, I, I])
template <int I>
__device__ __forceinline__ int blockLane(int v) { return __builtin_amdgcn_mov_dpp(v, I * 0x55, 0xf, 0xf, true); }

template <int SRC>
__device__ __forceinline__ void matSampleTransp(const TranspArgs &T) {
	const MatArgs &A = T.m;
	const int lane = threadIdx.x & 63;
	const int li = (int)blockIdx.x;
	if(li >= A.s.nPackets || transpSkipped(T, li)) return;
	const PacketPos P = matPacket<SRC>(A, li);
	const size_t quad = P.pidx * 64 + lane;
	const float inf = __builtin_inff();
	float d[3][4];
	unsigned mask4 = 15u;
	if(SRC == SRC_MIRROR) {
		loadQuad3(A.s.rDir, quad, d);
		if(A.s.rMask) mask4 = A.s.rMask[quad] & 15u;
	} else matRays(A.s, P, lane, d);
	// hasMask is the PACKET's: RayGroup<0, 0> when all 256 lanes are selected, RayGroup<0, 1> otherwise (src/scene_trace.cpp:615-617, :631-633)
	const bool pktMasked = SRC == SRC_MIRROR && __builtin_amdgcn_ballot_w64(mask4 != 15u) != 0;
	float bx[4], by[4];
	bool hit[4];
	int obj[4];
	{
		const size_t uvq = SRC == SRC_MIRROR ? quad * (size_t)A.rUVStride : quad * 4;
		const float4 tv = *(const float4 *)((SRC == SRC_MIRROR ? A.s.rDist : A.s.hitT) + quad * 4);
		const float4 uv = *(const float4 *)((SRC == SRC_MIRROR ? A.rU : A.hitU) + uvq), vv = *(const float4 *)((SRC == SRC_MIRROR ? A.rV : A.hitV) + uvq);
		const int4 iv = *(const int4 *)((SRC == SRC_MIRROR ? (const int *)A.s.rObj : A.s.hitId) + quad * 4);
		const float t[4] = {tv.x, tv.y, tv.z, tv.w};
		const int id[4] = {iv.x, iv.y, iv.z, iv.w};
		bx[0] = uv.x; bx[1] = uv.y; bx[2] = uv.z; bx[3] = uv.w;
		by[0] = vv.x; by[1] = vv.y; by[2] = vv.z; by[3] = vv.w;
#pragma unroll
		for(int l = 0; l < 4; l++) {
			hit[l] = t[l] < inf && ((mask4 >> l) & 1u) != 0;   // mask = tDistance < maxDist && selector, :157
			int i = id[l] < 0 ? 0 : id[l];
			i = i < A.nTris ? i : A.nTris - 1;
			obj[l] = hit[l] ? i : 0;       // object = Condition(mask, tObject, 0), :161
		}
	}
	const bool full = blockAll(hit[0] && hit[1] && hit[2] && hit[3], lane);
	const int obj0b = blockFirst(obj[0]);
	const bool single = blockAll(obj[0] == obj0b && obj[1] == obj0b && obj[2] == obj0b && obj[3] == obj0b, lane) && full;

	float nrm[3][4], tc[2][4], tdx = 0.0f, tdy = 0.0f;
	int mid[4];
#pragma unroll
	for(int l = 0; l < 4; l++) { nrm[0][l] = nrm[1][l] = nrm[2][l] = 0.0f; tc[0][l] = tc[1][l] = 0.0f; mid[l] = -1; }
	if(single) {
		// (a): one triangle for the block
		const ShTri S = loadShTri(A, obj0b);
		const int m = matIdOf(A, S.matId);
		const bool flat = S.matId < 0;
		const int mk = m >= 0 ? A.mats[m].kind : MAT_SIMPLE;
		const bool texd = mk == MAT_TEX || mk == MAT_TRANSPARENT;     // Material::fTexCoords  [T]: TransparentMaterial carries it too
#pragma unroll
		for(int l = 0; l < 4; l++) {
			mid[l] = m;
			if(texd) {
#pragma unroll
				for(int c = 0; c < 2; c++) tc[c][l] = lerpL(S.uv[0][c], S.uv[1][c], S.uv[2][c], bx[l], by[l]);
#pragma unroll
				for(int c = 0; c < 3; c++) nrm[c][l] = lerpL(S.nrm[0][c], S.nrm[1][c], S.nrm[2][c], bx[l], by[l]);
			} else {
#pragma unroll
				for(int c = 0; c < 3; c++) nrm[c][l] = flat ? S.nrm[0][c] : lerpR(S.nrm[0][c], S.nrm[1][c], S.nrm[2][c], bx[l], by[l]);
			}
		}
		if(texd) {
			tdx = vmax(vmax(tc[0][0], tc[0][1]), vmax(tc[0][2], tc[0][3])) - vmin(vmin(tc[0][0], tc[0][1]), vmin(tc[0][2], tc[0][3]));
			tdy = vmax(vmax(tc[1][0], tc[1][1]), vmax(tc[1][2], tc[1][3])) - vmin(vmin(tc[1][0], tc[1][1]), vmin(tc[1][2], tc[1][3]));
		}
	} else {
		// (b): per quad
		if(hit[0]) {
			const ShTri S = loadShTri(A, obj[0]);
			const int m = matIdOf(A, S.matId);
#pragma unroll
			for(int l = 0; l < 4; l++) {
				mid[l] = hit[l] ? m : -1;
#pragma unroll
				for(int c = 0; c < 2; c++) tc[c][l] = lerpL(S.uv[0][c], S.uv[1][c], S.uv[2][c], bx[l], by[l]);
#pragma unroll
				for(int c = 0; c < 3; c++) nrm[c][l] = lerpL(S.nrm[0][c], S.nrm[1][c], S.nrm[2][c], bx[l], by[l]);
			}
		}
#pragma unroll
		for(int l = 1; l < 4; l++)
			if(hit[l] && obj[l] != obj[0]) {
				const ShTri S = loadShTri(A, obj[l]);
				mid[l] = matIdOf(A, S.matId);
#pragma unroll
				for(int c = 0; c < 2; c++) tc[c][l] = lerpL(S.uv[0][c], S.uv[1][c], S.uv[2][c], bx[l], by[l]);
#pragma unroll
				for(int c = 0; c < 3; c++) nrm[c][l] = lerpL(S.nrm[0][c], S.nrm[1][c], S.nrm[2][c], bx[l], by[l]);
			}
	}
	const int mid0b = blockFirst(mid[0]);
	const bool unmasked = blockAll(mid[0] == mid0b && mid[1] == mid0b && mid[2] == mid0b && mid[3] == mid0b, lane) && full && !(single && pktMasked);

	float diff[3][4], spec[3][4], opac[4];
	int flagged[4];   // [T] the lane's material when it carries Material::fTransparency and the lane is selected, else -1
#pragma unroll
	for(int l = 0; l < 4; l++) {
		int kind = MAT_SIMPLE, ndotr = 1, tex = 0, tex2 = 0;
		float col[3] = {1.0f, 1.0f, 1.0f}, sp[3] = {0.0f, 0.0f, 0.0f}, dissolve = 0.0f;   // defaultMat = SimpleMaterial<true>(1, 1, 1), src/scene.cpp:6
		if(mid[l] >= 0) {
			const uint4 *r = (const uint4 *)(A.mats + mid[l]);
			const uint4 a = r[0], b = r[1], c = r[2];
			kind = (int)a.x; ndotr = (int)a.y;
			col[0] = asf(a.z); col[1] = asf(a.w); col[2] = asf(b.x);
			sp[0] = asf(b.y); sp[1] = asf(b.z); sp[2] = asf(b.w);
			tex = (int)c.x; tex2 = (int)c.y; dissolve = asf(c.z);   // [T] MatRec::pad[0], pad[1]: the opacity map, the dissolve factor
		}
		const float dn = d[0][l] * nrm[0][l] + d[1][l] * nrm[1][l] + d[2][l] * nrm[2][l];
		const float adn = __builtin_fabsf(dn);
		float t1[3] = {0.0f, 0.0f, 0.0f}, t2[3] = {0.0f, 0.0f, 0.0f};
		if(__builtin_amdgcn_ballot_w64(kind == MAT_TEX && hit[l]) != 0) {
			if(kind == MAT_TEX && hit[l]) matSampleTex(A, tex, tc[0][l], tc[1][l], tdx, tdy, t1);
		}
		// [T] TransparentMaterial::Shade_: both samplers with mipmapping off (Sample(samples, sc, 0)) -- level 0 whatever texDiff says
		if(__builtin_amdgcn_ballot_w64(kind == MAT_TRANSPARENT && hit[l]) != 0) {
			if(kind == MAT_TRANSPARENT && hit[l]) {
				matSampleTex(A, tex, tc[0][l], tc[1][l], 0.0f, 0.0f, t1);
				matSampleTex(A, tex2, tc[0][l], tc[1][l], 0.0f, 0.0f, t2);
			}
		}
#pragma unroll
		for(int c = 0; c < 3; c++) {
			float df, sf;
			if(kind == MAT_TEX || kind == MAT_TRANSPARENT) { df = ndotr ? t1[c] * dn : t1[c]; sf = df; }
			else if(kind == MAT_UBER) { df = col[c] * adn; sf = unmasked ? df : sp[c]; }
			else { df = ndotr ? col[c] * adn : col[c]; sf = df; }
			diff[c][l] = hit[l] ? df : 0.0f;
			spec[c][l] = hit[l] ? sf : 0.0f;
			nrm[c][l] = hit[l] ? nrm[c][l] : 0.0f;
		}
		// [T] Sample::opacity: temp1.x of the opacity sampler / dissFactor; the other kinds never write it (read before written: zero)
		const float op = kind == MAT_TRANSPARENT ? t2[0] : kind == MAT_UBER ? dissolve : 0.0f;
		opac[l] = hit[l] ? op : 0.0f;
		const bool fl = kind == MAT_TRANSPARENT || (kind == MAT_UBER && dissolve > 0.0f);   // UberMaterial: fTransparency iff dissolveFactor > 0
		flagged[l] = (hit[l] && fl) ? mid[l] : -1;
	}
	// [T] transSel.  (a) / (b): the block's one material's flag for the whole block (:190, :306).  (c): for each material of the block's list that
	// carries the flag, IN THE LIST'S ORDER -- first appearance over the quads, then the lanes, among the selected lanes -- transSel[b4 + q] =
	// mask[q] is ASSIGNED for all four quads (:347-349): the last flagged material of the list wins.  One rule covers the three branches: the
	// winner is the flagged material whose first appearance comes latest; a block of one material has one candidate.
	unsigned sel = 0;
	if(__builtin_amdgcn_ballot_w64((flagged[0] & flagged[1] & flagged[2] & flagged[3]) != -1) != 0) {
		int e[16];
#pragma unroll
		for(int l = 0; l < 4; l++) {
			e[0 + l] = blockLane<0>(flagged[l]); e[4 + l] = blockLane<1>(flagged[l]);
			e[8 + l] = blockLane<2>(flagged[l]); e[12 + l] = blockLane<3>(flagged[l]);
		}
		int win = -1;
#pragma unroll
		for(int p = 0; p < 16; p++) {
			bool first = e[p] >= 0;
#pragma unroll
			for(int k = 0; k < p; k++) first = first && e[k] != e[p];
			win = first ? e[p] : win;
		}
#pragma unroll
		for(int l = 0; l < 4; l++)
			sel |= (win >= 0 && flagged[l] == win && opac[l] < 1.0f) ? (1u << l) : 0u;   // transSel[q] &= ForWhich(opacity < 1.0f), :472
	}
	float4 *o = (float4 *)((SRC == SRC_MIRROR ? A.nSamples : A.samples) + P.pidx * (9 * 256)) + lane;
#pragma unroll
	for(int c = 0; c < 3; c++) {
		o[(0 + c) * 64] = make_float4(nrm[c][0], nrm[c][1], nrm[c][2], nrm[c][3]);
		o[(3 + c) * 64] = make_float4(diff[c][0], diff[c][1], diff[c][2], diff[c][3]);
		o[(6 + c) * 64] = make_float4(spec[c][0], spec[c][1], spec[c][2], spec[c][3]);
	}
	*(float4 *)(T.opacity + quad * 4) = make_float4(opac[0], opac[1], opac[2], opac[3]);
	T.sel[quad] = (unsigned char)sel;
}
__global__ __launch_bounds__(64) void k_mat_sample_transp(TranspArgs T) { matSampleTransp<SRC_PRIMARY>(T); }
__global__ __launch_bounds__(64) void k_mat_sample_transp_rays(TranspArgs T) { matSampleTransp<SRC_MIRROR>(T); }

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
	const unsigned selq = transpSkipped(T, li) ? 0u : (T.cSel[quad] & 15u);   // (a packet outside its level's call selected nothing: its buffers were never written)
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
	if((int)blockIdx.x >= T.m.s.nPackets || transpSkipped(T, (int)blockIdx.x)) return;
	matLight<DEEP, SRC_MIRROR>(T.m, lds);
}
template <bool DEEP>
__global__ __launch_bounds__(64) void k_mat_light_transp_heat(TranspArgs T) {
	__shared__ float lds[LDS_FLOATS_PER_WAVE];
	if((int)blockIdx.x >= T.m.s.nPackets || transpSkipped(T, (int)blockIdx.x)) return;
	matLight<DEEP, SRC_MIRROR, true>(T.m, lds);
}
__global__ __launch_bounds__(64) void k_mat_colour_transp(TranspArgs T) {
	if((int)blockIdx.x >= T.m.s.nPackets || transpSkipped(T, (int)blockIdx.x)) return;
	matFinal<SRC_MIRROR, false>(T.m);
}
// (this stage and k_mat_truncated index the level's buffers by the list position li, as matPacket<SRC_MIRROR> does: the frames always run over a
// packet list -- matTranspDev makes the whole frame's when the caller brings none -- so the primary level's P.pidx is li as well)
__global__ __launch_bounds__(64) void k_mat_blend_transp(TranspArgs T) {
	const int lane = threadIdx.x & 63;
	const int li = (int)blockIdx.x;
	if(li >= T.m.s.nPackets || transpSkipped(T, li)) return;
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
	if(li >= T.m.s.nPackets || transpSkipped(T, li)) return;
	const unsigned sel = T.bSel[(size_t)li * 64 + lane] & 15u;
	unsigned cnt = 0;
#pragma unroll
	for(int l = 0; l < 4; l++) cnt += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64((sel >> l) & 1u));
	if(lane == 0 && cnt) atomicAdd(T.trunc, (unsigned long long)cnt);
}

} // namespace SNAIL_DEV_NS
