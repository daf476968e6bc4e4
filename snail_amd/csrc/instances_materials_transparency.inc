// instances_materials_transparency.inc -- transparent materials under full shading of an instanced scene
// (include/snail_instances_materials_transparency.h): the transparency continuation of Scene<DBVH>::RayTrace (src/scene_trace.cpp:468-483) and
// Scene::TraceTransparency (:620-634, instantiated for DBVH at :657-659).  Included once per arithmetic after instances_materials_bounce.inc and
// materials_transparency.inc, into the same namespace (dev / dev_sse); one wave per packet or per (packet, light), lane q = quad q, the
// reference's block of 4 quads = lanes 4b .. 4b + 3 (a DPP quad), wave-uniform control flow, as there.
//   k_imat_sample_transp / k_imat_sample_transp_rays   k_imat_sample / k_imat_sample_rays with the [T] additions of matSampleTransp: the kinds that
//                          can select a transparent lane, Sample::opacity per ray and the transSel selector after the opacity < 1 filter
//   k_imat_trace_level<DEEP>   DBVH::TraversePrimary<0, 1> of a level's generated packets, with barycentrics, under the generator's order list
//   k_imat_light_transp<DEEP>  a level's lights: one wave per (packet, light), DBVH::TraverseShadow, under the level's order list
// Unchanged, because they read nothing of the scene: k_mat_continue / k_mat_continue_rays, k_mat_blend_transp, k_mat_colour_transp,
// k_mat_truncated (materials_transparency.inc); for the primary level k_inst_frame, k_imat_light and k_mat_final.
// Kernels of their own: the existing sample, walk and light kernels stay as they are, and a set they can be given never holds these kinds
// (checkIMat).  Table look-ups in their fully checked form.
namespace SNAIL_DEV_NS {

struct ITranspArgs {
	IMatArgs a;                // FIRST: its hostTab opens the kernel-argument segment.  Primary level: a.m.s.hitT / hitId / a.m.hitU / hitV / a.hitInst; a generic
	                           // level: a.m.s.rDir / rMask / rDist / rObj (triIds), a.m.rU / rV / rUVStride, a.m.nSamples, as k_imat_sample_rays reads and writes them
	const int *rInst;          // instance slot of a generic level's hits, indexed by list position
	float *opacity;            // sample stage: Sample::opacity [packet][256]
	unsigned char *sel;        // sample stage: transSel after the opacity filter, one byte per quad [packet][64]
	const int *inOrder;        // the level's OWN order list (TranspArgs::inOrder): a packet whose word is negative is skipped by every stage of the level; null: every packet
};
struct ILevelArgs {
	InstArgs i;                // FIRST (hostTab).  The generic packets of k_inst_trace: size, origin, dir, idir, mask, distance, object, element, bary, stats
	const int *order;          // the generator's order list: a packet whose word is negative is not walked
};
__device__ __forceinline__ bool imatSkipped(const int *order, int li) { return order && __builtin_amdgcn_readfirstlane(order[li]) < 0; }

// TWINS: this body is THREE kernels' at once, and a change to any of them belongs here too:
//   k_imat_sample (instances_materials.inc)            the keys (slot, triId), their clamps, the (slot 0, triId 0) quirk, imatLoadTri, the primary input side
//   k_imat_sample_rays (instances_materials_bounce.inc) the generic input side: directions, mask, bary stride, hit = t < inf AND the mask bit, the packet's hasMask
//   matSampleTransp (materials_transparency.inc)        the additions marked [T]: MAT_TRANSPARENT (fTexCoords, both maps at mip level 0), opac, flagged, the
//                                                      16-entry winner scan through blockLane<I>, the opacity < 1 filter, the level's inOrder skip
// and through them k_mat_sample / k_mat_sample_rays (materials.inc): blocks, texDiff, the mip choice, the kinds, the nine planes -- which for a set
// without the [T] kinds are k_imat_sample's / k_imat_sample_rays' byte for byte.  A material's identity in the winner scan is its index in the ONE
// scene-wide list: two BLASes' triangles of one entry are one candidate.
template <int SRC>
__device__ __forceinline__ void imatSampleTransp(const ITranspArgs &B) {
	const IMatArgs &A = B.a;
	const int lane = threadIdx.x & 63;
	const int li = (int)blockIdx.x;
	if(li >= A.m.s.nPackets || imatSkipped(B.inOrder, li)) return;
	const PacketPos P = matPacket<SRC>(A.m, li);
	const size_t quad = P.pidx * 64 + lane;
	const float inf = __builtin_inff();
	float d[3][4];
	unsigned mask4 = 15u;
	if(SRC == SRC_MIRROR) {
		loadQuad3(A.m.s.rDir, quad, d);
		if(A.m.s.rMask) mask4 = A.m.s.rMask[quad] & 15u;
	} else matRays(A.m.s, P, lane, d);
	// hasMask is the PACKET's: RayGroup<0, 0> when all 256 lanes are selected, RayGroup<0, 1> otherwise (src/scene_trace.cpp:615-617, :631-633)
	const bool pktMasked = SRC == SRC_MIRROR && __builtin_amdgcn_ballot_w64(mask4 != 15u) != 0;
	float bx[4], by[4];
	bool hit[4];
	int obj[4], slt[4];
	{
		const size_t uvq = SRC == SRC_MIRROR ? quad * (size_t)A.m.rUVStride : quad * 4;
		const float4 tv = *(const float4 *)((SRC == SRC_MIRROR ? A.m.s.rDist : A.m.s.hitT) + quad * 4);
		const float4 uv = *(const float4 *)((SRC == SRC_MIRROR ? A.m.rU : A.m.hitU) + uvq), vv = *(const float4 *)((SRC == SRC_MIRROR ? A.m.rV : A.m.hitV) + uvq);
		const int4 iv = *(const int4 *)((SRC == SRC_MIRROR ? (const int *)A.m.s.rObj : A.m.s.hitId) + quad * 4);
		const int4 sv = *(const int4 *)((SRC == SRC_MIRROR ? B.rInst : A.hitInst) + quad * 4);
		const float t[4] = {tv.x, tv.y, tv.z, tv.w};
		const int id[4] = {iv.x, iv.y, iv.z, iv.w};
		const int sl[4] = {sv.x, sv.y, sv.z, sv.w};
		bx[0] = uv.x; bx[1] = uv.y; bx[2] = uv.z; bx[3] = uv.w;
		by[0] = vv.x; by[1] = vv.y; by[2] = vv.z; by[3] = vv.w;
#pragma unroll
		for(int l = 0; l < 4; l++) {
			hit[l] = t[l] < inf && ((mask4 >> l) & 1u) != 0;   // mask = tDistance < maxDist && selector, :157
			int s = sl[l] < 0 ? 0 : sl[l];
			s = s < A.nSlots ? s : A.nSlots - 1;
			const int i = id[l] < 0 ? 0 : id[l];   // (its upper bound is the BLAS's, in imatLoadTri)
			slt[l] = hit[l] ? s : 0;       // object = Condition(mask, tObject, 0), :161
			obj[l] = hit[l] ? i : 0;       // element = Condition(mask, tElement, 0), :162
		}
	}
	// mask4 == 0x0f0f0f0f, and the 16 (object, element) pairs equal to the block's first (:178-182)
	const bool full = blockAll(hit[0] && hit[1] && hit[2] && hit[3], lane);
	const int obj0b = blockFirst(obj[0]), slt0b = blockFirst(slt[0]);
	const bool single = blockAll(obj[0] == obj0b && obj[1] == obj0b && obj[2] == obj0b && obj[3] == obj0b &&
								 slt[0] == slt0b && slt[1] == slt0b && slt[2] == slt0b && slt[3] == slt0b, lane) && full;

	float nrm[3][4], tc[2][4], tdx = 0.0f, tdy = 0.0f;
	int mid[4];
#pragma unroll
	for(int l = 0; l < 4; l++) { nrm[0][l] = nrm[1][l] = nrm[2][l] = 0.0f; tc[0][l] = tc[1][l] = 0.0f; mid[l] = -1; }
	if(single) {
		// (a): one triangle of one instance for the block
		int m;
		const ShTri T = imatLoadTri(A, slt0b, obj0b, m);
		const bool flat = T.matId < 0;
		const int mk = m >= 0 ? A.m.mats[m].kind : MAT_SIMPLE;
		const bool texd = mk == MAT_TEX || mk == MAT_TRANSPARENT;     // Material::fTexCoords  [T]: TransparentMaterial carries it too
#pragma unroll
		for(int l = 0; l < 4; l++) {
			mid[l] = m;
			if(texd) {
#pragma unroll
				for(int c = 0; c < 2; c++) tc[c][l] = lerpL(T.uv[0][c], T.uv[1][c], T.uv[2][c], bx[l], by[l]);
#pragma unroll
				for(int c = 0; c < 3; c++) nrm[c][l] = lerpL(T.nrm[0][c], T.nrm[1][c], T.nrm[2][c], bx[l], by[l]);
			} else {
#pragma unroll
				for(int c = 0; c < 3; c++) nrm[c][l] = flat ? T.nrm[0][c] : lerpR(T.nrm[0][c], T.nrm[1][c], T.nrm[2][c], bx[l], by[l]);
			}
		}
		if(texd) {   // texDiff = Maximize(texCoord) - Minimize(texCoord) of the quad (:219; finite values: the fold's order is immaterial)
			tdx = vmax(vmax(tc[0][0], tc[0][1]), vmax(tc[0][2], tc[0][3])) - vmin(vmin(tc[0][0], tc[0][1]), vmin(tc[0][2], tc[0][3]));
			tdy = vmax(vmax(tc[1][0], tc[1][1]), vmax(tc[1][2], tc[1][3])) - vmin(vmin(tc[1][0], tc[1][1]), vmin(tc[1][2], tc[1][3]));
		}
	} else {
		// (b): per quad; lane 0's triangle for all four lanes if lane 0 hit, then lanes 1..3 whose (slot, triId) differs from lane 0's ((0, 0) when
		// lane 0 missed or is masked: a lane that hit slot 0's triangle 0 beside it keeps the default material and zero normal / texCoord).  A record
		// is loaded and transformed only on lanes that hit.
		if(hit[0]) {
			int m;
			const ShTri T = imatLoadTri(A, slt[0], obj[0], m);
#pragma unroll
			for(int l = 0; l < 4; l++) {
				mid[l] = hit[l] ? m : -1;
#pragma unroll
				for(int c = 0; c < 2; c++) tc[c][l] = lerpL(T.uv[0][c], T.uv[1][c], T.uv[2][c], bx[l], by[l]);
#pragma unroll
				for(int c = 0; c < 3; c++) nrm[c][l] = lerpL(T.nrm[0][c], T.nrm[1][c], T.nrm[2][c], bx[l], by[l]);
			}
		}
#pragma unroll
		for(int l = 1; l < 4; l++)
			if(hit[l] && (obj[l] != obj[0] || slt[l] != slt[0])) {
				const ShTri T = imatLoadTri(A, slt[l], obj[l], mid[l]);
#pragma unroll
				for(int c = 0; c < 2; c++) tc[c][l] = lerpL(T.uv[0][c], T.uv[1][c], T.uv[2][c], bx[l], by[l]);
#pragma unroll
				for(int c = 0; c < 3; c++) nrm[c][l] = lerpL(T.nrm[0][c], T.nrm[1][c], T.nrm[2][c], bx[l], by[l]);
			}
	}
	// One material for 16 hit rays: Shade unmasked (:224, :301-308) -- the ids index ONE scene-wide list, so two BLASes' triangles of one material
	// meet here --; otherwise (c) every selected lane by its own material on the masked path (:310-355), each lane once: see k_mat_sample.
	// Branch (a) calls Shade with the packet's own hasMask (:224), (b)'s single-material call is RayGroup<.., 0> whatever the packet is (:308).
	const int mid0b = blockFirst(mid[0]);
	const bool unmasked = blockAll(mid[0] == mid0b && mid[1] == mid0b && mid[2] == mid0b && mid[3] == mid0b, lane) && full && !(single && pktMasked);

	float diff[3][4], spec[3][4], opac[4];
	int flagged[4];   // [T] the lane's material when it carries Material::fTransparency and the lane is selected, else -1
#pragma unroll
	for(int l = 0; l < 4; l++) {
		// the lane's material: loaded values of an unrolled loop (compile-time indices), never a runtime-indexed array
		int kind = MAT_SIMPLE, ndotr = 1, tex = 0, tex2 = 0;
		float col[3] = {1.0f, 1.0f, 1.0f}, sp[3] = {0.0f, 0.0f, 0.0f}, dissolve = 0.0f;   // defaultMat = SimpleMaterial<true>(1, 1, 1), src/scene.cpp:6
		if(mid[l] >= 0) {
			const uint4 *r = (const uint4 *)(A.m.mats + mid[l]);
			const uint4 a = r[0], b = r[1], c = r[2];
			kind = (int)a.x; ndotr = (int)a.y;
			col[0] = asf(a.z); col[1] = asf(a.w); col[2] = asf(b.x);
			sp[0] = asf(b.y); sp[1] = asf(b.z); sp[2] = asf(b.w);
			tex = (int)c.x; tex2 = (int)c.y; dissolve = asf(c.z);   // [T] MatRec::pad[0], pad[1]: the opacity map, the dissolve factor
		}
		const float dn = d[0][l] * nrm[0][l] + d[1][l] * nrm[1][l] + d[2][l] * nrm[2][l];
		const float adn = __builtin_fabsf(dn);
		float t1[3] = {0.0f, 0.0f, 0.0f}, t2[3] = {0.0f, 0.0f, 0.0f};
		// the kinds present among the wave's lanes: a branch per kind that needs code of its own, skipped when no lane has it
		if(__builtin_amdgcn_ballot_w64(kind == MAT_TEX && hit[l]) != 0) {
			if(kind == MAT_TEX && hit[l]) matSampleTex(A.m, tex, tc[0][l], tc[1][l], tdx, tdy, t1);
		}
		// [T] TransparentMaterial::Shade_: both samplers with mipmapping off (Sample(samples, sc, 0)) -- level 0 whatever texDiff says
		if(__builtin_amdgcn_ballot_w64(kind == MAT_TRANSPARENT && hit[l]) != 0) {
			if(kind == MAT_TRANSPARENT && hit[l]) {
				matSampleTex(A.m, tex, tc[0][l], tc[1][l], 0.0f, 0.0f, t1);
				matSampleTex(A.m, tex2, tc[0][l], tc[1][l], 0.0f, 0.0f, t2);
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
	// [T] transSel, matSampleTransp's one rule for the three branches: the winner is the flagged material whose first appearance -- over the quads,
	// then the lanes, among the selected lanes -- comes latest (:190, :306, :347-349); a block of one material has one candidate.
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
	float4 *o = (float4 *)((SRC == SRC_MIRROR ? A.m.nSamples : A.m.samples) + P.pidx * (9 * 256)) + lane;
#pragma unroll
	for(int c = 0; c < 3; c++) {
		o[(0 + c) * 64] = make_float4(nrm[c][0], nrm[c][1], nrm[c][2], nrm[c][3]);
		o[(3 + c) * 64] = make_float4(diff[c][0], diff[c][1], diff[c][2], diff[c][3]);
		o[(6 + c) * 64] = make_float4(spec[c][0], spec[c][1], spec[c][2], spec[c][3]);
	}
	*(float4 *)(B.opacity + quad * 4) = make_float4(opac[0], opac[1], opac[2], opac[3]);
	B.sel[quad] = (unsigned char)sel;
}
__global__ __launch_bounds__(64) void k_imat_sample_transp(ITranspArgs B) { imatSampleTransp<SRC_PRIMARY>(B); }
__global__ __launch_bounds__(64) void k_imat_sample_transp_rays(ITranspArgs B) { imatSampleTransp<SRC_MIRROR>(B); }

// ---- a level's walk: DBVH::TraversePrimary<0, 1>(Context&) of the generated packets, with barycentrics, under the generator's order list ----
// TWINS: the body is k_inst_trace<false, true, DEEP, true>'s (instances.inc: instWalk<false, true, false, true, DEEP>), behind the order word; a
// change there belongs here too.  A kernel of its own: k_inst_trace itself must not gain a pointer test -- its comment records that one cost the
// other launches' kernel scalar spills and, in one instantiation, a wave.  A packet that is not walked books no TreeStats and keeps its buffers.
template <bool DEEP>
__global__ __launch_bounds__(64) void k_imat_trace_level(ILevelArgs L) {
	__shared__ float lds[LDS_FLOATS_PER_WAVE];
	const InstArgs &A = L.i;
	const int lane = threadIdx.x & 63;
	const int p = (int)blockIdx.x;
	if(p >= A.nPackets || imatSkipped(L.order, p)) return;
	const int size = A.size;
	const bool live = lane < size;
	const size_t q = (size_t)p * size + (live ? lane : 0);
	float d[3][4], id[3][4], org[3][4];
	loadQuad3(A.dir, q, d);
	loadQuad3(A.idir, q, id);
	loadQuad3(A.origin, q, org);
	const unsigned mask4 = A.mask[q] & 15u;
	const float4 dv = *(const float4 *)(A.distance + q * 4);
	const int4 ov = *(const int4 *)(A.object + q * 4), ev = *(const int4 *)(A.element + q * 4);
	float dist[4] = {dv.x, dv.y, dv.z, dv.w};
	int obj[4] = {ov.x, ov.y, ov.z, ov.w}, elem[4] = {ev.x, ev.y, ev.z, ev.w};
	float bu[4], bv[4];
	{
		const float4 b0 = *(const float4 *)(A.bary + q * 8), b1 = *(const float4 *)(A.bary + q * 8 + 4);
		bu[0] = b0.x; bu[1] = b0.y; bu[2] = b0.z; bu[3] = b0.w;
		bv[0] = b1.x; bv[1] = b1.y; bv[2] = b1.z; bv[3] = b1.w;
	}
	Counters st = {0, 0, 0, 0, 0};
	instWalk<false, true, false, true, DEEP>(A, size, lane, org, d, id, mask4, dist, obj, elem, bu, bv, lds, st);
	flushStats(A.stats, st, 0u, lane);
	if(live) {
		*(float4 *)(A.distance + q * 4) = make_float4(dist[0], dist[1], dist[2], dist[3]);
		*(int4 *)(A.object + q * 4) = make_int4(obj[0], obj[1], obj[2], obj[3]);
		*(int4 *)(A.element + q * 4) = make_int4(elem[0], elem[1], elem[2], elem[3]);
		*(float4 *)(A.bary + q * 8) = make_float4(bu[0], bu[1], bu[2], bu[3]);
		*(float4 *)(A.bary + q * 8 + 4) = make_float4(bv[0], bv[1], bv[2], bv[3]);
	}
}

// ---- one (level packet, light): the nested call's shadow packet on the level's samples' normals, and DBVH::TraverseShadow ----
// TWINS: this is k_imat_light_rays<DEEP> (instances_materials_bounce.inc) behind the level's order word, as k_mat_light_transp is
// matLight<DEEP, SRC_MIRROR> behind transpSkipped (materials_transparency.inc); a change to k_imat_light_rays, or to what its own note names
// (matLight<DEEP, SRC_MIRROR>'s sample load and set-up, k_imat_light's walk and stats flush), belongs here too.
template <bool DEEP>
__global__ __launch_bounds__(64) void k_imat_light_transp(ITranspArgs B) {
	__shared__ float lds[LDS_FLOATS_PER_WAVE];
	const IMatArgs &A = B.a;
	const int lane = threadIdx.x & 63;
	const int li = (int)blockIdx.x, n = (int)blockIdx.y;
	if(li >= A.m.s.nPackets || n >= A.m.s.nLights || imatSkipped(B.inOrder, li)) return;
	const PacketPos P = matPacket<SRC_MIRROR>(A.m, li);
	const float lp[3] = {A.m.s.lights[n][0], A.m.s.lights[n][1], A.m.s.lights[n][2]};
	const float radius = A.m.s.lights[n][6], radSq = radius * radius;
	Quad Q;
	{
		Samples S;
		matLoadSamples<SRC_MIRROR>(A.m, P, lane, S);
		float tMin[3], tMax[3];
		hitBounds(S, tMin, tMax);
		if(lightCulled(tMin, tMax, lp, radSq)) return;   // (wave-uniform; k_mat_colour_transp skips the light by the same test)
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
	flushStats(A.m.s.stats, st, rays, lane);
	*(float4 *)(A.m.nSDist + ((size_t)n * (size_t)A.m.s.nPackets + P.pidx) * 256 + (size_t)lane * 4) = make_float4(Q.dist[0], Q.dist[1], Q.dist[2], Q.dist[3]);
}

} // namespace SNAIL_DEV_NS
