// instances_materials_bounce.inc -- the one mirrored bounce of gVals[7] under full shading of an instanced scene
// (include/snail_instances_materials_bounce.h): Scene<DBVH>::RayTrace's call of Scene::TraceReflection (src/scene_trace.cpp:454-466, :603-618) on
// the samples of instances_materials.inc, i.e. the nested RayTrace<0, hasMask> of the mirrored packets -- rays that do not come from the camera and
// hit several instances.  Included once per arithmetic after instances_materials.inc, into the same namespace (dev / dev_sse).  Between
// k_imat_sample and k_imat_light:
//   k_mat_mirror             (materials.inc, unchanged: it reads the sample buffer, the primary distances and the camera alone)
//   k_inst_trace<false, true, DEEP, true>   DBVH::TraversePrimary<0, 1> of the mirrored packets, with barycentrics (instances.inc, unchanged)
//   k_imat_sample_rays       the sample stage on generic packets: RayGroup<0, hasMask>, hasMask = not all 256 lanes selected (:615-617), keys (slot, triId)
//   k_imat_light_rays<DEEP>  the nested lights: one wave per (mirrored packet, light), DBVH::TraverseShadow -> [light][packet][256]
//   k_mat_colour_rays        (materials.inc, unchanged) the nested outColor as FLOATS [packet][256][3]
// and k_mat_final_blend (materials.inc, unchanged) instead of k_mat_final.  Table look-ups in their fully checked form.
namespace SNAIL_DEV_NS {

struct IMatRaysArgs {
	IMatArgs a;            // FIRST: its hostTab opens the kernel-argument segment.  a.m.s.rDir / rMask (null = all lanes selected) / rDist / rObj (triIds),
	                       // a.m.rU / rV / rUVStride and a.m.nSamples as k_mat_sample_rays reads and writes them
	const int *rInst;      // instance slot of the generic packets' hits, indexed by list position
};

// The sample stage on GENERIC packets of an instanced scene, RayGroup<0, hasMask> (the nested call of the bounce): k_imat_sample with the
// directions read from the packet, a hit = t < inf AND the lane's mask bit, and branch (a) shaded with the packet's own hasMask.
// TWINS: the input side -- directions, mask, bary stride, the packet's hasMask and where it shows -- is k_mat_sample_rays' (materials.inc); the
// keys (slot, triId), their clamps, the (slot 0, triId 0) quirk and imatLoadTri are k_imat_sample's (instances_materials.inc); everything else --
// blocks, texDiff, the mip choice, the kinds, the output -- is k_mat_sample's.  A change to any of the three belongs here too.  A kernel of its
// own, not a template argument of k_imat_sample, for the reason k_mat_sample_rays gives.  imatSampleTransp
// (instances_materials_transparency.inc) repeats this kernel's input side: a change here belongs there too.
__global__ __launch_bounds__(64) void k_imat_sample_rays(IMatRaysArgs B) {
	const IMatArgs &A = B.a;
	const int lane = threadIdx.x & 63;
	const int li = (int)blockIdx.x;
	if(li >= A.m.s.nPackets) return;
	const PacketPos P = matPacket<SRC_MIRROR>(A.m, li);
	const size_t quad = P.pidx * 64 + lane;
	const float inf = __builtin_inff();
	float d[3][4];
	unsigned mask4 = 15u;
	loadQuad3(A.m.s.rDir, quad, d);
	if(A.m.s.rMask) mask4 = A.m.s.rMask[quad] & 15u;
	// hasMask is the PACKET's: RayGroup<0, 0> when all 256 lanes are selected, RayGroup<0, 1> otherwise (src/scene_trace.cpp:615-617)
	const bool pktMasked = __builtin_amdgcn_ballot_w64(mask4 != 15u) != 0;
	float bx[4], by[4];
	bool hit[4];
	int obj[4], slt[4];
	{
		const size_t uvq = quad * (size_t)A.m.rUVStride;
		const float4 tv = *(const float4 *)(A.m.s.rDist + quad * 4), uv = *(const float4 *)(A.m.rU + uvq), vv = *(const float4 *)(A.m.rV + uvq);
		const int4 iv = *(const int4 *)(A.m.s.rObj + quad * 4), sv = *(const int4 *)(B.rInst + quad * 4);
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
		const bool texd = m >= 0 && A.m.mats[m].kind == MAT_TEX;     // Material::fTexCoords
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

	float diff[3][4], spec[3][4];
#pragma unroll
	for(int l = 0; l < 4; l++) {
		// the lane's material: loaded values of an unrolled loop (compile-time indices), never a runtime-indexed array
		int kind = MAT_SIMPLE, ndotr = 1, tex = 0;
		float col[3] = {1.0f, 1.0f, 1.0f}, sp[3] = {0.0f, 0.0f, 0.0f};   // defaultMat = SimpleMaterial<true>(1, 1, 1), src/scene.cpp:6
		if(mid[l] >= 0) {
			const uint4 *r = (const uint4 *)(A.m.mats + mid[l]);
			const uint4 a = r[0], b = r[1], c = r[2];
			kind = (int)a.x; ndotr = (int)a.y;
			col[0] = asf(a.z); col[1] = asf(a.w); col[2] = asf(b.x);
			sp[0] = asf(b.y); sp[1] = asf(b.z); sp[2] = asf(b.w);
			tex = (int)c.x;
		}
		const float dn = d[0][l] * nrm[0][l] + d[1][l] * nrm[1][l] + d[2][l] * nrm[2][l];
		const float adn = __builtin_fabsf(dn);
		float t1[3] = {0.0f, 0.0f, 0.0f};
		// the kinds present among the wave's lanes: a branch per kind that needs code of its own, skipped when no lane has it
		if(__builtin_amdgcn_ballot_w64(kind == MAT_TEX && hit[l]) != 0) {
			if(kind == MAT_TEX && hit[l]) matSampleTex(A.m, tex, tc[0][l], tc[1][l], tdx, tdy, t1);
		}
#pragma unroll
		for(int c = 0; c < 3; c++) {
			float df, sf;
			if(kind == MAT_TEX) { df = ndotr ? t1[c] * dn : t1[c]; sf = df; }
			else if(kind == MAT_UBER) { df = col[c] * adn; sf = unmasked ? df : sp[c]; }
			else { df = ndotr ? col[c] * adn : col[c]; sf = df; }
			diff[c][l] = hit[l] ? df : 0.0f;
			spec[c][l] = hit[l] ? sf : 0.0f;
			nrm[c][l] = hit[l] ? nrm[c][l] : 0.0f;
		}
	}
	float4 *o = (float4 *)(A.m.nSamples + P.pidx * (9 * 256)) + lane;
#pragma unroll
	for(int c = 0; c < 3; c++) {
		o[(0 + c) * 64] = make_float4(nrm[c][0], nrm[c][1], nrm[c][2], nrm[c][3]);
		o[(3 + c) * 64] = make_float4(diff[c][0], diff[c][1], diff[c][2], diff[c][3]);
		o[(6 + c) * 64] = make_float4(spec[c][0], spec[c][1], spec[c][2], spec[c][3]);
	}
}

// ---- one (mirrored packet, light): the nested call's shadow packet on the nested samples' normals, and DBVH::TraverseShadow ----
// TWINS: the sample load (position = reflDir * t + reflOrig, hit = t < inf and the lane's mask bit) and the shadow-packet set-up are
// matLight<DEEP, SRC_MIRROR>'s (materials.inc), the walk and the stats flush are k_imat_light's (instances_materials.inc), i.e.
// k_inst_light<DEEP, SRC_MIRROR>'s (instances_shade.inc); a change to any of them belongs here too, and a change here in k_imat_light_transp
// (instances_materials_transparency.inc), which is this kernel behind a level's order word.
template <bool DEEP>
__global__ __launch_bounds__(64) void k_imat_light_rays(IMatArgs A) {
	__shared__ float lds[LDS_FLOATS_PER_WAVE];
	const int lane = threadIdx.x & 63;
	const int li = (int)blockIdx.x, n = (int)blockIdx.y;
	if(li >= A.m.s.nPackets || n >= A.m.s.nLights) return;
	const PacketPos P = matPacket<SRC_MIRROR>(A.m, li);
	const float lp[3] = {A.m.s.lights[n][0], A.m.s.lights[n][1], A.m.s.lights[n][2]};
	const float radius = A.m.s.lights[n][6], radSq = radius * radius;
	Quad Q;
	{
		Samples S;
		matLoadSamples<SRC_MIRROR>(A.m, P, lane, S);
		float tMin[3], tMax[3];
		hitBounds(S, tMin, tMax);
		if(lightCulled(tMin, tMax, lp, radSq)) return;   // (wave-uniform; k_mat_colour_rays skips the light by the same test)
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
