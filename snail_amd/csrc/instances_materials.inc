// instances_materials.inc -- full shading of the primary packets of an instanced scene (include/snail_instances_materials.h): the gVals[6] &&
// HasShadingData() branch of Scene<DBVH>::RayTrace (src/scene_trace.cpp:145-358) with DBVH::HasShadingData() answering 1 -- this project's
// completion of the reference's TODO (src/dbvh/tree.h:207-209); everything else as the reference writes it -- and, on its samples, the lights of
// instances_shade.inc.  Included once per arithmetic after materials.inc, into the same namespace (dev / dev_sse).  Always over an explicit packet
// list, one wave per packet or per (packet, light), lane q = quad q, the reference's block of 4 quads = lanes 4b .. 4b + 3:
//   k_imat_sample          hit records (t, u, v, instance slot, triId) + per-BLAS ShTriangle records and material maps + the instance records'
//                          rotations + ONE scene-wide material and texture list -> 9 floats per ray, the sample buffer of k_mat_sample
//   k_imat_light<DEEP>     one wave per (packet, light): position + the sample's (interpolated, rotated) normal -> light cull -> shadow packet ->
//                          DBVH::TraverseShadow -> the surviving distances [light][packet][256]      Scene::TraceLight, src/scene_trace.cpp:523-566
//   k_mat_final            (materials.inc, unchanged: it reads samples, hits and the surviving distances alone)
// DBVH::GetSElement(slot, triId) (src/dbvh/tree.h:211-215) = the BLAS's record through ShTriangle::Transform (src/triangle.h:206-219);
// DBVH::GetMaterialId(idx, slot) (:246-248) = the BLAS's own map entry, an index into the ONE scene-wide list.  Every equality of :171-356 is on
// the pair (object, element) = (slot, triId), as the reference compares wherever isctFlags & fElement is set (:162, :179-182, :252-253, :263).
// Table look-ups in their fully checked form.
namespace SNAIL_DEV_NS {

struct IMatBlas {          // 24 bytes: the shading data of one BLAS
	const uint4 *shtris;   // ShTriangle records, 4 x uint4 each, that BLAS's triId order
	const int *matMap;
	int nTris, nMap;
};
struct IMatArgs {
	MatArgs m;             // FIRST: its hostTab opens the kernel-argument segment.  s.hitT / s.hitId (triIds) / hitU / hitV = the primary hits; shtris / matMap unused
	InstArgs i;            // top, inst, blas: the tree the shadow walks and the records' rotations read
	const int *hitInst;    // instance slot of the primary hits, packet-major
	const IMatBlas *tab;   // [nBlas]
	int nBlas, nSlots;     // nSlots: the instance records the handle's buffer has room for (a slot is clamped below it)
};

// DBVH::GetSElement(slot, triId) and DBVH::GetMaterialId(shTri.MatId(), slot): the instance record as instLoadSamples reads it (per lane), the
// BLAS's record, ShTriangle::Transform -- nrm[1], nrm[2] made absolute, the three vectors through Rot (x * r.x + y * r.y + z * r.z, added left to
// right), made differences again with the ROTATED nrm[0]; uv and matId untouched, nothing renormalised, the translation unused.  The round trip
// is not exact in fp32, so the identity rotation goes through it as every other.  (The set's creation has checked every record and entry; the
// clamps here only keep a corrupted hit record or table from turning into an address.)
__device__ __forceinline__ ShTri imatLoadTri(const IMatArgs &A, int slot, int tri, int &mat) {
	const uint4 *rec = A.i.inst + (size_t)slot * 4;
	const uint4 q0 = rec[0], q1 = rec[1], q2 = rec[2];
	int b = (int)q0.w;
	b = b < 0 ? 0 : b;
	b = b < A.nBlas ? b : A.nBlas - 1;
	const IMatBlas B = A.tab[b];
	const int idx = tri < B.nTris ? tri : B.nTris - 1;
	const uint4 *r = B.shtris + (size_t)idx * 4;
	const uint4 a = r[0], bb = r[1], c = r[2], e = r[3];
	ShTri T;
	T.uv[0][0] = asf(a.x); T.uv[0][1] = asf(a.y); T.uv[1][0] = asf(a.z); T.uv[1][1] = asf(a.w);
	T.uv[2][0] = asf(bb.x); T.uv[2][1] = asf(bb.y);
	T.matId = (int)e.w;
	const float n0[3] = {asf(bb.z), asf(bb.w), asf(c.x)};
	const float n1[3] = {asf(c.y) + n0[0], asf(c.z) + n0[1], asf(c.w) + n0[2]};
	const float n2[3] = {asf(e.x) + n0[0], asf(e.y) + n0[1], asf(e.z) + n0[2]};
	const float R[3][3] = {{asf(q0.x), asf(q0.y), asf(q0.z)}, {asf(q1.x), asf(q1.y), asf(q1.z)}, {asf(q2.x), asf(q2.y), asf(q2.z)}};
#pragma unroll
	for(int k = 0; k < 3; k++) {
		T.nrm[0][k] = n0[0] * R[k][0] + n0[1] * R[k][1] + n0[2] * R[k][2];
		T.nrm[1][k] = n1[0] * R[k][0] + n1[1] * R[k][1] + n1[2] * R[k][2];
		T.nrm[2][k] = n2[0] * R[k][0] + n2[1] * R[k][1] + n2[2] * R[k][2];
	}
#pragma unroll
	for(int k = 0; k < 3; k++) { T.nrm[1][k] = T.nrm[1][k] - T.nrm[0][k]; T.nrm[2][k] = T.nrm[2][k] - T.nrm[0][k]; }
	const int mi = T.matId & 0x7fffffff;
	mat = -1;
	if(mi < B.nMap) {
		const int m = B.matMap[mi];
		mat = (unsigned)m < (unsigned)A.m.nMats ? m : -1;
	}
	return T;
}

// TWINS: this kernel is k_mat_sample (materials.inc) for an instanced scene: a block's key is the pair (slot, triId) and a record comes through
// imatLoadTri; everything else -- blocks, the (slot 0, triId 0) quirk, texDiff, the mip choice, the kinds, the output -- is k_mat_sample's; a
// change there belongs here too.  A second kernel, not a template argument of k_mat_sample, for the reason k_mat_sample_rays gives.
// k_imat_sample_rays (instances_materials_bounce.inc) is this kernel for generic packets (k_mat_sample_rays' input side): a change to the keys,
// their clamps, the quirk or imatLoadTri belongs there too -- and in imatSampleTransp (instances_materials_transparency.inc), which is both
// kernels with the transparent kinds, Sample::opacity and the selector.
__global__ __launch_bounds__(64) void k_imat_sample(IMatArgs A) {
	const int lane = threadIdx.x & 63;
	const int li = (int)blockIdx.x;
	if(li >= A.m.s.nPackets) return;
	const PacketPos P = packetOf(A.m.s, li);
	const size_t quad = P.pidx * 64 + lane;
	const float inf = __builtin_inff();
	float d[3][4];
	matRays(A.m.s, P, lane, d);
	float bx[4], by[4];
	bool hit[4];
	int obj[4], slt[4];
	{
		const float4 tv = *(const float4 *)(A.m.s.hitT + quad * 4), uv = *(const float4 *)(A.m.hitU + quad * 4), vv = *(const float4 *)(A.m.hitV + quad * 4);
		const int4 iv = *(const int4 *)(A.m.s.hitId + quad * 4), sv = *(const int4 *)(A.hitInst + quad * 4);
		const float t[4] = {tv.x, tv.y, tv.z, tv.w};
		const int id[4] = {iv.x, iv.y, iv.z, iv.w};
		const int sl[4] = {sv.x, sv.y, sv.z, sv.w};
		bx[0] = uv.x; bx[1] = uv.y; bx[2] = uv.z; bx[3] = uv.w;
		by[0] = vv.x; by[1] = vv.y; by[2] = vv.z; by[3] = vv.w;
#pragma unroll
		for(int l = 0; l < 4; l++) {
			hit[l] = t[l] < inf;
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
		// lane 0 missed: a lane that hit slot 0's triangle 0 beside it keeps the default material and zero normal / texCoord).  A record is loaded
		// and transformed only on lanes that hit.
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
	const int mid0b = blockFirst(mid[0]);
	const bool unmasked = blockAll(mid[0] == mid0b && mid[1] == mid0b && mid[2] == mid0b && mid[3] == mid0b, lane) && full;

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
	float4 *o = (float4 *)(A.m.samples + P.pidx * (9 * 256)) + lane;
#pragma unroll
	for(int c = 0; c < 3; c++) {
		o[(0 + c) * 64] = make_float4(nrm[c][0], nrm[c][1], nrm[c][2], nrm[c][3]);
		o[(3 + c) * 64] = make_float4(diff[c][0], diff[c][1], diff[c][2], diff[c][3]);
		o[(6 + c) * 64] = make_float4(spec[c][0], spec[c][1], spec[c][2], spec[c][3]);
	}
}

// ---- one (packet, light): the shadow packet (src/scene_trace.cpp:538-558) on the sample buffer's normals, and DBVH::TraverseShadow ----
// TWINS: the sample load and the shadow-packet set-up are matLight<DEEP, SRC_PRIMARY>'s (materials.inc), the walk and the stats flush are
// k_inst_light<DEEP, SRC_PRIMARY>'s (instances_shade.inc); a change to either belongs here too, and a change here in k_imat_light_rays
// (instances_materials_bounce.inc), which is this kernel on the mirrored packets' samples.
template <bool DEEP>
__global__ __launch_bounds__(64) void k_imat_light(IMatArgs A) {
	__shared__ float lds[LDS_FLOATS_PER_WAVE];
	const int lane = threadIdx.x & 63;
	const int li = (int)blockIdx.x, n = (int)blockIdx.y;
	if(li >= A.m.s.nPackets || n >= A.m.s.nLights) return;
	const PacketPos P = packetOf(A.m.s, li);
	const float lp[3] = {A.m.s.lights[n][0], A.m.s.lights[n][1], A.m.s.lights[n][2]};
	const float radius = A.m.s.lights[n][6], radSq = radius * radius;
	Quad Q;
	{
		Samples S;
		matLoadSamples<SRC_PRIMARY>(A.m, P, lane, S);
		float tMin[3], tMax[3];
		hitBounds(S, tMin, tMax);
		if(lightCulled(tMin, tMax, lp, radSq)) return;   // (wave-uniform; k_mat_final skips the light by the same test)
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
	*(float4 *)(A.m.s.sDist + ((size_t)n * (size_t)A.m.s.nPackets + P.pidx) * 256 + (size_t)lane * 4) = make_float4(Q.dist[0], Q.dist[1], Q.dist[2], Q.dist[3]);
}

} // namespace SNAIL_DEV_NS
