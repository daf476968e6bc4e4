// instances_materials.inc -- full shading of the primary packets of an instanced scene (include/snail_instances_materials.h): the gVals[6] &&
// HasShadingData() branch of Scene<DBVH>::RayTrace (src/scene_trace.cpp:145-358) with DBVH::HasShadingData() answering 1 -- this project's
// completion of the reference's TODO (src/dbvh/tree.h:207-209); everything else as the reference writes it -- and, on its samples, the lights of
// instances_shade.inc.  Included once per arithmetic after materials.inc, into the same namespace (dev / dev_sse).  Always over an explicit packet
// list, one wave per packet or per (packet, light), lane q = quad q, the reference's block of 4 quads = lanes 4b .. 4b + 3:
//   k_imat_sample          hit records (t, u, v, instance slot, triId) + per-BLAS ShTriangle records and material maps + the instance records'
//                          rotations + ONE scene-wide material and texture list -> 9 floats per ray, the sample buffer of k_mat_sample
//   k_imat_light<DEEP>     one wave per (packet, light): position + the sample's (interpolated, rotated) normal -> light cull -> shadow packet ->
//                          DBVH::TraverseShadow -> the surviving distances [light][packet][256]      Scene::TraceLight, src/scene_trace.cpp:523-566
//   k_imat_light_heat<DEEP>   the same, booking its counters per packet as well (the heat-map launches, include/snail_instances_materials_heatmap.h)
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

// The key of an instanced scene's hit for matSample (materials.inc): the pair (slot, triId).  The slot comes from `inst` (hitInst of the primary
// hits, or the generic packets' slot buffer, indexed by list position) and is clamped to nSlots; the triId's upper bound is the BLAS's, in
// imatLoadTri, through which the record and its material come.
struct IMatKey {
	typedef IMatArgs Args;
	enum { SLOTS = 1 };
	static __device__ __forceinline__ const MatArgs &mat(const IMatArgs &A) { return A.m; }
	static __device__ __forceinline__ void slots(const IMatArgs &A, const int *inst, size_t quad, int (&s)[4]) {
		const int4 sv = *(const int4 *)(inst + quad * 4);
		const int sl[4] = {sv.x, sv.y, sv.z, sv.w};
#pragma unroll
		for(int l = 0; l < 4; l++) {
			s[l] = sl[l] < 0 ? 0 : sl[l];
			s[l] = s[l] < A.nSlots ? s[l] : A.nSlots - 1;
		}
	}
	static __device__ __forceinline__ int tri(const IMatArgs &, int id) { return id < 0 ? 0 : id; }
	static __device__ __forceinline__ ShTri load(const IMatArgs &A, int slot, int tri, int &mat) { return imatLoadTri(A, slot, tri, mat); }
};
__global__ __launch_bounds__(64) void k_imat_sample(IMatArgs A) { matSample<SRC_PRIMARY, false, IMatKey>(A, A.hitInst, nullptr, nullptr, nullptr); }

// ---- one (packet, light): the shadow packet (src/scene_trace.cpp:538-558) on the sample buffer's normals, and DBVH::TraverseShadow ----
// ONE body for k_imat_light (SRC_PRIMARY), k_imat_light_rays (instances_materials_bounce.inc; SRC_MIRROR: the mirrored packets' samples --
// position = reflDir * t + reflOrig, hit = t < inf and the lane's mask bit -- and the nested distance buffer) and k_imat_light_transp
// (instances_materials_transparency.inc; SRC_MIRROR behind a level's order list; `order` null: every packet).
// TWINS: the sample load and the shadow-packet set-up are matLight<DEEP, SRC>'s (materials.inc), the walk and the stats flush are
// k_inst_light<DEEP, SRC>'s (instances_shade.inc); a change to either belongs here too.
// PSTATS: the heat-map launches' instantiation (include/snail_instances_materials_heatmap.h), which also books the (packet, light)'s counters per
// packet at P.pidx -- a template argument as in matLight and k_inst_light, so that the other launches' kernels stay the code they were.  The array's
// address is read late, from the kernel-argument segment (bookPacketLate): ShadeArgs opens MatArgs, which opens IMatArgs, which opens ITranspArgs,
// so ShadeArgs::pstats is at the same offset of the segment in k_imat_light_heat and in k_imat_light_transp_heat.  A culled pair has returned
// before the booking: it books nothing.
static_assert(offsetof(IMatArgs, m) == 0 && offsetof(MatArgs, s) == 0, "bookPacketLate<ShadeArgs> reads pstats at the record's offset in the kernel-argument segment");
template <bool DEEP, int SRC, bool PSTATS = false>
__device__ __forceinline__ void imatLight(const IMatArgs &A, const int *order, float *lds) {
	const int lane = threadIdx.x & 63;
	const int li = (int)blockIdx.x, n = (int)blockIdx.y;
	if(li >= A.m.s.nPackets || n >= A.m.s.nLights || orderSkipped(order, li)) return;
	const PacketPos P = matPacket<SRC>(A.m, li);
	const float lp[3] = {A.m.s.lights[n][0], A.m.s.lights[n][1], A.m.s.lights[n][2]};
	const float radius = A.m.s.lights[n][6], radSq = radius * radius;
	Quad Q;
	{
		Samples S;
		matLoadSamples<SRC>(A.m, P, lane, S);
		float tMin[3], tMax[3];
		hitBounds(S, tMin, tMax);
		if(lightCulled(tMin, tMax, lp, radSq)) return;   // (wave-uniform; the colour stage -- k_mat_final, k_mat_colour_rays, k_mat_colour_transp -- skips the light by the same test)
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
	if(PSTATS) bookPacketLate<ShadeArgs>(P.pidx, st, rays, lane);
	*(float4 *)((SRC == SRC_MIRROR ? A.m.nSDist : A.m.s.sDist) + ((size_t)n * (size_t)A.m.s.nPackets + P.pidx) * 256 + (size_t)lane * 4) = make_float4(Q.dist[0], Q.dist[1], Q.dist[2], Q.dist[3]);
}
template <bool DEEP>
__global__ __launch_bounds__(64) void k_imat_light(IMatArgs A) {
	__shared__ float lds[LDS_FLOATS_PER_WAVE];
	imatLight<DEEP, SRC_PRIMARY>(A, nullptr, lds);
}
template <bool DEEP>
__global__ __launch_bounds__(64) void k_imat_light_heat(IMatArgs A) {
	__shared__ float lds[LDS_FLOATS_PER_WAVE];
	imatLight<DEEP, SRC_PRIMARY, true>(A, nullptr, lds);
}

} // namespace SNAIL_DEV_NS
