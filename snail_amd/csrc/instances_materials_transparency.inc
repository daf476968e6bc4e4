// instances_materials_transparency.inc -- transparent materials under full shading of an instanced scene
// (include/snail_instances_materials_transparency.h): the transparency continuation of Scene<DBVH>::RayTrace (src/scene_trace.cpp:468-483) and
// Scene::TraceTransparency (:620-634, instantiated for DBVH at :657-659).  Included once per arithmetic after instances_materials_bounce.inc and
// materials_transparency.inc, into the same namespace (dev / dev_sse); one wave per packet or per (packet, light), lane q = quad q, the
// reference's block of 4 quads = lanes 4b .. 4b + 3 (a DPP quad), wave-uniform control flow, as there.
//   k_imat_sample_transp / k_imat_sample_transp_rays   k_imat_sample / k_imat_sample_rays with the [T] additions of matSample (materials.inc): the kinds that
//                          can select a transparent lane, Sample::opacity per ray and the transSel selector after the opacity < 1 filter
//   k_imat_trace_level<DEEP>   DBVH::TraversePrimary<0, 1> of a level's generated packets, with barycentrics, under the generator's order list
//   k_imat_light_transp<DEEP>  a level's lights: one wave per (packet, light), DBVH::TraverseShadow, under the level's order list
// Unchanged, because they read nothing of the scene: k_mat_continue / k_mat_continue_rays, k_mat_blend_transp, k_mat_colour_transp,
// k_mat_truncated (materials_transparency.inc); for the primary level k_inst_frame, k_imat_light and k_mat_final.
// Kernels of their own: the existing sample, walk and light kernels stay the code they are, and a set they can be given never holds these kinds
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

// the sample stage with the [T] additions: matSample (materials.inc) with TRANSP on and the keys (slot, triId) of IMatKey
// (instances_materials.inc), behind the level's order list; the slots are hitInst's (primary level) or rInst's (a generic level)
__global__ __launch_bounds__(64) void k_imat_sample_transp(ITranspArgs B) { matSample<SRC_PRIMARY, true, IMatKey>(B.a, B.a.hitInst, B.inOrder, B.opacity, B.sel); }
__global__ __launch_bounds__(64) void k_imat_sample_transp_rays(ITranspArgs B) { matSample<SRC_MIRROR, true, IMatKey>(B.a, B.rInst, B.inOrder, B.opacity, B.sel); }

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
	if(p >= A.nPackets || orderSkipped(L.order, p)) return;
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

// ---- one (level packet, light): the nested call's shadow packet on the level's samples' normals, and DBVH::TraverseShadow: imatLight
// (instances_materials.inc) behind the level's order word, as k_mat_light_transp is matLight<DEEP, SRC_MIRROR> behind its order word
// (materials_transparency.inc) ----
template <bool DEEP>
__global__ __launch_bounds__(64) void k_imat_light_transp(ITranspArgs B) {
	__shared__ float lds[LDS_FLOATS_PER_WAVE];
	imatLight<DEEP, SRC_MIRROR>(B.a, B.inOrder, lds);
}

} // namespace SNAIL_DEV_NS
