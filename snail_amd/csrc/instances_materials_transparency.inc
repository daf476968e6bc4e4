// instances_materials_transparency.inc -- transparent materials under full shading of an instanced scene
// (include/snail_instances_materials_transparency.h): the transparency continuation of Scene<DBVH>::RayTrace (src/scene_trace.cpp:468-483) and
// Scene::TraceTransparency (:620-634, instantiated for DBVH at :657-659).  Included once per arithmetic after instances_materials_bounce.inc and
// materials_transparency.inc, into the same namespace (dev / dev_sse); one wave per packet or per (packet, light), lane q = quad q, the
// reference's block of 4 quads = lanes 4b .. 4b + 3 (a DPP quad), wave-uniform control flow, as there.
//   k_imat_sample_transp / k_imat_sample_transp_rays   k_imat_sample / k_imat_sample_rays with the [T] additions of matSample (materials.inc): the kinds that
//                          can select a transparent lane, Sample::opacity per ray and the transSel selector after the opacity < 1 filter
//   k_imat_trace_level<DEEP>   DBVH::TraversePrimary<0, 1> of a level's generated packets, with barycentrics, under the generator's order list
//   k_imat_light_transp<DEEP>  a level's lights: one wave per (packet, light), DBVH::TraverseShadow, under the level's order list
//   k_imat_trace_level_heat<DEEP> / k_imat_light_transp_heat<DEEP>   the same two, booking their counters per packet as well (the heat-map launches)
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
// PSTATS (k_imat_trace_level_heat, the heat-map launches of include/snail_instances_materials_heatmap.h): the walk's counters per packet as well, at
// the packet's list position in InstArgs::pstats, as k_inst_trace<.., PSTATS> books them -- decided at compile time, for the reason above.  The body
// is instances_materials_trace_level_body.inc, included once per kernel.
template <bool DEEP>
__global__ __launch_bounds__(64) void k_imat_trace_level(ILevelArgs L) {
#define SNAIL_TRACE_LEVEL_PSTATS 0
#include "instances_materials_trace_level_body.inc"
#undef SNAIL_TRACE_LEVEL_PSTATS
}
template <bool DEEP>
__global__ __launch_bounds__(64) void k_imat_trace_level_heat(ILevelArgs L) {
#define SNAIL_TRACE_LEVEL_PSTATS 1
#include "instances_materials_trace_level_body.inc"
#undef SNAIL_TRACE_LEVEL_PSTATS
}

// ---- one (level packet, light): the nested call's shadow packet on the level's samples' normals, and DBVH::TraverseShadow: imatLight
// (instances_materials.inc) behind the level's order word, as k_mat_light_transp is matLight<DEEP, SRC_MIRROR> behind its order word
// (materials_transparency.inc) ----
template <bool DEEP>
__global__ __launch_bounds__(64) void k_imat_light_transp(ITranspArgs B) {
	__shared__ float lds[LDS_FLOATS_PER_WAVE];
	imatLight<DEEP, SRC_MIRROR>(B.a, B.inOrder, lds);
}
static_assert(offsetof(ITranspArgs, a) == 0, "imatLight's late booking reads ShadeArgs::pstats at offset 0 of this kernel's argument record too");
template <bool DEEP>
__global__ __launch_bounds__(64) void k_imat_light_transp_heat(ITranspArgs B) {
	__shared__ float lds[LDS_FLOATS_PER_WAVE];
	imatLight<DEEP, SRC_MIRROR, true>(B.a, B.inOrder, lds);
}

} // namespace SNAIL_DEV_NS
