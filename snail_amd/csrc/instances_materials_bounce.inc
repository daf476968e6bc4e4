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

// The sample stage on GENERIC packets of an instanced scene, RayGroup<0, hasMask> (the nested call of the bounce): matSample (materials.inc) with
// SRC_MIRROR's input side -- the directions read from the packet, a hit = t < inf AND the lane's mask bit, branch (a) shaded with the packet's own
// hasMask -- around the keys (slot, triId) of IMatKey (instances_materials.inc), the slots from rInst.
__global__ __launch_bounds__(64) void k_imat_sample_rays(IMatRaysArgs B) { matSample<SRC_MIRROR, false, IMatKey>(B.a, B.rInst, nullptr, nullptr, nullptr); }

// ---- one (mirrored packet, light): the nested call's shadow packet on the nested samples' normals, and DBVH::TraverseShadow: imatLight
// (instances_materials.inc) on the mirrored packets' samples, into the nested distance buffer ----
template <bool DEEP>
__global__ __launch_bounds__(64) void k_imat_light_rays(IMatArgs A) {
	__shared__ float lds[LDS_FLOATS_PER_WAVE];
	imatLight<DEEP, SRC_MIRROR>(A, nullptr, lds);
}

} // namespace SNAIL_DEV_NS
