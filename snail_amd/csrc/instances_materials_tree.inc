// instances_materials_tree.inc -- the transparency continuation together with the one mirrored bounce of gVals[7] under full shading of an
// instanced scene (include/snail_instances_materials_tree.h).  Included once per arithmetic after materials_tree.inc, into the same namespace
// (dev / dev_sse).  Every stage of the triangle of calls exists and runs unchanged on the levels of both chains: k_inst_frame, k_imat_sample_transp /
// _rays, k_imat_trace_level<DEEP> (a null order list walks every packet: B_{0,0}), k_imat_light_transp<DEEP>, k_imat_light<DEEP>
// (instances*.inc) and the scene-free k_mat_continue / _rays, k_mat_mirror / _rays, k_mat_blend_transp, k_mat_blend_refl / _rays, k_mat_colour /
// _transp, k_mat_truncated, k_mat_final, k_inst_aa_packets, k_inst_store.  Every stage the B chain runs behind an order list already takes one,
// so no wrapper kernel is needed.  Here, for snail_instances_materials_mirror_rays_dev on its own alone:
//   k_imat_clear_hits      zeros in the element and barycentric buffers of the packets that are part of the level -- the walk leaves both as it
//                          found them on a lane without a hit -- behind the level's order list: a packet that is not part keeps what it held
// (the frames clear whole levels with ONE hipMemsetAsync, as imatNested does).  Plain stores, no arithmetic: once for both arithmetics.
namespace SNAIL_DEV_NS {

#if !SNAIL_ARITH_SSE
__global__ __launch_bounds__(64) void k_imat_clear_hits(int *element, float *bary, const int *order, int nPackets) {
	const int lane = threadIdx.x & 63;
	const int li = (int)blockIdx.x;
	if(li >= nPackets || orderSkipped(order, li)) return;
	const size_t quad = (size_t)li * 64 + lane;
	*(int4 *)(element + quad * 4) = make_int4(0, 0, 0, 0);
	*(float4 *)(bary + quad * 8) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	*(float4 *)(bary + quad * 8 + 4) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}
#endif

} // namespace SNAIL_DEV_NS
