// instances_materials_heat_host.inc -- the C-ABI of include/snail_instances_materials_heatmap.h: per-packet TreeStats and the gVals[5] heat-map
// of instanced scenes under full shading; included by snail_hip.hip after instances_materials_tree_host.inc.  The instanced twin of
// materials_heat_host.inc: every form is levelsStore (materials_levels_host.inc) in its heat mode -- the tree of snail_instances_materials_tree.h with
// the PSTATS / _heat instantiations of its walking, light, generator and mirror stages, without the stages that only make colours, and the
// stores of heatmap.inc (dev_heat::k_heat_store, or dev_heat::k_heat_colours into dev::k_inst_store) after the last slice.  The arguments are
// judged by matHeatArgsOk (materials_heat_host.inc): the same rules, the same texts.
#include "../../include/snail_instances_materials_heatmap.h"

namespace {

// the _dev forms: the packet list (null: the frame's own grid) through levelsStore's heat mode; handle checked, nothing else held.  Every
// launch is booked through instancesBegin / instancesEnd under the handle's mu (IMatLevels), as a frame's is.
int imatHeatDev(SnailInstancesMaterials *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights,
				int flags, const float *tint, uint8_t *bgrPackets, uint32_t *dPacketStats, int maxDepth, uint64_t *dTrunc, uint64_t *dStats, hipStream_t st) {
	DeviceGuard guard(m->device);
	std::lock_guard<std::mutex> lock(m->inst->mu);
	if(!dXY) { if(int rc = m->frameLists.get(resx, resy, &dXY, &np)) return rc; }
	if(np > (1 << 24)) { snail_set_error("%s: more than 2^24 packets", fn); return 1; }
	return levelsStore<IMatLevels>(m, fn, cam, resx, resy, dXY, np, lights7, nLights, kMatHeatNoColour, flags, tint, bgrPackets, nullptr, maxDepth, dTrunc, dStats, st, true, dPacketStats);
}

} // namespace

extern "C" {

int snail_instances_materials_packet_stats_dev(SnailInstancesMaterials *m, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets,
											   const float *lights7, int nLights, int flags, int maxDepth, uint32_t *dPacketStats, uint64_t *dTruncated, uint64_t *dStats,
											   void *stream) {
	const char *fn = "snail_instances_materials_packet_stats_dev";
	if(int rc = matHeatArgsOk(fn, cam, resx, resy, lights7, nLights, flags, SNAIL_RENDER_REFLECTIONS, nullptr, maxDepth, dTruncated)) return rc;
	if(!dPacketStats || ((uintptr_t)dPacketStats & 3) || ((uintptr_t)dStats & 7) || ((uintptr_t)dTruncated & 7)) {
		snail_set_error("%s: d_packet_stats must be a 4-byte aligned device pointer (d_truncated: 8-byte aligned; d_stats: 8-byte aligned or null)", fn);
		return 1;
	}
	if(int rc = checkIMatAny(m, fn)) return rc;
	if(dPacketXY && nPackets <= 0) return 0;
	return imatHeatDev(m, fn, cam, resx, resy, dPacketXY, nPackets, lights7, nLights, flags, nullptr, nullptr, dPacketStats, maxDepth, dTruncated, dStats, (hipStream_t)stream);
}

int snail_instances_materials_heat_packets_dev(SnailInstancesMaterials *m, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets,
											   const float *lights7, int nLights, int flags, const float *tint, uint8_t *dBgr, uint32_t *dPacketStats, int maxDepth,
											   uint64_t *dTruncated, uint64_t *dStats, void *stream) {
	const char *fn = "snail_instances_materials_heat_packets_dev";
	if(int rc = matHeatArgsOk(fn, cam, resx, resy, lights7, nLights, flags, SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_AA4, tint, maxDepth, dTruncated)) return rc;
	if(!dBgr || ((uintptr_t)dBgr & 3) || ((uintptr_t)dPacketStats & 3) || ((uintptr_t)dStats & 7) || ((uintptr_t)dTruncated & 7)) {
		snail_set_error("%s: d_bgr_packets must be a 4-byte aligned device pointer (d_packet_stats: 4-byte aligned or null; d_truncated: 8-byte aligned; d_stats: 8-byte aligned or null)", fn);
		return 1;
	}
	if(int rc = checkIMatAny(m, fn)) return rc;
	if(dPacketXY && nPackets <= 0) return 0;
	return imatHeatDev(m, fn, cam, resx, resy, dPacketXY, nPackets, lights7, nLights, flags, tint, dBgr, dPacketStats, maxDepth, dTruncated, dStats, (hipStream_t)stream);
}

int snail_instances_materials_render_heat_tiles(SnailInstancesMaterials *m, const float cam[13], int resx, int resy, const int32_t *coords, const int64_t *offsets,
												int nTiles, const float *lights7, int nLights, int flags, const float *tint, uint8_t *data, int maxDepth, uint64_t *truncated,
												uint64_t stats[4]) {
	const char *fn = "snail_instances_materials_render_heat_tiles";
	if(int rc = matHeatArgsOk(fn, cam, resx, resy, lights7, nLights, flags, SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_AA4, tint, maxDepth, truncated)) return rc;
	if(nTiles > 0 && (!coords || !offsets || !data)) { snail_set_error("%s: null buffer", fn); return 1; }
	if(int rc = tileRectsOk(fn, coords, nTiles)) return rc;
	if(int rc = checkIMatAny(m, fn)) return rc;
	if(nTiles <= 0) return 0;
	return renderTilesHost<IMatLevels>(m, fn, cam, resx, resy, coords, offsets, nTiles, lights7, nLights, kMatHeatNoColour, flags, tint, data, maxDepth, truncated, stats, true, levelsStore<IMatLevels>);
}

int snail_instances_materials_render_heat_frame(SnailInstancesMaterials *m, const float cam[13], int resx, int resy, const float *lights7, int nLights, int flags,
												uint8_t *image, int pitch, int maxDepth, uint64_t *truncated, uint64_t stats[4]) {
	const char *fn = "snail_instances_materials_render_heat_frame";
	if(int rc = matHeatArgsOk(fn, cam, resx, resy, lights7, nLights, flags, SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_AA4, nullptr, maxDepth, truncated)) return rc;
	if(!image || pitch < resx * 3) { snail_set_error("%s: null image or a pitch below 3 * resx", fn); return 1; }
	if(int rc = checkIMatAny(m, fn)) return rc;
	return renderFrameHost<IMatLevels>(m, fn, cam, resx, resy, lights7, nLights, kMatHeatNoColour, flags, image, pitch, maxDepth, truncated, stats, true, levelsStore<IMatLevels>);
}

} // extern "C"
