// materials_heat_host.inc -- the C-ABI of include/snail_materials_heatmap.h: per-packet TreeStats and the gVals[5] heat-map under full shading;
// included by snail_hip.hip after materials_tree_host.inc.  Every form is levelsStore (materials_levels_host.inc) in its heat mode: the tree of snail_materials_tree.h with
// the PSTATS / _heat instantiations of its walking, light, generator and mirror stages, without the stages that only make colours, and the
// stores of heatmap.inc (dev_heat::k_heat_store, or dev_heat::k_heat_colours into dev::k_inst_store) after the last slice.
#include "../../include/snail_materials_heatmap.h"

namespace {

// everything that can be judged without the handle; the flags first.  `allowed` = the flag bits of the entry point
int matHeatArgsOk(const char *fn, const float *cam, int resx, int resy, const float *lights7, int nLights, int flags, int allowed, const float *tint, int maxDepth,
				  const uint64_t *trunc) {
	if(flags & SNAIL_RENDER_DEPTH) {
		snail_set_error("%s: SNAIL_RENDER_DEPTH in flags has no heat-map (gVals[1] returns from RayTrace before the counters' colour): use the depth entry points", fn);
		return 1;
	}
	if(flags & ~allowed) { snail_set_error("%s: unknown or unsupported bits in flags 0x%x (allowed: 0x%x)", fn, flags & ~allowed, allowed); return 1; }
	if(maxDepth < 1 || maxDepth > SNAIL_MAT_TRANSP_MAX_DEPTH) { snail_set_error("%s: maxDepth %d outside 1..%d", fn, maxDepth, SNAIL_MAT_TRANSP_MAX_DEPTH); return 1; }
	if(!trunc) { snail_set_error("%s: null truncated-lane counter", fn); return 1; }
	if(!cam || resx <= 0 || resy <= 0 || resx > (1 << 20) || resy > (1 << 20)) { snail_set_error("%s: bad camera or resolution", fn); return 1; }
	if(nLights < 0 || nLights > SNAIL_MAX_LIGHTS || (nLights && !lights7)) { snail_set_error("%s: 0..%d lights (got %d) with a non-null lights7", fn, SNAIL_MAX_LIGHTS, nLights); return 1; }
	if(tint && !(std::isfinite(tint[0]) && std::isfinite(tint[1]) && std::isfinite(tint[2]))) { snail_set_error("%s: the tint is not finite", fn); return 1; }
	return 0;
}

// the colour of the material reaches no counter: any ambient will do for the record the stages share
const float kMatHeatNoColour[3] = {0.0f, 0.0f, 0.0f};

// the _dev forms: the packet list (null: the frame's own grid) through levelsStore's heat mode; handle checked, nothing else held
int matHeatDev(SnailMaterials *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights, int flags,
			   const float *tint, uint8_t *bgrPackets, uint32_t *dPacketStats, int maxDepth, uint64_t *dTrunc, uint64_t *dStats, hipStream_t st) {
	DeviceGuard guard(m->device);
	SNAIL_LOCK(m->scene);
	if(!dXY) { if(int rc = m->frameLists.get(resx, resy, &dXY, &np)) return rc; }
	if(np > (1 << 24)) { snail_set_error("%s: more than 2^24 packets", fn); return 1; }
	return levelsStore<MatLevels>(m, fn, cam, resx, resy, dXY, np, lights7, nLights, kMatHeatNoColour, flags, tint, bgrPackets, nullptr, maxDepth, dTrunc, dStats, st, true, dPacketStats);
}

} // namespace

extern "C" {

int snail_materials_packet_stats_dev(SnailMaterials *m, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets, const float *lights7, int nLights,
									 int flags, int maxDepth, uint32_t *dPacketStats, uint64_t *dTruncated, uint64_t *dStats, void *stream) {
	const char *fn = "snail_materials_packet_stats_dev";
	if(int rc = matHeatArgsOk(fn, cam, resx, resy, lights7, nLights, flags, SNAIL_RENDER_REFLECTIONS, nullptr, maxDepth, dTruncated)) return rc;
	if(!dPacketStats || ((uintptr_t)dPacketStats & 3) || ((uintptr_t)dStats & 7) || ((uintptr_t)dTruncated & 7)) {
		snail_set_error("%s: d_packet_stats must be a 4-byte aligned device pointer (d_truncated: 8-byte aligned; d_stats: 8-byte aligned or null)", fn);
		return 1;
	}
	if(int rc = checkMaterialsAny(m, fn)) return rc;
	if(dPacketXY && nPackets <= 0) return 0;
	return matHeatDev(m, fn, cam, resx, resy, dPacketXY, nPackets, lights7, nLights, flags, nullptr, nullptr, dPacketStats, maxDepth, dTruncated, dStats, (hipStream_t)stream);
}

int snail_materials_heat_packets_dev(SnailMaterials *m, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets, const float *lights7, int nLights,
									 int flags, const float *tint, uint8_t *dBgr, uint32_t *dPacketStats, int maxDepth, uint64_t *dTruncated, uint64_t *dStats, void *stream) {
	const char *fn = "snail_materials_heat_packets_dev";
	if(int rc = matHeatArgsOk(fn, cam, resx, resy, lights7, nLights, flags, SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_AA4, tint, maxDepth, dTruncated)) return rc;
	if(!dBgr || ((uintptr_t)dBgr & 3) || ((uintptr_t)dPacketStats & 3) || ((uintptr_t)dStats & 7) || ((uintptr_t)dTruncated & 7)) {
		snail_set_error("%s: d_bgr_packets must be a 4-byte aligned device pointer (d_packet_stats: 4-byte aligned or null; d_truncated: 8-byte aligned; d_stats: 8-byte aligned or null)", fn);
		return 1;
	}
	if(int rc = checkMaterialsAny(m, fn)) return rc;
	if(dPacketXY && nPackets <= 0) return 0;
	return matHeatDev(m, fn, cam, resx, resy, dPacketXY, nPackets, lights7, nLights, flags, tint, dBgr, dPacketStats, maxDepth, dTruncated, dStats, (hipStream_t)stream);
}

int snail_materials_render_heat_tiles(SnailMaterials *m, const float cam[13], int resx, int resy, const int32_t *coords, const int64_t *offsets, int nTiles, const float *lights7,
									  int nLights, int flags, const float *tint, uint8_t *data, int maxDepth, uint64_t *truncated, uint64_t stats[4]) {
	const char *fn = "snail_materials_render_heat_tiles";
	if(int rc = matHeatArgsOk(fn, cam, resx, resy, lights7, nLights, flags, SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_AA4, tint, maxDepth, truncated)) return rc;
	if(nTiles > 0 && (!coords || !offsets || !data)) { snail_set_error("%s: null buffer", fn); return 1; }
	if(int rc = tileRectsOk(fn, coords, nTiles)) return rc;
	if(int rc = checkMaterialsAny(m, fn)) return rc;
	if(nTiles <= 0) return 0;
	return renderTilesHost<MatLevels>(m, fn, cam, resx, resy, coords, offsets, nTiles, lights7, nLights, kMatHeatNoColour, flags, tint, data, maxDepth, truncated, stats, true, levelsStore<MatLevels>);
}

int snail_materials_render_heat_frame(SnailMaterials *m, const float cam[13], int resx, int resy, const float *lights7, int nLights, int flags, uint8_t *image, int pitch,
									  int maxDepth, uint64_t *truncated, uint64_t stats[4]) {
	const char *fn = "snail_materials_render_heat_frame";
	if(int rc = matHeatArgsOk(fn, cam, resx, resy, lights7, nLights, flags, SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_AA4, nullptr, maxDepth, truncated)) return rc;
	if(!image || pitch < resx * 3) { snail_set_error("%s: null image or a pitch below 3 * resx", fn); return 1; }
	if(int rc = checkMaterialsAny(m, fn)) return rc;
	return renderFrameHost<MatLevels>(m, fn, cam, resx, resy, lights7, nLights, kMatHeatNoColour, flags, image, pitch, maxDepth, truncated, stats, true, levelsStore<MatLevels>);
}

} // extern "C"
