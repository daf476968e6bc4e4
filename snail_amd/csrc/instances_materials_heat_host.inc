// instances_materials_heat_host.inc -- the C-ABI of include/snail_instances_materials_heatmap.h: per-packet TreeStats and the gVals[5] heat-map
// of instanced scenes under full shading; included by snail_hip.hip after instances_materials_tree_host.inc.  The instanced twin of
// materials_heat_host.inc, function for function: every form is imatTreeStore in its heat mode -- the tree of snail_instances_materials_tree.h with
// the PSTATS / _heat instantiations of its walking, light, generator and mirror stages, without the stages that only make colours, and the
// stores of heatmap.inc (dev_heat::k_heat_store, or dev_heat::k_heat_colours into dev::k_inst_store) after the last slice.  The arguments are
// judged by matHeatArgsOk (materials_heat_host.inc): the same rules, the same texts.
#include "../../include/snail_instances_materials_heatmap.h"

namespace {

// the _dev forms: the packet list (null: the frame's own grid) through imatTreeStore's heat mode; handle checked, nothing else held.  Every
// launch is booked through instancesBegin / instancesEnd under the handle's mu (imatShadeTree), as a frame's is.
int imatHeatDev(SnailInstancesMaterials *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights,
				int flags, const float *tint, uint8_t *bgrPackets, uint32_t *dPacketStats, int maxDepth, uint64_t *dTrunc, uint64_t *dStats, hipStream_t st) {
	DeviceGuard guard(m->device);
	std::lock_guard<std::mutex> lock(m->inst->mu);
	if(!dXY) { if(int rc = imatFrameList(m, resx, resy, &dXY, &np)) return rc; }
	if(np > (1 << 24)) { snail_set_error("%s: more than 2^24 packets", fn); return 1; }
	return imatTreeStore(m, fn, cam, resx, resy, dXY, np, lights7, nLights, kMatHeatNoColour, flags, tint, bgrPackets, nullptr, maxDepth, dTrunc, dStats, st, true, dPacketStats);
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
	for(int k = 0; k < nTiles; k++) {
		const long long x = coords[(size_t)k * 4 + 0], y = coords[(size_t)k * 4 + 1], w = coords[(size_t)k * 4 + 2], hh = coords[(size_t)k * 4 + 3];
		if(w <= 0 || hh <= 0 || x < 0 || y < 0 || x + w > (1 << 24) || y + hh > (1 << 24)) {
			snail_set_error("%s: tile %d: bad rect %lld,%lld %lldx%lld", fn, k, x, y, w, hh);
			return 1;
		}
	}
	if(int rc = checkIMatAny(m, fn)) return rc;
	if(nTiles <= 0) return 0;
	SnailInstances *h = m->inst;
	std::lock_guard<std::mutex> renderLock(m->renderMu);   // the set's ONE cached tile job, shared with snail_instances_materials_tree_render_tiles
	DeviceGuard guard(m->device);
	HostCallScope hc(h->blas[0], fn);   // (a stream, counters and staging arena of the call's own; the BLAS handle only lends its free list)
	if(hc.rc) return hc.rc;
	if(!m->tileJob) m->tileJob = new InstTileJob();
	InstTileJob &J = *m->tileJob;
	if(int rc = buildInstTileJob(J, resx, resy, coords, nTiles)) return rc;
	if(stats) { if(int rc = hc.zeroStats()) return rc; }
	if(int rc = hc.reserve(HostCallScope::pad(8))) return rc;
	uint64_t *dTrunc = (uint64_t *)hc.carve(8);
	HIP_TRY(hipMemsetAsync(dTrunc, 0, 8, hc.stream()));
	{
		std::lock_guard<std::mutex> lock(h->mu);
		if(int rc = imatTreeStore(m, fn, cam, resx, resy, J.dXY, J.nPackets, lights7, nLights, kMatHeatNoColour, flags, tint, nullptr, &J, maxDepth, dTrunc,
								  stats ? hc.stats() : nullptr, hc.stream(), true, nullptr))
			return rc;
	}
	HIP_TRY(hipMemcpyAsync(J.hPinned, J.dOut, J.planarBytes, hipMemcpyDeviceToHost, hc.stream()));
	uint64_t got = 0;
	if(int rc = hc.get(&got, dTrunc, 8)) return rc;
	if(int rc = hc.finish(stats)) return rc;
	*truncated += got;
	for(int k = 0; k < nTiles; k++)
		memcpy(data + offsets[k], J.hPinned + J.compactOff[(size_t)k], (size_t)3 * coords[(size_t)k * 4 + 2] * coords[(size_t)k * 4 + 3]);
	return 0;
}

int snail_instances_materials_render_heat_frame(SnailInstancesMaterials *m, const float cam[13], int resx, int resy, const float *lights7, int nLights, int flags,
												uint8_t *image, int pitch, int maxDepth, uint64_t *truncated, uint64_t stats[4]) {
	const char *fn = "snail_instances_materials_render_heat_frame";
	if(int rc = matHeatArgsOk(fn, cam, resx, resy, lights7, nLights, flags, SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_AA4, nullptr, maxDepth, truncated)) return rc;
	if(!image || pitch < resx * 3) { snail_set_error("%s: null image or a pitch below 3 * resx", fn); return 1; }
	if(int rc = checkIMatAny(m, fn)) return rc;
	SnailInstances *h = m->inst;
	DeviceGuard guard(m->device);
	HostCallScope hc(h->blas[0], fn);
	if(hc.rc) return hc.rc;
	if(stats) { if(int rc = hc.zeroStats()) return rc; }
	const int np = ((resx + 15) / 16) * ((resy + 15) / 16);
	const size_t row = (size_t)resx * 3;
	typedef HostCallScope H;
	if(int rc = hc.reserve(H::pad((size_t)np * 768) + H::pad(row * resy + 4) + H::pad(8))) return rc;
	uint8_t *bgr = (uint8_t *)hc.carve((size_t)np * 768), *dImg = (uint8_t *)hc.carve(row * resy + 4);
	uint64_t *dTrunc = (uint64_t *)hc.carve(8);
	HIP_TRY(hipMemsetAsync(dTrunc, 0, 8, hc.stream()));
	{
		std::lock_guard<std::mutex> lock(h->mu);
		const int32_t *dXY = nullptr;
		int n = 0;
		if(int rc = imatFrameList(m, resx, resy, &dXY, &n)) return rc;
		// (the frame's packets carry no tint and no planes: their bytes come from k_heat_store, which k_heat_colours + k_inst_store equal byte for byte)
		if(int rc = imatTreeStore(m, fn, cam, resx, resy, dXY, np, lights7, nLights, kMatHeatNoColour, flags, nullptr, bgr, nullptr, maxDepth, dTrunc, stats ? hc.stats() : nullptr,
								  hc.stream(), true, nullptr))
			return rc;
		// (under mu: the cached frame list may be dropped by a later call, which first waits for everything enqueued)
		if(int rc = snail_packets_bgr_to_frame_dev(dXY, np, resx, resy, bgr, dImg, (int)row, hc.stream())) return rc;
	}
	HIP_TRY(hipMemcpy2DAsync(image, (size_t)pitch, dImg, row, row, (size_t)resy, hipMemcpyDeviceToHost, hc.stream()));
	uint64_t got = 0;
	if(int rc = hc.get(&got, dTrunc, 8)) return rc;
	if(int rc = hc.finish(stats)) return rc;
	*truncated += got;
	return 0;
}

} // extern "C"
