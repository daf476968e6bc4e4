// heatmap_host.inc -- C-ABI of include/snail_heatmap.h (included by snail_hip.hip last: the host-pointer forms share the cached tile jobs of
// render_host.inc and instances_tiles_host.inc).  Plain scenes: every form is renderWhitted with a HeatOut -- the staged pipeline of the lit frame
// with per-packet booking (dev::bookPacket) and dev_heat::k_heat_store in place of the colour stores.  Instanced scenes: instancesShade with a
// per-packet array, then the counters' colours as floats (dev_heat::k_heat_colours) into the tile renderer's own store stage (dev::k_inst_store:
// reduction, rank tint, ConvColor, bytes or planes).
namespace {

// everything that can be refused before a device is touched; `allowed` = the flag bits of the entry point
int heatArgsOk(const char *fn, const SnailScene *s, const float *cam, int resx, int resy, const float *lights7, int nLights, int flags, int allowed) {
	if(flags & SNAIL_RENDER_DEPTH) {
		snail_set_error("%s: SNAIL_RENDER_DEPTH has no heat-map (gVals[1] returns from RayTrace before the counters' colour): use the depth entry points", fn);
		return 1;
	}
	if(flags & ~allowed) { snail_set_error("%s: unknown or unsupported flag bits 0x%x (allowed: 0x%x)", fn, flags & ~allowed, allowed); return 1; }
	if(nLights < 0 || nLights > SNAIL_MAX_LIGHTS || (nLights && !lights7)) { snail_set_error("%s: 0..%d lights (got %d) with a non-null lights7", fn, SNAIL_MAX_LIGHTS, nLights); return 1; }
	if(int rc = checkScene(s, fn)) return rc;
	if(!cam || resx <= 0 || resy <= 0) { snail_set_error("%s: null camera or bad resolution %dx%d", fn, resx, resy); return 1; }
	return 0;
}

// the colour of the material does not reach a counter: any ambient / colour will do for the record the stages share
const float kHeatNoColour[3] = {0.0f, 0.0f, 0.0f};

int heatLaunch(const char *fn, SnailScene *s, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets, const float *lights7, int nLights, int flags,
			   uint8_t *dBgr, uint32_t *dPacketStats, uint64_t *dStats, hipStream_t stream) {
	HeatOut H;
	H.dPacketStats = dPacketStats; H.dBgr = dBgr; H.aa = (flags & SNAIL_RENDER_AA4) != 0;
	SNAIL_LOCK(s);
	return renderWhitted(fn, s, cam, resx, resy, dPacketXY, nPackets, lights7, nLights, kHeatNoColour, kHeatNoColour, (flags & SNAIL_RENDER_REFLECTIONS) ? SNAIL_WHITTED_REFLECTIONS : 0,
						 nullptr, 0, nullptr, dStats, stream, nullptr, nullptr, nullptr, nullptr, 0, &H);
}

} // namespace

extern "C" {

int snail_packet_stats_dev(SnailScene *s, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets, const float *lights7, int nLights, int flags,
						   uint32_t *dPacketStats, uint64_t *dStats, void *stream) {
	if(int rc = heatArgsOk("snail_packet_stats_dev", s, cam, resx, resy, lights7, nLights, flags, SNAIL_RENDER_REFLECTIONS)) return rc;
	if(dPacketXY && nPackets <= 0) return 0;
	if(!dPacketStats || ((uintptr_t)dPacketStats & 3) || ((uintptr_t)dStats & 7)) { snail_set_error("snail_packet_stats_dev: d_packet_stats must be a 4-byte aligned device pointer (d_stats: 8-byte aligned or null)"); return 1; }
	return heatLaunch("snail_packet_stats_dev", s, cam, resx, resy, dPacketXY, nPackets, lights7, nLights, flags, nullptr, dPacketStats, dStats, (hipStream_t)stream);
}

int snail_render_heat_packets_dev(SnailScene *s, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets, const float *lights7, int nLights, int flags,
								  uint8_t *dBgr, uint32_t *dPacketStats, uint64_t *dStats, void *stream) {
	if(int rc = heatArgsOk("snail_render_heat_packets_dev", s, cam, resx, resy, lights7, nLights, flags, SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_AA4)) return rc;
	if(dPacketXY && nPackets <= 0) return 0;
	if(!dBgr || ((uintptr_t)dBgr & 3) || ((uintptr_t)dPacketStats & 3) || ((uintptr_t)dStats & 7)) {
		snail_set_error("snail_render_heat_packets_dev: d_bgr_packets must be a 4-byte aligned device pointer (d_packet_stats: 4-byte aligned or null; d_stats: 8-byte aligned or null)");
		return 1;
	}
	return heatLaunch("snail_render_heat_packets_dev", s, cam, resx, resy, dPacketXY, nPackets, lights7, nLights, flags, dBgr, dPacketStats, dStats, (hipStream_t)stream);
}

int snail_render_heat_tiles(SnailScene *s, const float cam[13], int resx, int resy, const int32_t *coords, const int64_t *offsets, int nTiles, const float *lights7, int nLights,
							int flags, uint8_t *data, uint64_t stats[4]) {
	if(int rc = heatArgsOk("snail_render_heat_tiles", s, cam, resx, resy, lights7, nLights, flags, SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_AA4)) return rc;
	if(nTiles <= 0) return 0;
	if(!coords || !offsets || !data) { snail_set_error("snail_render_heat_tiles: null buffer"); return 1; }
	std::lock_guard<std::mutex> renderLock(s->renderMu);   // the scene's ONE cached tile job, shared with snail_render_tiles
	DeviceGuard guard(s->device);
	HostCallScope hc(s, "snail_render_heat_tiles");
	if(hc.rc) return hc.rc;
	if(!s->tileJob) s->tileJob = new TileJob();
	TileJob &J = *s->tileJob;
	if(int rc = buildTileJob(J, resx, resy, coords, nTiles, false)) return rc;
	if(stats) { if(int rc = hc.zeroStats()) return rc; }
	if(int rc = heatLaunch("snail_render_heat_tiles", s, cam, resx, resy, J.dXY, J.nPackets, lights7, nLights, flags, J.dBgr, nullptr, stats ? hc.stats() : nullptr, hc.stream())) return rc;
	for(int t0 = 0; t0 < nTiles; t0 += 65535) {   // the encode kernel's grid.y limit
		const int nt = nTiles - t0 < 65535 ? nTiles - t0 : 65535;
		if(int rc = snail_packets_bgr_to_planar_dev(J.dTiles + (size_t)t0 * 4, J.dFirst + t0, J.dOff + t0, nt, J.dBgr, J.dOut, hc.stream())) return rc;
	}
	HIP_TRY(hipMemcpyAsync(J.hPinned, J.dOut, J.planarBytes, hipMemcpyDeviceToHost, hc.stream()));
	return renderTilesEnd(s, coords, offsets, nTiles, data, hc, stats);
}

int snail_render_heat_image(SnailScene *s, const float cam[13], int resx, int resy, const float *lights7, int nLights, int flags, uint8_t *image_bgr, int pitch, uint64_t stats[4]) {
	if(int rc = heatArgsOk("snail_render_heat_image", s, cam, resx, resy, lights7, nLights, flags, SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_AA4)) return rc;
	if(!image_bgr || pitch < resx * 3) { snail_set_error("snail_render_heat_image: null image or pitch < 3 * resx"); return 1; }
	std::lock_guard<std::mutex> renderLock(s->renderMu);   // the scene's ONE cached frame job, shared with snail_render_image
	DeviceGuard guard(s->device);
	HostCallScope hc(s, "snail_render_heat_image");
	if(hc.rc) return hc.rc;
	if(!s->frameJob) s->frameJob = new TileJob();
	TileJob &J = *s->frameJob;
	if(int rc = buildTileJob(J, resx, resy, nullptr, 1, true)) return rc;
	if(stats) { if(int rc = hc.zeroStats()) return rc; }
	if(int rc = heatLaunch("snail_render_heat_image", s, cam, resx, resy, J.dXY, J.nPackets, lights7, nLights, flags, J.dBgr, nullptr, stats ? hc.stats() : nullptr, hc.stream())) return rc;
	if(int rc = snail_packets_bgr_to_frame_dev(J.dXY, J.nPackets, resx, resy, J.dBgr, J.dOut, resx * 3, hc.stream())) return rc;
	HIP_TRY(hipMemcpyAsync(J.hPinned, J.dOut, J.planarBytes, hipMemcpyDeviceToHost, hc.stream()));
	if(int rc = hc.finish(stats)) return rc;
	for(int y = 0; y < resy; y++) memcpy(image_bgr + (size_t)y * pitch, J.hPinned + (size_t)y * resx * 3, (size_t)resx * 3);
	return 0;
}

} // extern "C"

// ---- instanced scenes -------------------------------------------------------------------------------------------------------------------------
namespace {

int instHeatArgsOk(const char *fn, const SnailInstances *h, const float *cam, int resx, int resy, const float *lights7, int nLights, int flags, int allowed, const float *tint) {
	if(flags & SNAIL_RENDER_DEPTH) {
		snail_set_error("%s: SNAIL_RENDER_DEPTH has no heat-map (gVals[1] returns from RayTrace before the counters' colour): use the depth entry points", fn);
		return 1;
	}
	if(flags & ~allowed) { snail_set_error("%s: unknown or unsupported flag bits 0x%x (allowed: 0x%x)", fn, flags & ~allowed, allowed); return 1; }
	if(nLights < 0 || nLights > SNAIL_MAX_LIGHTS || (nLights && !lights7)) { snail_set_error("%s: 0..%d lights (got %d) with a non-null lights7", fn, SNAIL_MAX_LIGHTS, nLights); return 1; }
	if(int rc = checkInstances(h, fn)) return rc;
	if(!cam || resx <= 0 || resy <= 0 || resx > (1 << 20) || resy > (1 << 20)) { snail_set_error("%s: null camera or bad resolution %dx%d", fn, resx, resy); return 1; }
	if(tint && !(std::isfinite(tint[0]) && std::isfinite(tint[1]) && std::isfinite(tint[2]))) { snail_set_error("%s: the tint is not finite", fn); return 1; }
	return 0;
}

// One heat-map run over the np packets of dXY (null: the frame's grid, row-major): counters into dPacketStats (or the set's own array), colours -- if any
// output is given -- through k_inst_store into packet-major bytes (bgrPackets) or the planes of J's tiles.  mu held.
int instancesHeat(SnailInstances *h, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights, int flags,
				  const float *tint, uint8_t *bgrPackets, const InstTileJob *J, uint32_t *dPacketStats, uint64_t *dStats, hipStream_t st) {
	if(!dXY) { if(int rc = h->frameLists.get(resx, resy, &dXY, &np)) return rc; }
	if(np > (1 << 24)) { snail_set_error("%s: more than 2^24 packets", fn); return 1; }
	const bool aa = (flags & SNAIL_RENDER_AA4) != 0, refl = (flags & SNAIL_RENDER_REFLECTIONS) != 0;
	const size_t n = aa ? (size_t)np * 4 : (size_t)np;
	const int rx = aa ? resx * 2 : resx, ry = aa ? resy * 2 : resy;
	SnailInstances::ShadeSet *Wp = nullptr;
	if(int rc = instancesNextSet(h, n, refl, true, st, &Wp)) return rc;
	SnailInstances::ShadeSet &W = *Wp;
	W.b = SnailInstances::ShadeBufs();
	W.b.carve(W.base, n, nLights, refl, true);
	const int32_t *list = dXY;
	if(aa) {
		hipLaunchKernelGGL(dev::k_inst_aa_packets, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const int2 *)dXY, np, (int2 *)W.b.xy2);
		list = W.b.xy2;
	}
	uint32_t *pst = dPacketStats ? dPacketStats : W.b.pstats;
	HIP_TRY(hipMemsetAsync(pst, 0, n * 16, st));
	if(int rc = instancesShade(h, fn, cam, rx, ry, list, (int)n, lights7, nLights, kHeatNoColour, kHeatNoColour, refl, nullptr, 0, nullptr, W.b, dStats, st, nullptr, pst)) return rc;
	if(bgrPackets || J) {
		hipLaunchKernelGGL(dev_heat::k_heat_colours, dim3((unsigned)n), dim3(64), 0, st, (const unsigned *)pst, (int)n, W.b.col);
		dev::InstStoreArgs S;
		memset(&S, 0, sizeof(S));
		S.in = W.b.col;
		S.nPackets = np;
		if(tint) { S.tinted = 1; for(int c = 0; c < 3; c++) S.tint[c] = tint[c]; }
		S.bgrPackets = bgrPackets;
		if(J) {
			S.tiles = (const int4 *)J->dTiles; S.packetTile = J->dPacketTile; S.firstPacket = J->dFirst; S.outOff = (const long long *)J->dOff;
			S.out = J->dOut; S.resx = resx; S.resy = resy;
		}
		// (no look-up in the colour path: the IEEE namespace's store serves both arithmetics)
		const dim3 grid((unsigned)np), wave(64);
		if(aa && J) hipLaunchKernelGGL((dev::k_inst_store<false, true, true>), grid, wave, 0, st, S);
		else if(aa) hipLaunchKernelGGL((dev::k_inst_store<false, true, false>), grid, wave, 0, st, S);
		else if(J) hipLaunchKernelGGL((dev::k_inst_store<false, false, true>), grid, wave, 0, st, S);
		else hipLaunchKernelGGL((dev::k_inst_store<false, false, false>), grid, wave, 0, st, S);
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(W.done, st));
	W.used = true;
	return 0;
}

} // namespace

extern "C" {

int snail_instances_packet_stats_dev(SnailInstances *h, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets, const float *lights7, int nLights,
									 int flags, uint32_t *dPacketStats, uint64_t *dStats, void *stream) {
	const char *fn = "snail_instances_packet_stats_dev";
	if(int rc = instHeatArgsOk(fn, h, cam, resx, resy, lights7, nLights, flags, SNAIL_RENDER_REFLECTIONS, nullptr)) return rc;
	if(dPacketXY && nPackets <= 0) return 0;
	if(!dPacketStats || ((uintptr_t)dPacketStats & 3) || ((uintptr_t)dStats & 7)) { snail_set_error("%s: d_packet_stats must be a 4-byte aligned device pointer (d_stats: 8-byte aligned or null)", fn); return 1; }
	DeviceGuard guard(h->device);
	std::lock_guard<std::mutex> lock(h->mu);
	return instancesHeat(h, fn, cam, resx, resy, dPacketXY, nPackets, lights7, nLights, flags, nullptr, nullptr, nullptr, dPacketStats, dStats, (hipStream_t)stream);
}

int snail_instances_heat_packets_dev(SnailInstances *h, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets, const float *lights7, int nLights,
									 int flags, const float *tint, uint8_t *dBgr, uint32_t *dPacketStats, uint64_t *dStats, void *stream) {
	const char *fn = "snail_instances_heat_packets_dev";
	if(int rc = instHeatArgsOk(fn, h, cam, resx, resy, lights7, nLights, flags, SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_AA4, tint)) return rc;
	if(dPacketXY && nPackets <= 0) return 0;
	if(!dBgr || ((uintptr_t)dBgr & 3) || ((uintptr_t)dPacketStats & 3) || ((uintptr_t)dStats & 7)) {
		snail_set_error("%s: d_bgr_packets must be a 4-byte aligned device pointer (d_packet_stats: 4-byte aligned or null; d_stats: 8-byte aligned or null)", fn);
		return 1;
	}
	DeviceGuard guard(h->device);
	std::lock_guard<std::mutex> lock(h->mu);
	return instancesHeat(h, fn, cam, resx, resy, dPacketXY, nPackets, lights7, nLights, flags, tint, dBgr, nullptr, dPacketStats, dStats, (hipStream_t)stream);
}

int snail_instances_render_heat_tiles(SnailInstances *h, const float cam[13], int resx, int resy, const int32_t *coords, const int64_t *offsets, int nTiles, const float *lights7,
									  int nLights, int flags, const float *tint, uint8_t *data, uint64_t stats[4]) {
	const char *fn = "snail_instances_render_heat_tiles";
	if(int rc = instHeatArgsOk(fn, h, cam, resx, resy, lights7, nLights, flags, SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_AA4, tint)) return rc;
	if(nTiles <= 0) return 0;
	if(!coords || !offsets || !data) { snail_set_error("%s: null buffer", fn); return 1; }
	for(int k = 0; k < nTiles; k++) {
		const long long x = coords[(size_t)k * 4 + 0], y = coords[(size_t)k * 4 + 1], w = coords[(size_t)k * 4 + 2], hh = coords[(size_t)k * 4 + 3];
		if(w <= 0 || hh <= 0 || x < 0 || y < 0 || x + w > (1 << 24) || y + hh > (1 << 24)) { snail_set_error("%s: tile %d: bad rect %lld,%lld %lldx%lld", fn, k, x, y, w, hh); return 1; }
	}
	std::lock_guard<std::mutex> renderLock(h->renderMu);   // the handle's ONE cached tile job, shared with snail_instances_render_tiles
	DeviceGuard guard(h->device);
	HostCallScope hc(h->blas[0], fn);
	if(hc.rc) return hc.rc;
	if(!h->tileJob) h->tileJob = new InstTileJob();
	InstTileJob &J = *h->tileJob;
	if(int rc = buildInstTileJob(J, resx, resy, coords, nTiles)) return rc;
	if(stats) { if(int rc = hc.zeroStats()) return rc; }
	{
		std::lock_guard<std::mutex> lock(h->mu);
		if(int rc = instancesHeat(h, fn, cam, resx, resy, J.dXY, J.nPackets, lights7, nLights, flags, tint, nullptr, &J, nullptr, stats ? hc.stats() : nullptr, hc.stream())) return rc;
	}
	HIP_TRY(hipMemcpyAsync(J.hPinned, J.dOut, J.planarBytes, hipMemcpyDeviceToHost, hc.stream()));
	if(int rc = hc.finish(stats)) return rc;
	for(int k = 0; k < nTiles; k++)
		memcpy(data + offsets[k], J.hPinned + J.compactOff[(size_t)k], (size_t)3 * coords[(size_t)k * 4 + 2] * coords[(size_t)k * 4 + 3]);
	return 0;
}

int snail_instances_render_heat_frame(SnailInstances *h, const float cam[13], int resx, int resy, const float *lights7, int nLights, int flags, uint8_t *image, int pitch,
									  uint64_t stats[4]) {
	const char *fn = "snail_instances_render_heat_frame";
	if(int rc = instHeatArgsOk(fn, h, cam, resx, resy, lights7, nLights, flags, SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_AA4, nullptr)) return rc;
	if(!image || pitch < resx * 3) { snail_set_error("%s: null image or pitch < 3 * resx", fn); return 1; }
	DeviceGuard guard(h->device);
	HostCallScope hc(h->blas[0], fn);
	if(hc.rc) return hc.rc;
	if(stats) { if(int rc = hc.zeroStats()) return rc; }
	const int np = ((resx + 15) / 16) * ((resy + 15) / 16);
	const size_t row = (size_t)resx * 3;
	typedef HostCallScope H;
	if(int rc = hc.reserve(H::pad((size_t)np * 768) + H::pad(row * resy + 4))) return rc;
	uint8_t *bgr = (uint8_t *)hc.carve((size_t)np * 768), *dImg = (uint8_t *)hc.carve(row * resy + 4);
	{
		std::lock_guard<std::mutex> lock(h->mu);
		const int32_t *dXY = nullptr;
		int n = 0;
		if(int rc = h->frameLists.get(resx, resy, &dXY, &n)) return rc;
		if(int rc = instancesHeat(h, fn, cam, resx, resy, dXY, np, lights7, nLights, flags, nullptr, bgr, nullptr, nullptr, stats ? hc.stats() : nullptr, hc.stream())) return rc;
		// (under mu: the cached frame list may be dropped by a later call, which first waits for everything enqueued)
		if(int rc = snail_packets_bgr_to_frame_dev(dXY, np, resx, resy, bgr, dImg, (int)row, hc.stream())) return rc;
	}
	HIP_TRY(hipMemcpy2DAsync(image, (size_t)pitch, dImg, row, row, (size_t)resy, hipMemcpyDeviceToHost, hc.stream()));
	return hc.finish(stats);
}

} // extern "C"
