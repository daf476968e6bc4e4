// instances_tiles_host.inc -- host side of the tile renderer of instanced scenes (include/snail_instances_tiles.h); included by snail_hip.hip
// after instances_host.inc.  RenderTask::Work (src/render.cpp:47-211) around the staged pipeline of instances_host.inc:
//   [k_inst_aa_packets: the four double-resolution packets of every packet]  ->  k_inst_frame (depth shading) or the lit pipeline with float
//   colours (ShadeArgs::colPackets)  ->  k_inst_store: reduction, tint, ConvColor, packet-major bytes or the tiles' planes.
// The kernels are in instances_shade.inc.
namespace {

// the device-side lists of ONE tile list (SnailInstances::tileJob), rebuilt when (resx, resy, coords) change
struct InstTileJob {
	std::vector<int32_t> coords;
	int resx = 0, resy = 0;
	int nTiles = 0, nPackets = 0;
	size_t planarBytes = 0;
	int32_t *dXY = nullptr, *dTiles = nullptr, *dFirst = nullptr, *dPacketTile = nullptr;
	int64_t *dOff = nullptr;
	uint8_t *dOut = nullptr, *hPinned = nullptr;
	std::vector<int64_t> compactOff; // offset of tile k in the compact device / staging buffer
	bool built = false;              // set after the LAST allocation: a build that failed half-way is never a cache hit
	void release() {
		built = false;
		for(void *p : {(void *)dXY, (void *)dTiles, (void *)dFirst, (void *)dPacketTile, (void *)dOff, (void *)dOut})
			if(p) (void)hipFree(p);
		if(hPinned) (void)hipHostFree(hPinned);
		dXY = dTiles = dFirst = dPacketTile = nullptr; dOff = nullptr; dOut = hPinned = nullptr;
		nTiles = nPackets = 0; planarBytes = 0; coords.clear(); compactOff.clear();
	}
};

void freeInstTileJob(InstTileJob *j) {
	if(j) { j->release(); delete j; }
}

// (the rects were checked by the caller)
int buildInstTileJob(InstTileJob &J, int resx, int resy, const int32_t *coords, int nTiles) {
	if(J.built && J.resx == resx && J.resy == resy && J.coords.size() == (size_t)nTiles * 4 && memcmp(J.coords.data(), coords, (size_t)nTiles * 16) == 0) return 0;
	HIP_TRY(hipDeviceSynchronize());
	J.release();
	J.coords.assign(coords, coords + (size_t)nTiles * 4);
	J.resx = resx; J.resy = resy;
	std::vector<int32_t> xy, first((size_t)nTiles), owner;
	J.compactOff.resize((size_t)nTiles);
	int64_t off = 0;
	for(int k = 0; k < nTiles; k++) {
		const int x = coords[(size_t)k * 4 + 0], y = coords[(size_t)k * 4 + 1], w = coords[(size_t)k * 4 + 2], h = coords[(size_t)k * 4 + 3];
		first[(size_t)k] = (int32_t)(xy.size() / 2);
		for(int py = y; py < y + h; py += 16)       // RenderTask::Work loop order: y outer, x inner (src/render.cpp:67-68)
			for(int px = x; px < x + w; px += 16) { xy.push_back(px); xy.push_back(py); owner.push_back(k); }
		if(xy.size() / 2 > (size_t)1 << 24) { snail_set_error("tile list: more than 2^24 packets"); return 1; }
		J.compactOff[(size_t)k] = off;
		off += (int64_t)3 * w * h;
	}
	J.nTiles = nTiles; J.nPackets = (int)owner.size();
	J.planarBytes = (size_t)off;
	HIP_TRY(hipMalloc((void **)&J.dXY, xy.size() * 4));
	HIP_TRY(hipMemcpy(J.dXY, xy.data(), xy.size() * 4, hipMemcpyHostToDevice));
	HIP_TRY(hipMalloc((void **)&J.dPacketTile, owner.size() * 4));
	HIP_TRY(hipMemcpy(J.dPacketTile, owner.data(), owner.size() * 4, hipMemcpyHostToDevice));
	HIP_TRY(hipMalloc((void **)&J.dTiles, (size_t)nTiles * 16));
	HIP_TRY(hipMemcpy(J.dTiles, coords, (size_t)nTiles * 16, hipMemcpyHostToDevice));
	HIP_TRY(hipMalloc((void **)&J.dFirst, (size_t)nTiles * 4));
	HIP_TRY(hipMemcpy(J.dFirst, first.data(), (size_t)nTiles * 4, hipMemcpyHostToDevice));
	HIP_TRY(hipMalloc((void **)&J.dOff, (size_t)nTiles * 8));
	HIP_TRY(hipMemcpy(J.dOff, J.compactOff.data(), (size_t)nTiles * 8, hipMemcpyHostToDevice));
	HIP_TRY(hipMalloc((void **)&J.dOut, J.planarBytes));
	HIP_TRY(hipMemset(J.dOut, 0, J.planarBytes));   // the store clips to the image: what a tile holds beyond resx x resy stays zero
	HIP_TRY(hipHostMalloc((void **)&J.hPinned, J.planarBytes, hipHostMallocDefault));
	J.built = true;
	return 0;
}

int instTilesArgsOk(const char *fn, const float *cam, int resx, int resy, const float *lights7, int nLights, const float *ambient, const float *color, int flags,
					const float *tint) {
	if(!cam || resx <= 0 || resy <= 0 || resx > (1 << 20) || resy > (1 << 20)) { snail_set_error("%s: bad camera or resolution", fn); return 1; }
	if(flags & ~(SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_DEPTH | SNAIL_RENDER_AA4)) { snail_set_error("%s: unknown flags 0x%x", fn, flags); return 1; }
	if(nLights < 0 || nLights > SNAIL_MAX_LIGHTS || (nLights && !lights7) || !ambient || !color) {
		snail_set_error("%s: bad arguments (at most %d lights, ambient, color)", fn, SNAIL_MAX_LIGHTS);
		return 1;
	}
	if(tint && !(std::isfinite(tint[0]) && std::isfinite(tint[1]) && std::isfinite(tint[2]))) { snail_set_error("%s: the tint is not finite", fn); return 1; }
	return 0;
}

#define SNAIL_INST_STORE(D, AA, PL) SNAIL_LAUNCH(sse, InstStoreArgs, dim3(np), dim3(64), 0, st, S, k_inst_store<D, AA, PL>)

// One run of the pipeline over the np packets of dXY with any flags and tint, into packet-major bytes (bgrPackets) or the planes of J's tiles
// (J->dOut); intermediates from the handle's next set; mu held.
int instancesShadeStore(SnailInstances *h, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights,
						const float ambient[3], const float color[3], int flags, const float *tint, uint8_t *bgrPackets, const InstTileJob *J, uint64_t *dStats,
						hipStream_t st) {
	const bool aa = (flags & SNAIL_RENDER_AA4) != 0, depth = (flags & SNAIL_RENDER_DEPTH) != 0;
	const bool refl = !depth && (flags & SNAIL_RENDER_REFLECTIONS) != 0;
	const size_t n = aa ? (size_t)np * 4 : (size_t)np;
	const int rx = aa ? resx * 2 : resx, ry = aa ? resy * 2 : resy;
	SnailInstances::ShadeSet *Wp = nullptr;
	if(int rc = instancesNextSet(h, n, refl, true, st, &Wp)) return rc;
	SnailInstances::ShadeSet &W = *Wp;
	W.b = SnailInstances::ShadeBufs();
	W.b.carve(W.base, n, depth ? 0 : nLights, refl, true);
	const int32_t *list = dXY;
	if(aa) {
		hipLaunchKernelGGL(dev::k_inst_aa_packets, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const int2 *)dXY, np, (int2 *)W.b.xy2);
		list = W.b.xy2;
	}
	const float *in = nullptr;
	if(depth) { // gVals[1]: the hit distances alone
		dev::InstArgs P;
		bool sse, deep;
		if(int rc = instancesBegin(h, fn, P, &sse, &deep, st)) return rc;
		P.g = makeGen(cam, rx, ry);
		P.resx = rx; P.resy = ry;
		P.packetXY = (const int2 *)list; P.nPackets = (int)n;
		P.t = W.b.hitT;
		P.stats = (dev::u64 *)dStats;
		if(deep) SNAIL_INST_LAUNCH(sse, dim3((unsigned)n), st, P, k_inst_frame<true>);
		else SNAIL_INST_LAUNCH(sse, dim3((unsigned)n), st, P, k_inst_frame<false>);
		if(int rc = instancesEnd(h, st)) return rc;
		in = W.b.hitT;
	} else {
		if(int rc = instancesShade(h, fn, cam, rx, ry, list, (int)n, lights7, nLights, ambient, color, refl, nullptr, 0, nullptr, W.b, dStats, st, W.b.col)) return rc;
		in = W.b.col;
	}
	const bool sse = h->blas[0]->arith == SNAIL_ARITH_HOST_SSE;
	dev::InstStoreArgs S;
	memset(&S, 0, sizeof(S));
	S.hostTab = sse ? h->blas[0]->dTab : nullptr;
	S.in = in;
	S.nPackets = np;
	if(tint) { S.tinted = 1; for(int c = 0; c < 3; c++) S.tint[c] = tint[c]; }
	S.bgrPackets = bgrPackets;
	if(J) {
		S.tiles = (const int4 *)J->dTiles; S.packetTile = J->dPacketTile; S.firstPacket = J->dFirst; S.outOff = (const long long *)J->dOff;
		S.out = J->dOut; S.resx = resx; S.resy = resy;
	}
	switch((depth ? 4 : 0) | (aa ? 2 : 0) | (J ? 1 : 0)) {
	case 0: SNAIL_INST_STORE(false, false, false); break;
	case 1: SNAIL_INST_STORE(false, false, true); break;
	case 2: SNAIL_INST_STORE(false, true, false); break;
	case 3: SNAIL_INST_STORE(false, true, true); break;
	case 4: SNAIL_INST_STORE(true, false, false); break;
	case 5: SNAIL_INST_STORE(true, false, true); break;
	case 6: SNAIL_INST_STORE(true, true, false); break;
	default: SNAIL_INST_STORE(true, true, true); break;
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(W.done, st));
	W.used = true;
	return 0;
}
#undef SNAIL_INST_STORE

} // namespace

extern "C" {

int snail_instances_shade_packets_dev(SnailInstances *h, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets, const float *lights7,
									  int nLights, const float ambient[3], const float color[3], int flags, const float *tint, uint8_t *bgrPackets, uint64_t *dStats,
									  void *stream) {
	const char *fn = "snail_instances_shade_packets_dev";
	if(int rc = checkInstances(h, fn)) return rc;
	if(!dPacketXY && nPackets > 0) { snail_set_error("%s: null packet list", fn); return 1; }
	if(nPackets <= 0) return 0;
	if(int rc = instTilesArgsOk(fn, cam, resx, resy, lights7, nLights, ambient, color, flags, tint)) return rc;
	if(nPackets > (1 << 24)) { snail_set_error("%s: more than 2^24 packets", fn); return 1; }
	if(!bgrPackets || ((unsigned long long)bgrPackets & 3)) { snail_set_error("%s: null or unaligned output", fn); return 1; }
	DeviceGuard guard(h->device);
	std::lock_guard<std::mutex> lock(h->mu);
	if(!tint && !(flags & (SNAIL_RENDER_DEPTH | SNAIL_RENDER_AA4)))   // the lit packets as they are: the merged path, bytes from k_inst_final
		return instancesShadeDev(h, fn, cam, resx, resy, dPacketXY, nPackets, lights7, nLights, ambient, color,
								 (flags & SNAIL_RENDER_REFLECTIONS) ? SNAIL_WHITTED_REFLECTIONS : 0, nullptr, 0, bgrPackets, dStats, (hipStream_t)stream);
	return instancesShadeStore(h, fn, cam, resx, resy, dPacketXY, nPackets, lights7, nLights, ambient, color, flags, tint, bgrPackets, nullptr, dStats, (hipStream_t)stream);
}

int snail_instances_render_tiles(SnailInstances *h, const float cam[13], int resx, int resy, const int32_t *coords, const int64_t *offsets, int nTiles,
								 const float *lights7, int nLights, const float ambient[3], const float color[3], int flags, const float *tint, uint8_t *data,
								 uint64_t stats[4]) {
	const char *fn = "snail_instances_render_tiles";
	if(int rc = checkInstances(h, fn)) return rc;
	if(nTiles <= 0) return 0;
	if(!coords || !offsets || !data) { snail_set_error("%s: null buffer", fn); return 1; }
	if(int rc = instTilesArgsOk(fn, cam, resx, resy, lights7, nLights, ambient, color, flags, tint)) return rc;
	for(int k = 0; k < nTiles; k++) {
		const long long x = coords[(size_t)k * 4 + 0], y = coords[(size_t)k * 4 + 1], w = coords[(size_t)k * 4 + 2], hh = coords[(size_t)k * 4 + 3];
		if(w <= 0 || hh <= 0 || x < 0 || y < 0 || x + w > (1 << 24) || y + hh > (1 << 24)) {
			snail_set_error("%s: tile %d: bad rect %lld,%lld %lldx%lld", fn, k, x, y, w, hh);
			return 1;
		}
	}
	std::lock_guard<std::mutex> renderLock(h->renderMu);   // one cached tile job per handle: its calls take turns
	DeviceGuard guard(h->device);
	HostCallScope hc(h->blas[0], fn);   // (a stream, counters and staging arena of the call's own; the BLAS handle only lends its free list)
	if(hc.rc) return hc.rc;
	if(!h->tileJob) h->tileJob = new InstTileJob();
	InstTileJob &J = *h->tileJob;
	if(int rc = buildInstTileJob(J, resx, resy, coords, nTiles)) return rc;
	if(stats) { if(int rc = hc.zeroStats()) return rc; }
	{
		std::lock_guard<std::mutex> lock(h->mu);
		if(int rc = instancesShadeStore(h, fn, cam, resx, resy, J.dXY, J.nPackets, lights7, nLights, ambient, color, flags, tint, nullptr, &J, stats ? hc.stats() : nullptr,
										hc.stream()))
			return rc;
	}
	HIP_TRY(hipMemcpyAsync(J.hPinned, J.dOut, J.planarBytes, hipMemcpyDeviceToHost, hc.stream()));
	if(int rc = hc.finish(stats)) return rc;
	for(int k = 0; k < nTiles; k++)
		memcpy(data + offsets[k], J.hPinned + J.compactOff[(size_t)k], (size_t)3 * coords[(size_t)k * 4 + 2] * coords[(size_t)k * 4 + 3]);
	return 0;
}

int snail_instances_render_frame(SnailInstances *h, const float cam[13], int resx, int resy, const float *lights7, int nLights, const float ambient[3],
								 const float color[3], int flags, uint8_t *image, int pitch, uint64_t stats[4]) {
	const char *fn = "snail_instances_render_frame";
	if(int rc = checkInstances(h, fn)) return rc;
	if(flags & ~(SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_DEPTH | SNAIL_RENDER_AA4)) { snail_set_error("%s: unknown flags 0x%x", fn, flags); return 1; }
	if(!(flags & SNAIL_RENDER_AA4)) return snail_instances_render_image(h, cam, resx, resy, lights7, nLights, ambient, color, flags, image, pitch, stats);
	if(int rc = instTilesArgsOk(fn, cam, resx, resy, lights7, nLights, ambient, color, flags, nullptr)) return rc;
	if(!image || pitch < resx * 3) { snail_set_error("%s: bad image", fn); return 1; }
	DeviceGuard guard(h->device);
	HostCallScope hc(h->blas[0], fn);
	if(hc.rc) return hc.rc;
	if(stats) { if(int rc = hc.zeroStats()) return rc; }
	const int np = ((resx + 15) / 16) * ((resy + 15) / 16);
	const size_t row = (size_t)resx * 3;
	typedef HostCallScope H;
	if(int rc = hc.reserve(H::pad((size_t)np * 768) + H::pad(row * resy + 4))) return rc;
	uint8_t *bgr = (uint8_t *)hc.carve((size_t)np * 768), *dImg = (uint8_t *)hc.carve(row * resy + 4);
	const int32_t *dXY = nullptr;
	{
		std::lock_guard<std::mutex> lock(h->mu);
		int n = 0;
		if(int rc = h->frameLists.get(resx, resy, &dXY, &n)) return rc;
		if(int rc = instancesShadeStore(h, fn, cam, resx, resy, dXY, np, lights7, nLights, ambient, color, flags, nullptr, bgr, nullptr, stats ? hc.stats() : nullptr, hc.stream()))
			return rc;
		// (under mu: the cached frame list may be dropped by a later call, which first waits for everything enqueued)
		if(int rc = snail_packets_bgr_to_frame_dev(dXY, np, resx, resy, bgr, dImg, (int)row, hc.stream())) return rc;
	}
	HIP_TRY(hipMemcpy2DAsync(image, (size_t)pitch, dImg, row, row, (size_t)resy, hipMemcpyDeviceToHost, hc.stream()));
	return hc.finish(stats);
}

} // extern "C"
