// wide_host.inc -- the C-ABI of include/snail_wide.h: BVH::WideTrace with one ray per lane and the photon pass (kernels: wide.inc).
namespace {

// what can be judged without the handle (the header's list), for both forms
int wideCheckArgs(const char *fn, int nRays, const float *origin, const float *dir, const int32_t *indices, int nIndices, const float *dist, int startNode) {
	if(nRays < 0 || (indices && nIndices < 0)) { snail_set_error("%s: negative count (nRays %d, nIndices %d)", fn, nRays, nIndices); return 1; }
	if(startNode < 0) { snail_set_error("%s: startNode %d outside the tree", fn, startNode); return 1; }
	if(nRays > 0 && (!origin || !dir || !dist)) { snail_set_error("%s: null ray array (origin, dir and dist are required)", fn); return 1; }
	return 0;
}

int photonCheckArgs(const char *fn, int nLights, int count, const float *origin, const float *dir, const float *lights7, const void *photons, const void *nPhotons) {
	if(nLights < 0 || nLights > SNAIL_MAX_LIGHTS) { snail_set_error("%s: %d lights outside 0..%d", fn, nLights, SNAIL_MAX_LIGHTS); return 1; }
	if(count < 0) { snail_set_error("%s: negative count (%d photons per light)", fn, count); return 1; }
	if(!nPhotons) { snail_set_error("%s: null photon count", fn); return 1; }
	if((long long)nLights * count > 0x7fffffffLL / 8) { snail_set_error("%s: %d x %d photons are more than one call takes", fn, nLights, count); return 1; }
	if(nLights * count > 0 && (!origin || !dir || !lights7 || !photons)) { snail_set_error("%s: null buffer (origin, dir, lights and photons are required)", fn); return 1; }
	return 0;
}

// stack entries per lane: the tree's depth (a handle that is rebuilt on the device: the depth its builder may reach)
int wideSlots(const SnailScene *s) { return std::max(1, s->fast ? s->fast->depthLimit : s->depth); }

// what needs the handle: startNode inside the node array, a depth the LDS stack takes
int wideCheckScene(const char *fn, const SnailScene *s, int startNode) {
	if(int rc = checkScene(s, fn)) return rc;
	if(startNode >= s->nNodes) { snail_set_error("%s: startNode %d outside the tree (%d nodes)", fn, startNode, s->nNodes); return 1; }
	if(wideSlots(s) > SNAIL_MAX_DEPTH) { snail_set_error("%s: the tree is %d levels deep, the per-lane stack takes %d", fn, wideSlots(s), SNAIL_MAX_DEPTH); return 1; }
	return 0;
}

// (mu held, arguments judged)
int launchWide(SnailScene *s, int nRays, const float *origin, const float *dir, const float *idir, const int32_t *indices, int nIndices, float *dist,
			   int startNode, int32_t *visits, uint64_t *dStats, hipStream_t stream) {
	const int n = indices ? nIndices : nRays;
	if(n <= 0 || nRays <= 0) return 0;
	SceneUse use(s, stream);
	if(use.rc) return use.rc;
	devw::WideArgs A;
	memset((void *)&A, 0, sizeof(A));
	A.nodes = s->dNodes; A.tris = s->dTris; A.nNodes = s->nNodes; A.nTris = s->nTris;
	A.origin = origin; A.dir = dir; A.idir = idir; A.indices = indices; A.n = n; A.nRays = nRays;
	A.dist = dist; A.startNode = startNode; A.slots = wideSlots(s);
	A.visits = visits; A.stats = (unsigned long long *)dStats;
	const unsigned blocks = (unsigned)(((long long)n + 63) / 64);
	hipLaunchKernelGGL(devw::k_wide_trace, dim3(blocks), dim3(64), (size_t)A.slots * 64 * sizeof(int), stream, A);
	HIP_TRY(hipGetLastError());
	s->lastBlocks = (int)blocks; s->lastThreads = 64;
	return 0;
}

// Photon::Photon's colour bytes (src/photons.h:11-13): u8(Clamp(c * 255, 0, 255)), Clamp = Min(Max(x, lo), hi) in veclib's select forms
unsigned photonColour(const float *rgb) {
	unsigned out = 0;
	for(int k = 0; k < 3; k++) {
		float x = rgb[k] * 255.0f;
		x = x > 0.0f ? x : 0.0f;
		x = x < 255.0f ? x : 255.0f;
		out |= (unsigned)(uint8_t)x << (8 * k);
	}
	return out;
}

// (mu held, arguments judged, n = nLights * count > 0)
int launchPhotons(SnailScene *s, int nLights, int count, const float *origin, const float *dir, const float *lights7, SnailPhoton *photons,
				  int32_t *nPhotons, uint64_t *dStats, hipStream_t stream) {
	const int n = nLights * count;
	const int nBlocks = (n + devw::kPhotonBlock - 1) / devw::kPhotonBlock;
	const size_t distBytes = HostCallScope::pad((size_t)n * sizeof(float)), need = distBytes + ((size_t)nBlocks + 1) * sizeof(unsigned);
	SnailScene::WideScratch &W = s->wide[s->wideCount++ % SnailScene::kDeferSlots];
	if(need > W.cap) {   // grown synchronously when a larger launch than ever before arrives (as launchRays' lists)
		HIP_TRY(hipDeviceSynchronize());
		if(W.p) (void)hipFree(W.p);
		W.p = nullptr; W.cap = 0;
		HIP_TRY(hipMalloc((void **)&W.p, need));
		W.cap = need;
	}
	if(!W.done) HIP_TRY(hipEventCreateWithFlags(&W.done, hipEventDisableTiming));
	if(W.used) HIP_TRY(hipStreamWaitEvent(stream, W.done, 0));
	float *dist = (float *)W.p;
	HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)dist, 0x7f800000, (size_t)n, stream));   // dists[n] = constant::inf
	if(int rc = launchWide(s, n, origin, dir, nullptr, nullptr, 0, dist, 0, nullptr, dStats, stream)) return rc;
	devw::PhotonArgs P;
	memset((void *)&P, 0, sizeof(P));
	P.origin = origin; P.dir = dir; P.dist = dist; P.n = n; P.count = count;
	for(int l = 0; l < nLights; l++) P.colour[l] = photonColour(lights7 + 7 * l + 3);
	P.blockCount = (unsigned *)(W.p + distBytes); P.nBlocks = nBlocks;
	P.photons = (unsigned *)photons; P.nPhotons = nPhotons;
	// three launches, each complete before the next starts: no workgroup ever waits for another
	hipLaunchKernelGGL(devw::k_photon_flag, dim3((unsigned)nBlocks), dim3(devw::kPhotonBlock), 0, stream, P);
	hipLaunchKernelGGL(devw::k_photon_scan, dim3(1), dim3(1024), 0, stream, P);
	hipLaunchKernelGGL(devw::k_photon_scatter, dim3((unsigned)nBlocks), dim3(devw::kPhotonBlock), 0, stream, P);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(W.done, stream));
	W.used = true;
	return 0;
}

} // namespace

extern "C" {

int snail_wide_trace_dev(SnailScene *s, int nRays, const float *origin, const float *dir, const float *idir, const int32_t *indices, int nIndices,
						 float *dist, int startNode, int32_t *visits, uint64_t *dStats, void *stream) {
	const char *fn = "snail_wide_trace_dev";
	if(int rc = wideCheckArgs(fn, nRays, origin, dir, indices, nIndices, dist, startNode)) return rc;
	if(nRays == 0) return 0;
	if(int rc = wideCheckScene(fn, s, startNode)) return rc;
	DeviceGuard guard(s->device);
	SNAIL_LOCK(s);
	return launchWide(s, nRays, origin, dir, idir, indices, nIndices, dist, startNode, visits, dStats, (hipStream_t)stream);
}

int snail_wide_trace(SnailScene *s, int nRays, const float *origin, const float *dir, const float *idir, const int32_t *indices, int nIndices,
					 float *dist, int startNode, int32_t *visits, uint64_t *stats2) {
	const char *fn = "snail_wide_trace";
	if(int rc = wideCheckArgs(fn, nRays, origin, dir, indices, nIndices, dist, startNode)) return rc;
	if(nRays == 0) return 0;
	if(int rc = wideCheckScene(fn, s, startNode)) return rc;
	const int n = indices ? nIndices : nRays;
	if(n <= 0 || nRays <= 0) return 0;
	DeviceGuard guard(s->device);
	HostCallScope hc(s, fn);
	if(hc.rc) return hc.rc;
	typedef HostCallScope H;
	const size_t b3 = (size_t)nRays * 12, b1 = (size_t)nRays * 4;
	if(int rc = hc.reserve(3 * H::pad(b3) + H::pad((size_t)n * 4) + H::pad(b1) + H::pad(2 * b1))) return rc;
	void *o = nullptr, *d = nullptr, *i = nullptr, *ix = nullptr, *ds = nullptr, *vs = nullptr;
	if(int rc = hc.put(&o, origin, b3)) return rc;
	if(int rc = hc.put(&d, dir, b3)) return rc;
	if(idir) { if(int rc = hc.put(&i, idir, b3)) return rc; }
	if(indices) { if(int rc = hc.put(&ix, indices, (size_t)n * 4)) return rc; }
	if(int rc = hc.put(&ds, dist, b1)) return rc;
	if(visits) {   // rays that are not listed keep what the caller's array holds
		if(int rc = hc.put(&vs, visits, 2 * b1)) return rc;
	}
	if(stats2) { if(int rc = hc.zeroStats()) return rc; }
	{
		SNAIL_LOCK(s);
		if(int rc = launchWide(s, nRays, (float *)o, (float *)d, (float *)i, (int32_t *)ix, nIndices, (float *)ds, startNode, (int32_t *)vs,
							   stats2 ? hc.stats() : nullptr, hc.stream()))
			return rc;
	}
	if(int rc = hc.get(dist, ds, b1)) return rc;
	if(int rc = hc.get(visits, vs, 2 * b1)) return rc;
	uint64_t hs[4] = {0, 0, 0, 0};
	if(int rc = hc.finish(stats2 ? hs : nullptr)) return rc;   // (the call's counter words are four; this header's are the first two)
	if(stats2) { stats2[0] += hs[0]; stats2[1] += hs[1]; }
	return 0;
}

int snail_photons_trace_dev(SnailScene *s, int nLights, int count, const float *origin, const float *dir, const float *lights7, SnailPhoton *photons,
							int32_t *nPhotons, uint64_t *dStats, void *stream) {
	const char *fn = "snail_photons_trace_dev";
	if(int rc = photonCheckArgs(fn, nLights, count, origin, dir, lights7, photons, nPhotons)) return rc;
	if(int rc = wideCheckScene(fn, s, 0)) return rc;
	DeviceGuard guard(s->device);
	if(nLights * count == 0) { HIP_TRY(hipMemsetAsync(nPhotons, 0, sizeof(int32_t), (hipStream_t)stream)); return 0; }
	SNAIL_LOCK(s);
	return launchPhotons(s, nLights, count, origin, dir, lights7, photons, nPhotons, dStats, (hipStream_t)stream);
}

int snail_photons_trace(SnailScene *s, int nLights, int count, const float *origin, const float *dir, const float *lights7, SnailPhoton *photons,
						int32_t *nPhotons, uint64_t *stats2) {
	const char *fn = "snail_photons_trace";
	if(int rc = photonCheckArgs(fn, nLights, count, origin, dir, lights7, photons, nPhotons)) return rc;
	if(int rc = wideCheckScene(fn, s, 0)) return rc;
	const int n = nLights * count;
	*nPhotons = 0;
	if(n == 0) return 0;
	DeviceGuard guard(s->device);
	HostCallScope hc(s, fn);
	if(hc.rc) return hc.rc;
	typedef HostCallScope H;
	const size_t b3 = (size_t)n * 12;
	if(int rc = hc.reserve(2 * H::pad(b3) + H::pad((size_t)n * sizeof(SnailPhoton)) + H::pad(sizeof(int32_t)))) return rc;
	void *o = nullptr, *d = nullptr, *ph = nullptr, *np = nullptr;
	if(int rc = hc.put(&o, origin, b3)) return rc;
	if(int rc = hc.put(&d, dir, b3)) return rc;
	if(int rc = hc.put(&ph, nullptr, (size_t)n * sizeof(SnailPhoton))) return rc;
	if(int rc = hc.put(&np, nullptr, sizeof(int32_t))) return rc;
	if(stats2) { if(int rc = hc.zeroStats()) return rc; }
	{
		SNAIL_LOCK(s);
		if(int rc = launchPhotons(s, nLights, count, (float *)o, (float *)d, lights7, (SnailPhoton *)ph, (int32_t *)np, stats2 ? hc.stats() : nullptr, hc.stream()))
			return rc;
	}
	int32_t got = 0;
	if(int rc = hc.get(&got, np, sizeof(got))) return rc;
	HIP_TRY(hipStreamSynchronize(hc.stream()));   // the count decides how many records come back
	if(got < 0 || got > n) { snail_set_error("%s: the device reported %d photons of %d rays", fn, got, n); return 1; }
	if(int rc = hc.get(photons, ph, (size_t)got * sizeof(SnailPhoton))) return rc;
	uint64_t hs[4] = {0, 0, 0, 0};
	if(int rc = hc.finish(stats2 ? hs : nullptr)) return rc;
	*nPhotons = got;
	if(stats2) { stats2[0] += hs[0]; stats2[1] += hs[1]; }
	return 0;
}

} // extern "C"
