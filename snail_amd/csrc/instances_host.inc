// instances_host.inc -- host side of the two-level instanced scenes (include/snail_instances.h); included at
// the end of snail_hip.hip.  The build is in dbvh_build.cpp, the kernels in instances.inc.

struct SnailInstances {
	int device = 0;
	std::vector<SnailScene *> blas;
	dev::InstBlas *dBlas = nullptr;
	uint4 *dTop = nullptr, *dInst = nullptr;   // top-level node records; 4 x 16 B per builder slot
	int topCap = 0, instCap = 0;
	int nNodes = 0, n = 0;
	// snail_instances_rebuild_dev (instances_build.inc): the BLAS root boxes (nBlas x 6 floats, from the BLAS scenes' root nodes at create), the
	// builder's scratch (one allocation, sized by the largest n so far) and {nNodes, n} of the tree the buffers hold, which only the device
	// knows once a rebuild has been enqueued (curOnDevice; a rebuild that fails leaves the previous values)
	float *dBlasBox = nullptr;
	char *buildBase = nullptr;
	int buildCap = 0;
	int *dCur = nullptr;
	bool curOnDevice = false;
	// mu: the ordering state below and the buffers' identity (held while a call enqueues)
	std::mutex mu;
	// snail_instances_update vs launches: the update's stream waits for every launch enqueued since the previous update (one event per stream
	// that launched), its copies come from pinned staging (reused once the previous update's copies are done), and every launch after it
	// waits for `ready`
	hipEvent_t ready = nullptr;
	bool hasReady = false;
	struct Use { hipStream_t stream; hipEvent_t ev; };
	std::vector<Use> uses;
	void *staging = nullptr;
	size_t stagingCap = 0;
	hipEvent_t stagingFree = nullptr;
	bool stagingUsed = false;
	// intermediates of snail_instances_render_whitted*_dev (hits, shadow distances, mirrored packets and colours), one set per launch in flight:
	// handed out round-robin, a recycled set's next user waits for the event recorded after its previous user's last kernel
	struct ShadeBufs {
		float *hitT = nullptr; int *hitInst = nullptr, *hitTri = nullptr;
		float *sDist = nullptr;
		float *rOrg = nullptr, *rDir = nullptr, *rIDir = nullptr, *rDist = nullptr, *rCol = nullptr;
		float *col = nullptr; int32_t *xy2 = nullptr;   // snail_instances_tiles.h: the packets' float colours, the double-resolution packet list
		uint32_t *pstats = nullptr;                     // snail_heatmap.h: the launch's per-packet TreeStats [packets][4] when the caller keeps none of its own
		int *rInst = nullptr, *rTri = nullptr;
		unsigned char *rMask = nullptr;
		static size_t bytes(size_t packets, int lights, bool refl, bool tiles = false) {
			const size_t rays = packets * 256;
			return rays * 12 + rays * 4 * (size_t)lights + (tiles ? rays * 12 + packets * 8 + 256 + packets * 16 + 256 : 0) + (refl ? rays * (36 + 12 + 12) + packets * 64 : 0) + 256;
		}
		void carve(char *base, size_t packets, int lights, bool refl, bool tiles = false) {
			const size_t rays = packets * 256;
			if(tiles) { // (first: 16-byte aligned whatever follows)
				col = (float *)base; base += rays * 12;
				xy2 = (int32_t *)base; base += (packets * 8 + 255) & ~(size_t)255;
				pstats = (uint32_t *)base; base += (packets * 16 + 255) & ~(size_t)255;
			}
			hitT = (float *)base; base += rays * 4;
			hitInst = (int *)base; base += rays * 4;
			hitTri = (int *)base; base += rays * 4;
			sDist = (float *)base; base += rays * 4 * (size_t)lights;
			if(!refl) return;
			rOrg = (float *)base; base += rays * 12;
			rDir = (float *)base; base += rays * 12;
			rIDir = (float *)base; base += rays * 12;
			rDist = (float *)base; base += rays * 4;
			rInst = (int *)base; base += rays * 4;
			rTri = (int *)base; base += rays * 4;
			rCol = (float *)base; base += rays * 12;
			rMask = (unsigned char *)base;
		}
	};
	enum { kShadeSets = 8 };
	struct ShadeSet {
		ShadeBufs b;
		char *base = nullptr;
		size_t packets = 0;
		bool refl = false, tiles = false;
		hipEvent_t done = nullptr;
		bool used = false;
	} shade[kShadeSets];
	unsigned shadeCount = 0;
	// packet lists of whole frames (row-major over the 16x16 packet grid), by grid size; built once each
	FrameLists frameLists;
	// snail_instances_render_tiles: ONE cached tile job per handle, whose calls take turns
	std::mutex renderMu;
	InstTileJob *tileJob = nullptr;
};

namespace {

// children inside the array and after their parent, leaf ranges inside [0, n), depth <= 64 over the nodes reached from the root
int validateInstances(const char *fn, const void *nodes32, int nNodes, const float *xf12, const int32_t *blasIdx, int n, int nBlas, int *depthOut) {
	if(!nodes32 || !xf12 || !blasIdx || nNodes <= 0 || n <= 0 || nNodes > (1 << 30) || n > (1 << 30)) { snail_set_error("%s: bad arguments", fn); return 1; }
	for(size_t i = 0; i < (size_t)n * 12; i++)
		if(!std::isfinite(xf12[i])) { snail_set_error("%s: instance slot %d has a non-finite transform", fn, (int)(i / 12)); return 1; }
	for(int i = 0; i < n; i++)
		if(blasIdx[i] < 0 || blasIdx[i] >= nBlas) { snail_set_error("%s: instance slot %d names BLAS %d of %d", fn, i, blasIdx[i], nBlas); return 1; }
	struct N { float b[6]; uint32_t sub; int32_t aux; };
	const N *nd = (const N *)nodes32;
	std::vector<int> depth((size_t)nNodes, -1);
	std::vector<char> reached((size_t)nNodes, 0);
	reached[0] = 1;
	for(int i = 0; i < nNodes; i++) {
		if(!reached[i]) continue;
		if(nd[i].sub & 0x80000000u) {
			const long long first = nd[i].sub & 0x7fffffffu, count = nd[i].aux;
			if(count < 0 || first + count > n) { snail_set_error("%s: leaf %d holds instances %lld..%lld of %d", fn, i, first, first + count - 1, n); return 1; }
		} else {
			const long long sub = nd[i].sub;
			if(sub <= i || sub + 1 >= nNodes) { snail_set_error("%s: node %d has children %lld, %lld (must follow it, inside %d nodes)", fn, i, sub, sub + 1, nNodes); return 1; }
			reached[sub] = reached[sub + 1] = 1;
		}
	}
	int maxDepth = 0;
	for(int i = nNodes - 1; i >= 0; i--) {
		if(!reached[i]) continue;
		depth[i] = (nd[i].sub & 0x80000000u) ? 0 : 1 + std::max(depth[nd[i].sub], depth[nd[i].sub + 1]);
		if(depth[i] > SNAIL_INSTANCES_MAX_DEPTH) { snail_set_error("%s: the tree is deeper than %d levels (depth limit SNAIL_INSTANCES_MAX_DEPTH)", fn, SNAIL_INSTANCES_MAX_DEPTH); return 2; }
	}
	maxDepth = depth[0];
	if(depthOut) *depthOut = maxDepth;
	return 0;
}

void packInstances(const float *xf12, const int32_t *blasIdx, int n, uint32_t *out16) {
	for(int i = 0; i < n; i++) {
		uint32_t *o = out16 + (size_t)i * 16;
		memset(o, 0, 64);
		for(int r = 0; r < 3; r++) memcpy(o + r * 4, xf12 + (size_t)i * 12 + r * 3, 12);
		o[3] = (uint32_t)blasIdx[i];
		memcpy(o + 12, xf12 + (size_t)i * 12 + 9, 12);
	}
}

// new records into the handle's buffers, ordered on `stream` after every launch since the previous update (mu held)
int instancesUpload(SnailInstances *h, const void *nodes32, int nNodes, const float *xf12, const int32_t *blasIdx, int n, hipStream_t stream) {
	for(auto &u : h->uses) HIP_TRY(hipStreamWaitEvent(stream, u.ev, 0));
	if(h->curOnDevice && h->hasReady) HIP_TRY(hipStreamWaitEvent(stream, h->ready, 0));   // a device rebuild still writing the buffers
	h->curOnDevice = false;
	const size_t topBytes = (size_t)nNodes * 32, instBytes = (size_t)n * 64;
	if(nNodes > h->topCap || n > h->instCap) { // grown: the old buffers may still be read by launches in flight
		HIP_TRY(hipStreamSynchronize(stream));
		HIP_TRY(hipDeviceSynchronize());
		if(nNodes > h->topCap) {
			if(h->dTop) (void)hipFree(h->dTop);
			h->dTop = nullptr; h->topCap = 0;
			HIP_TRY(hipMalloc((void **)&h->dTop, topBytes));
			h->topCap = nNodes;
		}
		if(n > h->instCap) {
			if(h->dInst) (void)hipFree(h->dInst);
			h->dInst = nullptr; h->instCap = 0;
			HIP_TRY(hipMalloc((void **)&h->dInst, instBytes));
			h->instCap = n;
		}
	}
	if(h->stagingUsed) HIP_TRY(hipEventSynchronize(h->stagingFree));   // the previous update's copies out of the staging area
	if(topBytes + instBytes > h->stagingCap) {
		if(h->staging) (void)hipHostFree(h->staging);
		h->staging = nullptr; h->stagingCap = 0;
		HIP_TRY(hipHostMalloc(&h->staging, topBytes + instBytes, hipHostMallocDefault));
		h->stagingCap = topBytes + instBytes;
	}
	char *st = (char *)h->staging;
	memcpy(st, nodes32, topBytes);
	packInstances(xf12, blasIdx, n, (uint32_t *)(st + topBytes));
	HIP_TRY(hipMemcpyAsync(h->dTop, st, topBytes, hipMemcpyHostToDevice, stream));
	HIP_TRY(hipMemcpyAsync(h->dInst, st + topBytes, instBytes, hipMemcpyHostToDevice, stream));
	if(!h->stagingFree) HIP_TRY(hipEventCreateWithFlags(&h->stagingFree, hipEventDisableTiming));
	HIP_TRY(hipEventRecord(h->stagingFree, stream));
	h->stagingUsed = true;
	if(!h->ready) HIP_TRY(hipEventCreateWithFlags(&h->ready, hipEventDisableTiming));
	HIP_TRY(hipEventRecord(h->ready, stream));
	h->hasReady = true;
	h->nNodes = nNodes; h->n = n;
	return 0;
}

// the launch's argument record (arithmetic and tree flavour of the BLASes) and its ordering against updates (mu held)
int instancesBegin(SnailInstances *h, const char *fn, dev::InstArgs &A, bool *sse, bool *deep, hipStream_t stream) {
	memset(&A, 0, sizeof(A));
	const int arith = h->blas[0]->arith;
	*deep = false;
	for(SnailScene *s : h->blas) {
		if(s->arith != arith) { snail_set_error("%s: the BLAS scenes are set to different arithmetics", fn); return 1; }
		*deep = *deep || useDeep(s);
	}
	*sse = arith == SNAIL_ARITH_HOST_SSE;
	A.hostTab = *sse ? h->blas[0]->dTab : nullptr;
	if(*sse) {
		for(SnailScene *s : h->blas)
			if(s->dTab != h->blas[0]->dTab && s->tabGen != h->blas[0]->tabGen) { snail_set_error("%s: the BLAS scenes hold different rcpps / rsqrtps tables", fn); return 1; }
	}
	A.top = h->dTop; A.inst = h->dInst; A.blas = h->dBlas;
	if(h->hasReady) HIP_TRY(hipStreamWaitEvent(stream, h->ready, 0));
	// a BLAS that is rebuilt on the device (snail_scene_rebuild_fast_dev): this launch reads its tree
	for(SnailScene *s : h->blas)
		if(s->fast) { std::lock_guard<std::mutex> lock(s->mu); if(int rc = fastSceneBegin(s, stream)) return rc; }
	return 0;
}
int instancesEnd(SnailInstances *h, hipStream_t stream) {
	HIP_TRY(hipGetLastError());
	for(SnailScene *s : h->blas)
		if(s->fast) { std::lock_guard<std::mutex> lock(s->mu); fastSceneEnd(s, stream); }
	for(auto &u : h->uses)
		if(u.stream == stream) { HIP_TRY(hipEventRecord(u.ev, stream)); return 0; }
	SnailInstances::Use u;
	u.stream = stream;
	HIP_TRY(hipEventCreateWithFlags(&u.ev, hipEventDisableTiming));
	HIP_TRY(hipEventRecord(u.ev, stream));
	h->uses.push_back(u);
	return 0;
}

int checkInstances(const SnailInstances *h, const char *fn) {
	if(!h || !h->dTop || !h->dInst || !h->dBlas || h->blas.empty()) { snail_set_error("%s: invalid instances handle", fn); return 1; }
	return 0;
}

#define SNAIL_INST_LAUNCH(SSE, GRID, STREAM, A, ...) SNAIL_LAUNCH(SSE, InstArgs, GRID, dim3(64), 0, STREAM, A, __VA_ARGS__)

int instancesPrimary(SnailInstances *h, const char *fn, const float cam[13], int resx, int resy, int x0, int y0, int w, int hh, const int32_t *dPacketXY,
					 int nPackets, float *t, float *u, float *v, int32_t *inst, int32_t *tri, uint64_t *dStats, hipStream_t stream) {
	if(int rc = checkInstances(h, fn)) return rc;
	if(!cam || resx <= 0 || resy <= 0) { snail_set_error("%s: bad camera or resolution", fn); return 1; }
	dev::InstArgs A;
	bool sse, deep;
	DeviceGuard guard(h->device);
	std::lock_guard<std::mutex> lock(h->mu);
	if(int rc = instancesBegin(h, fn, A, &sse, &deep, stream)) return rc;
	A.g = makeGen(cam, resx, resy);
	A.resx = resx; A.resy = resy;
	if(dPacketXY) {
		if(nPackets <= 0) return 0;
		A.packetXY = (const int2 *)dPacketXY;
		A.nPackets = nPackets;
	} else {
		if((x0 & 15) || (y0 & 15) || w <= 0 || hh <= 0 || x0 < 0 || y0 < 0) { snail_set_error("%s: rect origin must be a non-negative multiple of 16 and the size positive", fn); return 1; }
		A.x0 = x0; A.y0 = y0; A.w = w; A.h = hh;
		A.pw = (w + 15) / 16;
		A.nPackets = A.pw * ((hh + 15) / 16);
	}
	A.t = t; A.u = u; A.v = v; A.instOut = inst; A.triOut = tri;
	A.stats = (dev::u64 *)dStats;
	if(deep) SNAIL_INST_LAUNCH(sse, dim3(A.nPackets), stream, A, k_inst_frame<true>);
	else SNAIL_INST_LAUNCH(sse, dim3(A.nPackets), stream, A, k_inst_frame<false>);
	return instancesEnd(h, stream);
}

template <bool SHARED, bool MASK>
void instancesRaysKernels(bool sse, bool deep, bool bary, const dev::InstArgs &A, hipStream_t stream) {
	const dim3 grid(A.nPackets);
	if(deep && bary) SNAIL_INST_LAUNCH(sse, grid, stream, A, k_inst_trace<SHARED, MASK, true, true>);
	else if(deep) SNAIL_INST_LAUNCH(sse, grid, stream, A, k_inst_trace<SHARED, MASK, true, false>);
	else if(bary) SNAIL_INST_LAUNCH(sse, grid, stream, A, k_inst_trace<SHARED, MASK, false, true>);
	else SNAIL_INST_LAUNCH(sse, grid, stream, A, k_inst_trace<SHARED, MASK, false, false>);
}

int instancesRays(SnailInstances *h, const char *fn, bool shadow, int nPackets, int size, int sharedOrigin, const float *origin, const float *dir, const float *idir,
				  const uint8_t *mask, float *distance, int32_t *object, int32_t *element, float *bary, uint64_t *dStats, hipStream_t stream) {
	if(int rc = checkInstances(h, fn)) return rc;
	if(nPackets <= 0) return 0;
	if(size < 1 || size > SNAIL_PACKET_QUADS) { snail_set_error("%s: packet size %d outside 1..%d quads", fn, size, SNAIL_PACKET_QUADS); return 1; }
	if(!origin || !dir || !idir || !distance || (!shadow && (!object || !element))) { snail_set_error("%s: null ray array", fn); return 1; }
	dev::InstArgs A;
	bool sse, deep;
	DeviceGuard guard(h->device);
	std::lock_guard<std::mutex> lock(h->mu);
	if(int rc = instancesBegin(h, fn, A, &sse, &deep, stream)) return rc;
	A.nPackets = nPackets; A.size = size;
	A.origin = origin; A.dir = dir; A.idir = idir; A.mask = mask;
	A.distance = distance; A.object = object; A.element = element; A.bary = bary;
	A.stats = (dev::u64 *)dStats;
	if(shadow) {
		if(deep) SNAIL_INST_LAUNCH(sse, dim3(nPackets), stream, A, k_inst_occl<true>);
		else SNAIL_INST_LAUNCH(sse, dim3(nPackets), stream, A, k_inst_occl<false>);
	} else if(sharedOrigin && mask) instancesRaysKernels<true, true>(sse, deep, bary != nullptr, A, stream);
	else if(sharedOrigin) instancesRaysKernels<true, false>(sse, deep, bary != nullptr, A, stream);
	else if(mask) instancesRaysKernels<false, true>(sse, deep, bary != nullptr, A, stream);
	else instancesRaysKernels<false, false>(sse, deep, bary != nullptr, A, stream);
	return instancesEnd(h, stream);
}


// the whole frame's packets, row-major over the packet grid, through the call's own stream and arena (snail_instances_trace_frame_packets /
// snail_instances_render_depth): -> device t (and, if asked for, u, v, instance, triId), packet-major
static int instancesFramePackets(SnailInstances *h, const char *fn, HostCallScope &hc, const float cam[13], int resx, int resy, bool all, void **dXY,
								 float **dT, float **dU, float **dV, int32_t **dI, int32_t **dTri, int *nPackets) {
	if(!cam || resx <= 0 || resy <= 0) { snail_set_error("%s: bad camera or resolution", fn); return 1; }
	const int pw = (resx + 15) / 16, ph = (resy + 15) / 16, np = pw * ph;
	const std::vector<int32_t> xy = frameGrid(pw, ph);
	typedef HostCallScope H;
	const size_t rays = (size_t)np * 256;
	if(int rc = hc.reserve(H::pad(xy.size() * 4) + (all ? 5 : 1) * H::pad(rays * 4) + H::pad(rays * 3))) return rc;
	if(int rc = hc.put(dXY, xy.data(), xy.size() * 4)) return rc;
	*dT = (float *)hc.carve(rays * 4);
	*dU = *dV = nullptr; *dI = *dTri = nullptr;
	if(all) { *dU = (float *)hc.carve(rays * 4); *dV = (float *)hc.carve(rays * 4); *dI = (int32_t *)hc.carve(rays * 4); *dTri = (int32_t *)hc.carve(rays * 4); }
	*nPackets = np;
	return instancesPrimary(h, fn, cam, resx, resy, 0, 0, 0, 0, (const int32_t *)*dXY, np, *dT, *dU, *dV, *dI, *dTri, hc.stats(), hc.stream());
}

// ---- Scene<DBVH>::RayTrace, simple-shading configuration (instances_shade.inc) ----
int checkShadeArgs(const char *fn, const float cam[13], int resx, int resy, const float *lights7, int nLights, const float ambient[3], const float color[3]) {
	if(!cam || resx <= 0 || resy <= 0 || nLights < 0 || nLights > SNAIL_MAX_LIGHTS || (nLights && !lights7) || !ambient || !color) {
		snail_set_error("%s: bad arguments (camera, resolution, at most %d lights, ambient, color)", fn, SNAIL_MAX_LIGHTS);
		return 1;
	}
	return 0;
}

#define SNAIL_INST_SHADE_LAUNCH(SSE, GRID, STREAM, A, ...) SNAIL_LAUNCH(SSE, InstShadeArgs, GRID, dim3(64), 0, STREAM, A, __VA_ARGS__)

// the stages of one lit frame over the packet list dXY into `frame` (or packet-major `bgrPackets`), intermediates in W; mu held
int instancesShade(SnailInstances *h, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights,
				   const float ambient[3], const float color[3], bool refl, uint8_t *frame, int pitch, uint8_t *bgrPackets, const SnailInstances::ShadeBufs &W,
				   uint64_t *dStats, hipStream_t st, float *colPackets = nullptr, uint32_t *pstats = nullptr) {
	// pstats (a heat-map launch, heatmap_host.inc): every walking stage also books its counters per packet there (cleared by the caller) and the stages that
	// only make colours -- k_inst_final<.., DST_COLOR / DST_FRAME> -- are left out: the caller stores the counters' colours instead
	dev::InstArgs I;
	bool sse, deep;
	if(int rc = instancesBegin(h, fn, I, &sse, &deep, st)) return rc;
	const dim3 grid(np);
	// primary hits
	dev::InstArgs P = I;
	P.g = makeGen(cam, resx, resy);
	P.resx = resx; P.resy = resy;
	P.packetXY = (const int2 *)dXY; P.nPackets = np;
	P.t = W.hitT; P.instOut = W.hitInst; P.triOut = W.hitTri;
	P.stats = (dev::u64 *)dStats;
	P.pstats = pstats;
	if(deep) SNAIL_INST_LAUNCH(sse, grid, st, P, k_inst_frame<true>);
	else SNAIL_INST_LAUNCH(sse, grid, st, P, k_inst_frame<false>);

	dev::InstShadeArgs A;
	memset(&A, 0, sizeof(A));
	A.i = I;
	A.s.hostTab = I.hostTab;
	A.s.g = P.g;
	A.s.resx = resx; A.s.resy = resy; A.s.pw = (resx + 15) / 16; A.s.ph = (resy + 15) / 16;
	A.s.packetXY = (const int2 *)dXY; A.s.nPackets = np; A.s.nBlocks = np;
	A.s.bgrPackets = bgrPackets; A.s.frame = frame; A.s.pitch = pitch;
	A.s.colPackets = colPackets;   // the float colours k_inst_store goes on from, instead of bytes
	A.s.nLights = nLights;
	for(int n = 0; n < nLights; n++) for(int k = 0; k < 7; k++) A.s.lights[n][k] = lights7[n * 7 + k];
	for(int c = 0; c < 3; c++) { A.s.ambient[c] = ambient[c]; A.s.color[c] = color[c]; }
	A.s.hitT = W.hitT; A.s.hitId = W.hitTri; A.hitInst = W.hitInst;
	A.s.rOrg = W.rOrg; A.s.rDir = W.rDir; A.s.rIDir = W.rIDir; A.s.rMask = W.rMask; A.s.rDist = W.rDist; A.s.rObj = W.rTri; A.rInst = W.rInst; A.s.rCol = W.rCol;
	A.s.sDist = W.sDist;
	A.s.blend = refl ? 1 : 0;
	A.s.stats = (dev::u64 *)dStats;
	A.s.pstats = pstats;
	const dim3 lgrid(np, nLights > 0 ? nLights : 1);
	if(refl) { // the nested RayTrace of the mirrored packets
		SNAIL_INST_SHADE_LAUNCH(sse, grid, st, A, k_inst_final<dev::SRC_PRIMARY, dev::DST_MIRROR>);
		dev::InstArgs R = I;
		R.nPackets = np; R.size = 64;
		R.origin = W.rOrg; R.dir = W.rDir; R.idir = W.rIDir; R.mask = W.rMask;
		R.distance = W.rDist; R.object = W.rInst; R.element = W.rTri;
		R.stats = (dev::u64 *)dStats;
		R.pstats = pstats;
		if(pstats) {
			if(deep) SNAIL_INST_LAUNCH(sse, grid, st, R, k_inst_trace<false, true, true, false, true>);
			else SNAIL_INST_LAUNCH(sse, grid, st, R, k_inst_trace<false, true, false, false, true>);
		} else if(deep) SNAIL_INST_LAUNCH(sse, grid, st, R, k_inst_trace<false, true, true, false>);
		else SNAIL_INST_LAUNCH(sse, grid, st, R, k_inst_trace<false, true, false, false>);
		if(nLights && pstats) {
			if(deep) SNAIL_INST_SHADE_LAUNCH(sse, lgrid, st, A, k_inst_light<true, dev::SRC_MIRROR, true>);
			else SNAIL_INST_SHADE_LAUNCH(sse, lgrid, st, A, k_inst_light<false, dev::SRC_MIRROR, true>);
		} else if(nLights) {
			if(deep) SNAIL_INST_SHADE_LAUNCH(sse, lgrid, st, A, k_inst_light<true, dev::SRC_MIRROR>);
			else SNAIL_INST_SHADE_LAUNCH(sse, lgrid, st, A, k_inst_light<false, dev::SRC_MIRROR>);
		}
		if(!pstats) SNAIL_INST_SHADE_LAUNCH(sse, grid, st, A, k_inst_final<dev::SRC_MIRROR, dev::DST_COLOR>);
	}
	if(nLights && pstats) {
		if(deep) SNAIL_INST_SHADE_LAUNCH(sse, lgrid, st, A, k_inst_light<true, dev::SRC_PRIMARY, true>);
		else SNAIL_INST_SHADE_LAUNCH(sse, lgrid, st, A, k_inst_light<false, dev::SRC_PRIMARY, true>);
	} else if(nLights) {
		if(deep) SNAIL_INST_SHADE_LAUNCH(sse, lgrid, st, A, k_inst_light<true, dev::SRC_PRIMARY>);
		else SNAIL_INST_SHADE_LAUNCH(sse, lgrid, st, A, k_inst_light<false, dev::SRC_PRIMARY>);
	}
	if(!pstats) SNAIL_INST_SHADE_LAUNCH(sse, grid, st, A, k_inst_final<dev::SRC_PRIMARY, dev::DST_FRAME>);
	return instancesEnd(h, st);
}

// the next set of intermediates of the handle, grown if need be, its previous user's last kernel waited for on `st` (mu held).  tiles: with the
// float colours and the double-resolution packet list of snail_instances_tiles.h
int instancesNextSet(SnailInstances *h, size_t np, bool refl, bool tiles, hipStream_t st, SnailInstances::ShadeSet **out) {
	SnailInstances::ShadeSet &W = h->shade[h->shadeCount++ % SnailInstances::kShadeSets];
	if(!W.base || W.packets < np || (refl && !W.refl) || (tiles && !W.tiles)) { // grown (shadow distances sized for SNAIL_MAX_LIGHTS once): its previous user may still be running
		HIP_TRY(hipDeviceSynchronize());
		if(W.base) (void)hipFree(W.base);
		const size_t packets = std::max(W.packets, np);
		const bool r = refl || W.refl, t = tiles || W.tiles;
		W.base = nullptr; W.packets = 0; W.refl = W.tiles = false; W.used = false;
		HIP_TRY(hipMalloc((void **)&W.base, SnailInstances::ShadeBufs::bytes(packets, SNAIL_MAX_LIGHTS, r, t)));
		W.packets = packets; W.refl = r; W.tiles = t;
	}
	if(!W.done) HIP_TRY(hipEventCreateWithFlags(&W.done, hipEventDisableTiming));
	if(W.used) HIP_TRY(hipStreamWaitEvent(st, W.done, 0));
	*out = &W;
	return 0;
}

// snail_instances_render_whitted_dev / _packets_dev (mu held)
int instancesShadeDev(SnailInstances *h, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights,
					  const float ambient[3], const float color[3], int flags, uint8_t *frame, int pitch, uint8_t *bgrPackets, uint64_t *dStats, hipStream_t st) {
	const bool refl = (flags & SNAIL_WHITTED_REFLECTIONS) != 0;
	if(!dXY) { if(int rc = h->frameLists.get(resx, resy, &dXY, &np)) return rc; }
	SnailInstances::ShadeSet *Wp = nullptr;
	if(int rc = instancesNextSet(h, (size_t)np, refl, false, st, &Wp)) return rc;
	SnailInstances::ShadeSet &W = *Wp;
	W.b = SnailInstances::ShadeBufs();
	W.b.carve(W.base, (size_t)np, nLights, refl);
	if(int rc = instancesShade(h, fn, cam, resx, resy, dXY, np, lights7, nLights, ambient, color, refl, frame, pitch, bgrPackets, W.b, dStats, st)) return rc;
	HIP_TRY(hipEventRecord(W.done, st));
	W.used = true;
	return 0;
}
} // namespace

extern "C" {

SnailInstances *snail_instances_create(SnailScene *const *blas, int nBlas, const void *nodes32, int nNodes, const float *xf12, const int32_t *blasIdx,
									   int n, int depth) {
	const char *fn = "snail_instances_create";
	if(!blas || nBlas <= 0) { snail_set_error("%s: no BLAS scenes", fn); return nullptr; }
	int measured = 0;
	if(validateInstances(fn, nodes32, nNodes, xf12, blasIdx, n, nBlas, &measured)) return nullptr;
	for(int b = 0; b < nBlas; b++) {
		if(checkScene(blas[b], fn)) return nullptr;
		if(blas[b]->device != blas[0]->device) { snail_set_error("%s: BLAS %d lives on device %d, BLAS 0 on device %d", fn, b, blas[b]->device, blas[0]->device); return nullptr; }
	}
	(void)depth;   // (the depth that matters -- the stack the kernels need -- is measured above)
	DeviceGuard guard(blas[0]->device);
	if(!guard.ok) { snail_set_error("%s: cannot select device %d", fn, blas[0]->device); return nullptr; }
	SnailInstances *h = new SnailInstances();
	h->device = blas[0]->device;
	h->blas.assign(blas, blas + nBlas);
	std::vector<dev::InstBlas> rec((size_t)nBlas);
	for(int b = 0; b < nBlas; b++) { rec[b].nodes = blas[b]->dNodes; rec[b].tris = blas[b]->dTris; }
	hipError_t e = hipMalloc((void **)&h->dBlas, rec.size() * sizeof(dev::InstBlas));
	if(e == hipSuccess) e = hipMemcpy(h->dBlas, rec.data(), rec.size() * sizeof(dev::InstBlas), hipMemcpyHostToDevice);
	// the BLAS root boxes, for the device builder: each scene's own root node (what Scene.get_bbox returns)
	if(e == hipSuccess) e = hipMalloc((void **)&h->dBlasBox, (size_t)nBlas * 24);
	for(int b = 0; b < nBlas && e == hipSuccess; b++) e = hipMemcpy((char *)h->dBlasBox + (size_t)b * 24, blas[b]->dNodes, 24, hipMemcpyDeviceToDevice);
	if(e == hipSuccess) e = hipMalloc((void **)&h->dCur, 2 * sizeof(int));
	if(e != hipSuccess) { snail_set_error("%s: %s", fn, hipGetErrorString(e)); snail_instances_destroy(h); return nullptr; }
	int rc;
	{
		std::lock_guard<std::mutex> lock(h->mu);
		rc = instancesUpload(h, nodes32, nNodes, xf12, blasIdx, n, nullptr);
	}
	if(rc == 0 && hipStreamSynchronize(nullptr) != hipSuccess) { snail_set_error("%s: upload failed", fn); rc = 1; }
	if(rc) { snail_instances_destroy(h); return nullptr; }
	return h;
}

int snail_instances_update(SnailInstances *h, const void *nodes32, int nNodes, const float *xf12, const int32_t *blasIdx, int n, int depth, void *stream) {
	const char *fn = "snail_instances_update";
	if(int rc = checkInstances(h, fn)) return rc;
	if(int rc = validateInstances(fn, nodes32, nNodes, xf12, blasIdx, n, (int)h->blas.size(), nullptr)) return rc;
	(void)depth;
	DeviceGuard guard(h->device);
	std::lock_guard<std::mutex> lock(h->mu);
	return instancesUpload(h, nodes32, nNodes, xf12, blasIdx, n, (hipStream_t)stream);
}

void snail_instances_destroy(SnailInstances *h) {
	if(!h) return;
	DeviceGuard guard(h->device);
	(void)hipDeviceSynchronize();
	if(h->dBlas) (void)hipFree(h->dBlas);
	if(h->dTop) (void)hipFree(h->dTop);
	if(h->dInst) (void)hipFree(h->dInst);
	if(h->dBlasBox) (void)hipFree(h->dBlasBox);
	if(h->buildBase) (void)hipFree(h->buildBase);
	if(h->dCur) (void)hipFree(h->dCur);
	if(h->staging) (void)hipHostFree(h->staging);
	if(h->ready) (void)hipEventDestroy(h->ready);
	if(h->stagingFree) (void)hipEventDestroy(h->stagingFree);
	for(auto &u : h->uses) (void)hipEventDestroy(u.ev);
	for(auto &w : h->shade) {
		if(w.base) (void)hipFree(w.base);
		if(w.done) (void)hipEventDestroy(w.done);
	}
	h->frameLists.release();
	freeInstTileJob(h->tileJob);
	delete h;
}

int snail_instances_trace_primary_dev(SnailInstances *h, const float cam[13], int resx, int resy, int x0, int y0, int w, int hh, float *t, float *u, float *v,
									  int32_t *inst, int32_t *tri, uint64_t *dStats, void *stream) {
	return instancesPrimary(h, "snail_instances_trace_primary_dev", cam, resx, resy, x0, y0, w, hh, nullptr, 0, t, u, v, inst, tri, dStats, (hipStream_t)stream);
}

int snail_instances_trace_packets_dev(SnailInstances *h, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets, float *t, float *u,
									  float *v, int32_t *inst, int32_t *tri, uint64_t *dStats, void *stream) {
	if(!dPacketXY) { snail_set_error("snail_instances_trace_packets_dev: null packet list"); return 1; }
	return instancesPrimary(h, "snail_instances_trace_packets_dev", cam, resx, resy, 0, 0, 0, 0, dPacketXY, nPackets, t, u, v, inst, tri, dStats, (hipStream_t)stream);
}

int snail_instances_trace_rays_dev(SnailInstances *h, int nPackets, int size, int sharedOrigin, const float *origin, const float *dir, const float *idir,
								   const uint8_t *mask, float *distance, int32_t *object, int32_t *element, float *bary, uint64_t *dStats, void *stream) {
	return instancesRays(h, "snail_instances_trace_rays_dev", false, nPackets, size, sharedOrigin, origin, dir, idir, mask, distance, object, element, bary,
						 dStats, (hipStream_t)stream);
}

int snail_instances_trace_shadow_dev(SnailInstances *h, int nPackets, int size, const float *origin3, const float *dir, const float *idir, float *distance,
									 uint64_t *dStats, void *stream) {
	return instancesRays(h, "snail_instances_trace_shadow_dev", true, nPackets, size, 1, origin3, dir, idir, nullptr, distance, nullptr, nullptr, nullptr,
						 dStats, (hipStream_t)stream);
}

int snail_instances_trace_rays(SnailInstances *h, int nPackets, int size, int sharedOrigin, const float *origin, const float *dir, const float *idir,
							   const uint8_t *mask, float *distance, int32_t *object, int32_t *element, float *bary, uint64_t stats[4]) {
	const char *fn = "snail_instances_trace_rays";
	if(int rc = checkInstances(h, fn)) return rc;
	if(nPackets <= 0) return 0;
	if(size < 1 || size > SNAIL_PACKET_QUADS) { snail_set_error("%s: packet size %d outside 1..%d quads", fn, size, SNAIL_PACKET_QUADS); return 1; }
	if(!origin || !dir || !idir || !distance || !object || !element) { snail_set_error("%s: null ray array", fn); return 1; }
	DeviceGuard guard(h->device);
	HostCallScope hc(h->blas[0], fn);   // (a stream, counters and staging arena of the call's own; the BLAS handle only lends its free list)
	if(hc.rc) return hc.rc;
	const size_t nq = (size_t)nPackets * size;
	const size_t nOrg = (sharedOrigin ? (size_t)nPackets : nq) * 48;
	typedef HostCallScope H;
	if(int rc = hc.reserve(H::pad(nOrg) + 2 * H::pad(nq * 48) + H::pad(nq) + 3 * H::pad(nq * 16) + H::pad(nq * 32))) return rc;
	void *o = nullptr, *d = nullptr, *i = nullptr, *m = nullptr, *ds = nullptr, *ob = nullptr, *el = nullptr, *ba = nullptr;
	if(int rc = hc.put(&o, origin, nOrg)) return rc;
	if(int rc = hc.put(&d, dir, nq * 48)) return rc;
	if(int rc = hc.put(&i, idir, nq * 48)) return rc;
	if(mask) { if(int rc = hc.put(&m, mask, nq)) return rc; }
	if(int rc = hc.put(&ds, distance, nq * 16)) return rc;
	if(int rc = hc.put(&ob, object, nq * 16)) return rc;
	if(int rc = hc.put(&el, element, nq * 16)) return rc;
	if(bary) { if(int rc = hc.put(&ba, bary, nq * 32)) return rc; }
	if(stats) { if(int rc = hc.zeroStats()) return rc; }
	if(int rc = instancesRays(h, fn, false, nPackets, size, sharedOrigin, (float *)o, (float *)d, (float *)i, (uint8_t *)m, (float *)ds, (int32_t *)ob,
							  (int32_t *)el, (float *)ba, stats ? hc.stats() : nullptr, hc.stream()))
		return rc;
	if(int rc = hc.get(distance, ds, nq * 16)) return rc;
	if(int rc = hc.get(object, ob, nq * 16)) return rc;
	if(int rc = hc.get(element, el, nq * 16)) return rc;
	if(int rc = hc.get(bary, ba, nq * 32)) return rc;
	return hc.finish(stats);
}

int snail_instances_trace_shadow(SnailInstances *h, int nPackets, int size, const float *origin3, const float *dir, const float *idir, float *distance,
								 uint64_t stats[4]) {
	const char *fn = "snail_instances_trace_shadow";
	if(int rc = checkInstances(h, fn)) return rc;
	if(nPackets <= 0) return 0;
	if(size < 1 || size > SNAIL_PACKET_QUADS) { snail_set_error("%s: packet size %d outside 1..%d quads", fn, size, SNAIL_PACKET_QUADS); return 1; }
	if(!origin3 || !dir || !idir || !distance) { snail_set_error("%s: null ray array", fn); return 1; }
	DeviceGuard guard(h->device);
	HostCallScope hc(h->blas[0], fn);
	if(hc.rc) return hc.rc;
	const size_t nq = (size_t)nPackets * size;
	typedef HostCallScope H;
	if(int rc = hc.reserve(H::pad((size_t)nPackets * 12) + 2 * H::pad(nq * 48) + H::pad(nq * 16))) return rc;
	void *o = nullptr, *d = nullptr, *i = nullptr, *ds = nullptr;
	if(int rc = hc.put(&o, origin3, (size_t)nPackets * 12)) return rc;
	if(int rc = hc.put(&d, dir, nq * 48)) return rc;
	if(int rc = hc.put(&i, idir, nq * 48)) return rc;
	if(int rc = hc.put(&ds, distance, nq * 16)) return rc;
	if(stats) { if(int rc = hc.zeroStats()) return rc; }
	if(int rc = instancesRays(h, fn, true, nPackets, size, 1, (float *)o, (float *)d, (float *)i, nullptr, (float *)ds, nullptr, nullptr, nullptr,
							  stats ? hc.stats() : nullptr, hc.stream()))
		return rc;
	if(int rc = hc.get(distance, ds, nq * 16)) return rc;
	return hc.finish(stats);
}


int snail_instances_trace_frame_packets(SnailInstances *h, const float cam[13], int resx, int resy, float *t, float *u, float *v, int32_t *inst, int32_t *tri,
										uint64_t stats[4]) {
	const char *fn = "snail_instances_trace_frame_packets";
	if(int rc = checkInstances(h, fn)) return rc;
	if(!t || !u || !v || !inst || !tri) { snail_set_error("%s: null output", fn); return 1; }
	DeviceGuard guard(h->device);
	HostCallScope hc(h->blas[0], fn);
	if(hc.rc) return hc.rc;
	if(int rc = hc.zeroStats()) return rc;
	void *xy = nullptr; float *dT, *dU, *dV; int32_t *dI, *dTri; int np = 0;
	if(int rc = instancesFramePackets(h, fn, hc, cam, resx, resy, true, &xy, &dT, &dU, &dV, &dI, &dTri, &np)) return rc;
	const size_t bytes = (size_t)np * 256 * 4;
	if(int rc = hc.get(t, dT, bytes)) return rc;
	if(int rc = hc.get(u, dU, bytes)) return rc;
	if(int rc = hc.get(v, dV, bytes)) return rc;
	if(int rc = hc.get(inst, dI, bytes)) return rc;
	if(int rc = hc.get(tri, dTri, bytes)) return rc;
	return hc.finish(stats);
}

int snail_instances_render_depth(SnailInstances *h, const float cam[13], int resx, int resy, uint8_t *image, int pitch, uint64_t stats[4]) {
	const char *fn = "snail_instances_render_depth";
	if(int rc = checkInstances(h, fn)) return rc;
	if(!image || pitch < resx * 3) { snail_set_error("%s: bad image", fn); return 1; }
	DeviceGuard guard(h->device);
	HostCallScope hc(h->blas[0], fn);
	if(hc.rc) return hc.rc;
	if(int rc = hc.zeroStats()) return rc;
	void *xy = nullptr; float *dT, *dU, *dV; int32_t *dI, *dTri; int np = 0;
	if(int rc = instancesFramePackets(h, fn, hc, cam, resx, resy, false, &xy, &dT, &dU, &dV, &dI, &dTri, &np)) return rc;
	uint8_t *bgr = (uint8_t *)hc.carve((size_t)np * 256 * 3);
	if(int rc = snail_shade_depth_arith_dev(dT, np, bgr, h->blas[0]->arith, hc.stream())) return rc;
	// the image in device memory: a separate allocation of the call (frames are rare next to packets; freed once the copy is done)
	uint8_t *dImg = nullptr;
	HIP_TRY(hipMalloc((void **)&dImg, (size_t)pitch * resy));
	int rc = snail_packets_bgr_to_frame_dev((const int32_t *)xy, np, resx, resy, bgr, dImg, pitch, hc.stream());
	if(rc == 0 && hipMemcpy2DAsync(image, (size_t)pitch, dImg, (size_t)pitch, (size_t)resx * 3, (size_t)resy, hipMemcpyDeviceToHost, hc.stream()) != hipSuccess) {
		snail_set_error("%s: copy of the image failed", fn);
		rc = 1;
	}
	if(rc == 0) rc = hc.finish(stats);
	else (void)hipStreamSynchronize(hc.stream());
	(void)hipFree(dImg);
	return rc;
}

int snail_instances_render_whitted_dev(SnailInstances *h, const float cam[13], int resx, int resy, const float *lights7, int nLights, const float ambient[3],
									   const float color[3], int flags, uint8_t *frame, int pitch, uint64_t *dStats, void *stream) {
	const char *fn = "snail_instances_render_whitted_dev";
	if(int rc = checkInstances(h, fn)) return rc;
	if(int rc = checkShadeArgs(fn, cam, resx, resy, lights7, nLights, ambient, color)) return rc;
	if((flags & ~SNAIL_WHITTED_REFLECTIONS) || !frame || pitch < resx * 3) { snail_set_error("%s: bad frame, or flags other than SNAIL_WHITTED_REFLECTIONS", fn); return 1; }
	DeviceGuard guard(h->device);
	std::lock_guard<std::mutex> lock(h->mu);
	return instancesShadeDev(h, fn, cam, resx, resy, nullptr, 0, lights7, nLights, ambient, color, flags, frame, pitch, nullptr, dStats, (hipStream_t)stream);
}

int snail_instances_render_whitted_packets_dev(SnailInstances *h, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets,
											   const float *lights7, int nLights, const float ambient[3], const float color[3], int flags, uint8_t *bgrPackets,
											   uint64_t *dStats, void *stream) {
	const char *fn = "snail_instances_render_whitted_packets_dev";
	if(int rc = checkInstances(h, fn)) return rc;
	if(!dPacketXY && nPackets > 0) { snail_set_error("%s: null packet list", fn); return 1; }
	if(nPackets <= 0) return 0;
	if(int rc = checkShadeArgs(fn, cam, resx, resy, lights7, nLights, ambient, color)) return rc;
	if((flags & ~SNAIL_WHITTED_REFLECTIONS) || !bgrPackets || ((unsigned long long)bgrPackets & 3)) {
		snail_set_error("%s: null or unaligned output, or flags other than SNAIL_WHITTED_REFLECTIONS", fn);
		return 1;
	}
	DeviceGuard guard(h->device);
	std::lock_guard<std::mutex> lock(h->mu);
	return instancesShadeDev(h, fn, cam, resx, resy, dPacketXY, nPackets, lights7, nLights, ambient, color, flags, nullptr, 0, bgrPackets, dStats, (hipStream_t)stream);
}

int snail_instances_render_image(SnailInstances *h, const float cam[13], int resx, int resy, const float *lights7, int nLights, const float ambient[3],
								 const float color[3], int flags, uint8_t *image, int pitch, uint64_t stats[4]) {
	const char *fn = "snail_instances_render_image";
	if(int rc = checkInstances(h, fn)) return rc;
	if(flags & SNAIL_RENDER_AA4) { snail_set_error("%s: SNAIL_RENDER_AA4 is not available for instanced scenes", fn); return 1; }
	if(flags & ~(SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_DEPTH)) { snail_set_error("%s: unknown flags 0x%x", fn, flags); return 1; }
	if(!cam || resx <= 0 || resy <= 0 || !image || pitch < resx * 3) { snail_set_error("%s: bad camera, resolution or image", fn); return 1; }
	if(flags & SNAIL_RENDER_DEPTH) return snail_instances_render_depth(h, cam, resx, resy, image, pitch, stats);
	if(int rc = checkShadeArgs(fn, cam, resx, resy, lights7, nLights, ambient, color)) return rc;
	const bool refl = (flags & SNAIL_RENDER_REFLECTIONS) != 0;
	DeviceGuard guard(h->device);
	HostCallScope hc(h->blas[0], fn);
	if(hc.rc) return hc.rc;
	if(int rc = hc.zeroStats()) return rc;
	const int pw = (resx + 15) / 16, ph = (resy + 15) / 16, np = pw * ph;
	const std::vector<int32_t> xy = frameGrid(pw, ph);
	typedef HostCallScope H;
	const size_t imgBytes = (size_t)pitch * resy;
	if(int rc = hc.reserve(H::pad(xy.size() * 4) + H::pad(SnailInstances::ShadeBufs::bytes((size_t)np, nLights, refl)) + H::pad(imgBytes + 4))) return rc;
	void *dXY = nullptr;
	if(int rc = hc.put(&dXY, xy.data(), xy.size() * 4)) return rc;
	SnailInstances::ShadeBufs W;
	W.carve((char *)hc.carve(SnailInstances::ShadeBufs::bytes((size_t)np, nLights, refl)), (size_t)np, nLights, refl);
	uint8_t *dImg = (uint8_t *)hc.carve(imgBytes + 4);
	{
		std::lock_guard<std::mutex> lock(h->mu);
		if(int rc = instancesShade(h, fn, cam, resx, resy, (const int32_t *)dXY, np, lights7, nLights, ambient, color, refl, dImg, pitch, nullptr, W, hc.stats(), hc.stream()))
			return rc;
	}
	HIP_TRY(hipMemcpy2DAsync(image, (size_t)pitch, dImg, (size_t)pitch, (size_t)resx * 3, (size_t)resy, hipMemcpyDeviceToHost, hc.stream()));
	return hc.finish(stats);
}

} // extern "C"

// ---- snail_instances_build.h: DBVH::Construct on the device (kernels: instances_build.inc) ----
namespace {

// room for a tree over n instances in the handle's buffers -- their contents KEPT, a rebuild that fails must leave the previous tree --
// and in the builder's scratch (mu held).  Grown, never shrunk; growing waits for the device, as in instancesUpload
int buildReserve(SnailInstances *h, int n) {
	const int needTop = (int)(2LL * n - 1);
	if(needTop <= h->topCap && n <= h->instCap && n <= h->buildCap) return 0;
	HIP_TRY(hipDeviceSynchronize());
	if(needTop > h->topCap) {
		uint4 *p = nullptr;
		HIP_TRY(hipMalloc((void **)&p, (size_t)needTop * 32));
		if(hipMemcpy(p, h->dTop, (size_t)h->topCap * 32, hipMemcpyDeviceToDevice) != hipSuccess) { (void)hipFree(p); snail_set_error("snail_instances_rebuild_dev: copy of the nodes failed"); return 1; }
		(void)hipFree(h->dTop);
		h->dTop = p; h->topCap = needTop;
	}
	if(n > h->instCap) {
		uint4 *p = nullptr;
		HIP_TRY(hipMalloc((void **)&p, (size_t)n * 64));
		if(hipMemcpy(p, h->dInst, (size_t)h->instCap * 64, hipMemcpyDeviceToDevice) != hipSuccess) { (void)hipFree(p); snail_set_error("snail_instances_rebuild_dev: copy of the records failed"); return 1; }
		(void)hipFree(h->dInst);
		h->dInst = p; h->instCap = n;
	}
	if(n > h->buildCap) {
		if(h->buildBase) (void)hipFree(h->buildBase);
		h->buildBase = nullptr; h->buildCap = 0;
		const size_t bytes = buildScratchBytes(n);
		HIP_TRY(hipMalloc((void **)&h->buildBase, bytes));
		h->buildCap = n;
	}
	return 0;
}

// what snail_instances_rebuild_dev refuses before anything is enqueued (fn: the caller's name in the texts)
int instancesRebuildCheck(const char *fn, const SnailInstances *h, const float *d_xf12, int n) {
	if(n <= 0 || n > (1 << 30)) { snail_set_error("%s: %d instances (1 .. 1 << 30)", fn, n); return 1; }
	if(!d_xf12) { snail_set_error("%s: null transforms", fn); return 1; }
	if(int rc = checkInstances(h, fn)) return rc;
	if(!h->dBlasBox || !h->dCur) { snail_set_error("%s: invalid instances handle", fn); return 1; }
	return 0;
}

// snail_instances_rebuild_dev after its arguments were judged: the handle's mu held, its device current.  `held` (or null): BLAS scenes whose mu
// the CALLER holds already (snail_instances_materials_rebuild_all_dev, behind its BLAS rebuilds); every other BLAS scene's is taken here
int instancesRebuildLocked(SnailInstances *h, const float *d_xf12, const int32_t *d_blasIdx, int n, int32_t *d_perm, int32_t *d_info, hipStream_t st,
						   const std::vector<SnailScene *> *held) {
	if(int rc = buildReserve(h, n)) return rc;
	// after every launch enqueued since the previous update (they read the buffers the commit writes) and after the previous update or rebuild
	// itself (one scratch area per handle)
	for(auto &u : h->uses) HIP_TRY(hipStreamWaitEvent(st, u.ev, 0));
	if(h->hasReady) HIP_TRY(hipStreamWaitEvent(st, h->ready, 0));
	// the root box of a BLAS that can be rebuilt on the device (snail_scene_rebuild_fast_dev) is read again, after any rebuild enqueued so far
	for(size_t b = 0; b < h->blas.size(); b++) {
		SnailScene *s = h->blas[b];
		if(!s->fast) continue;
		std::unique_lock<std::mutex> blasLock(s->mu, std::defer_lock);
		if(!held || std::find(held->begin(), held->end(), s) == held->end()) blasLock.lock();
		if(int rc = fastSceneBegin(s, st)) return rc;
		HIP_TRY(hipMemcpyAsync((char *)h->dBlasBox + b * 24, s->dNodes, 24, hipMemcpyDeviceToDevice, st));
		fastSceneEnd(s, st);
	}
	devb::BuildArgs A;
	memset(&A, 0, sizeof(A));
	buildCarve(h->buildBase, h->buildCap, A);
	A.xf = d_xf12; A.blasIdx = d_blasIdx; A.n = n; A.maxDepth = devb::kMaxDepth; A.nBlas = (int)h->blas.size(); A.blasBox = h->dBlasBox;
	A.top = h->dTop; A.inst = h->dInst; A.cur = h->dCur; A.perm = d_perm; A.info = d_info;
	A.seed = h->curOnDevice ? 0 : 1; A.seedNodes = h->nNodes; A.seedN = h->n;
	const int perN = (n + 255) / 256;
	hipLaunchKernelGGL(devb::k_build_init, dim3(perN), dim3(256), 0, st, A);
	hipLaunchKernelGGL(devb::k_build_boxes, dim3(perN), dim3(256), 0, st, A);
	const devb::SplitArgs &SA = A;
	hipLaunchKernelGGL(devb::k_build_root<devb::SplitDbvh>, dim3(1), dim3(64), 0, st, SA);
	if(n > devb::kSmall) {
		// level L holds at most min(2^L, n / 65) nodes of more than 64 instances; how many it does hold only the device knows: sized for the
		// worst case (capped; the workgroups stride), the surplus leaves at once
		const int most = n / (devb::kSmall + 1) + 1;
		const int wide = 16;   // a level per launch up to here (2^16 x 65 instances before a balanced tree has such nodes deeper) ...
		for(int level = 0; level < wide; level++) {
			int grid = level < 10 ? (1 << level) : 1024;
			grid = std::min(grid, most);
			hipLaunchKernelGGL(devb::k_build_big<devb::SplitDbvh>, dim3(grid), dim3(256), 0, st, SA, level, level + 1);
		}
		hipLaunchKernelGGL(devb::k_build_big<devb::SplitDbvh>, dim3(1), dim3(256), 0, st, SA, wide, (int)devb::kLevels);   // ... the rest in one workgroup, level after level
	}
	if(n >= 2) hipLaunchKernelGGL(devb::k_build_small<devb::SplitDbvh>, dim3(std::min(n / 2 + 1, 4096)), dim3(64), 0, st, SA);
	hipLaunchKernelGGL(devb::k_build_scan, dim3(1), dim3(1024), 0, st, SA);
	hipLaunchKernelGGL(devb::k_build_commit, dim3(std::min((2 * (long long)n + 255) / 256, 2048LL)), dim3(256), 0, st, A);
	HIP_TRY(hipGetLastError());
	if(!h->ready) HIP_TRY(hipEventCreateWithFlags(&h->ready, hipEventDisableTiming));
	HIP_TRY(hipEventRecord(h->ready, st));
	h->hasReady = true;
	h->curOnDevice = true;
	return 0;
}

} // namespace

extern "C" {

int snail_instances_rebuild_dev(SnailInstances *h, const float *d_xf12, const int32_t *d_blasIdx, int n, int32_t *d_perm, int32_t *d_info, void *stream) {
	const char *fn = "snail_instances_rebuild_dev";
	if(int rc = instancesRebuildCheck(fn, h, d_xf12, n)) return rc;
	DeviceGuard guard(h->device);
	std::lock_guard<std::mutex> lock(h->mu);
	return instancesRebuildLocked(h, d_xf12, d_blasIdx, n, d_perm, d_info, (hipStream_t)stream, nullptr);
}

int snail_instances_read_tree(SnailInstances *h, void *nodes32, int nodeCap, int *nNodes, float *xf12_slots, int32_t *blasIdx_slots, int slotCap, int *n) {
	const char *fn = "snail_instances_read_tree";
	if(int rc = checkInstances(h, fn)) return rc;
	DeviceGuard guard(h->device);
	std::lock_guard<std::mutex> lock(h->mu);
	HIP_TRY(hipDeviceSynchronize());
	int cur[2] = {h->nNodes, h->n};
	if(h->curOnDevice) HIP_TRY(hipMemcpy(cur, h->dCur, sizeof(cur), hipMemcpyDeviceToHost));
	if(cur[0] <= 0 || cur[0] > h->topCap || cur[1] <= 0 || cur[1] > h->instCap) { snail_set_error("%s: the handle holds no tree", fn); return 1; }
	if(nNodes) *nNodes = cur[0];
	if(n) *n = cur[1];
	if(nodes32) {
		if(nodeCap < cur[0]) { snail_set_error("%s: room for %d nodes, the tree has %d", fn, nodeCap, cur[0]); return 1; }
		HIP_TRY(hipMemcpy(nodes32, h->dTop, (size_t)cur[0] * 32, hipMemcpyDeviceToHost));
	}
	if(xf12_slots || blasIdx_slots) {
		if(slotCap < cur[1]) { snail_set_error("%s: room for %d instances, the handle has %d", fn, slotCap, cur[1]); return 1; }
		std::vector<uint32_t> rec((size_t)cur[1] * 16);
		HIP_TRY(hipMemcpy(rec.data(), h->dInst, rec.size() * 4, hipMemcpyDeviceToHost));
		for(int i = 0; i < cur[1]; i++) {   // packInstances, backwards
			const uint32_t *o = rec.data() + (size_t)i * 16;
			if(xf12_slots) {
				for(int r = 0; r < 3; r++) memcpy(xf12_slots + (size_t)i * 12 + r * 3, o + r * 4, 12);
				memcpy(xf12_slots + (size_t)i * 12 + 9, o + 12, 12);
			}
			if(blasIdx_slots) blasIdx_slots[i] = (int32_t)o[3];
		}
	}
	return 0;
}

} // extern "C"
