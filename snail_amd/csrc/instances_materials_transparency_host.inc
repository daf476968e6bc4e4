// instances_materials_transparency_host.inc -- the C-ABI of include/snail_instances_materials_transparency.h: the creator that accepts the kinds which
// can select a transparent lane (one body with snail_instances_materials_create: imatCreate, instances_materials_host.inc), the query, the launches
// of instances_materials_transparency.inc on their own (k_imat_sample_transp / _rays) and of the scene-free generator (k_mat_continue / _rays,
// materials_transparency.inc), and the frames that run them level by level (shadeLevels, materials_levels_host.inc, without the
// bounce, beside imatShade: way down with k_imat_trace_level, truncation count, way back up with k_mat_blend_transp / k_imat_light_transp /
// k_mat_colour_transp and the primary k_imat_light / k_mat_final), with IMatLevels, what the level driver asks of an instanced scene.  These entry points take ANY set (checkIMatAny); the older ones refuse a set that answers the query with 1
// (checkIMat).  Included after instances_materials_bounce_host.inc and materials_transparency_host.inc, whose checkTranspFrameArgs and
// matAligned16 it calls.
#include "../../include/snail_instances_materials_transparency.h"

namespace {

#define SNAIL_ITRANSP_LAUNCH(SSE, GRID, STREAM, A, ...) SNAIL_LAUNCH(SSE, ITranspArgs, GRID, dim3(64), 0, STREAM, A, __VA_ARGS__)

// The instanced scene's kind of the level driver (materials_levels_host.inc); the handle's mu held.  Every launch is booked through
// instancesBegin / instancesEnd, so the frame is ordered against snail_instances_update and snail_instances_rebuild_dev as a walk is.  The sample
// and light stages take an ITranspArgs of the kind's own: its MatArgs is the frame's, copied into the scene-free stages' record whenever a level
// changes it.
struct IMatLevels : LevelsFrame {
	typedef SnailInstancesMaterials Handle;
	typedef SnailInstancesMaterials::Bufs Bufs;
	typedef SnailInstancesMaterials::BounceBufs BounceBufs;
	typedef SnailInstancesMaterials::Set Set;
	SnailInstancesMaterials *m;
	SnailInstances *h;
	dev::InstArgs I;
	dev::ITranspArgs S;
	IMatLevels(SnailInstancesMaterials *m_, const char *fn_, hipStream_t st_, uint32_t *pstats_, int np_, int nLights) : LevelsFrame(fn_, st_, pstats_, np_, nLights), m(m_), h(m_->inst) {}
	int begin() { return instancesBegin(h, fn, I, &sse, &deep, st); }
	// (the stages enqueued so far are booked as every launch of the handle is, whatever failed)
	int end() { return instancesEnd(h, st); }
	int primary(const float cam[13], int resx, int resy, const int32_t *dXY, const Bufs &W, uint64_t *dStats) {
		dev::InstArgs P = I;
		P.g = makeGen(cam, resx, resy);
		P.resx = resx; P.resy = resy;
		P.packetXY = (const int2 *)dXY; P.nPackets = np;
		P.t = W.hitT; P.u = W.hitU; P.v = W.hitV; P.instOut = W.hitInst; P.triOut = W.hitTri;
		P.stats = (dev::u64 *)dStats;
		P.pstats = pstats;   // (k_inst_frame books per packet whenever it is given the array)
		if(deep) SNAIL_INST_LAUNCH(sse, grid, st, P, k_inst_frame<true>);
		else SNAIL_INST_LAUNCH(sse, grid, st, P, k_inst_frame<false>);
		return launched("k_inst_frame");
	}
	dev::MatArgs &frameArgs(dev::TreeArgs &, const float cam[13], int resx, int resy, const int32_t *dXY, const Bufs &W) {
		memset(&S, 0, sizeof(S));
		imatFillArgs(m, S.a, I, cam, resx, resy, dXY, np);
		S.a.m.s.hitId = W.hitTri; S.a.hitInst = W.hitInst;
		return S.a.m;
	}
	// the object of the walk, of the generator and of the mirror stage is the instance slot, the sample stages' rObj the triIds
	static int *object(const BounceBufs &R) { return R.rInst; }
	void level(dev::TreeArgs &G, const BounceBufs &R, const int32_t *order, bool slotAsObject) {
		S.a.m.s.rObj = slotAsObject ? R.rInst : R.rTri;
		S.rInst = R.rInst;
		S.inOrder = order;
		G.t.m = S.a.m;
	}
	int walk(const BounceBufs &R, const int32_t *order, uint64_t *dStats) {
		// the walk leaves element and barycentrics of a lane without a hit as it found them: zeros, not what the buffers last held (rTri and bary
		// are neighbours: ONE memset, as imatNested's)
		const hipError_t e = hipMemsetAsync(R.rTri, 0, (size_t)np * 256 * 12, st);
		if(e != hipSuccess) return failed("clearing a level's hit records", e);
		dev::ILevelArgs V;
		memset(&V, 0, sizeof(V));
		V.i = I;
		V.i.nPackets = np; V.i.size = 64;
		V.i.origin = R.rOrg; V.i.dir = R.rDir; V.i.idir = R.rIDir; V.i.mask = R.rMask;
		V.i.distance = R.rDist; V.i.object = R.rInst; V.i.element = R.rTri; V.i.bary = R.bary;
		V.i.stats = (dev::u64 *)dStats;
		V.i.pstats = pstats;
		V.order = order;
		SNAIL_LEVELS_LAUNCH_DEEP(ILevelArgs, grid, V, k_imat_trace_level);
		return launched("k_imat_trace_level");
	}
	int samplePrimary(dev::TreeArgs &, float *opacity, unsigned char *sel) {
		S.opacity = opacity; S.sel = sel;
		SNAIL_ITRANSP_LAUNCH(sse, grid, st, S, k_imat_sample_transp);
		return launched("k_imat_sample_transp");
	}
	int sampleRays(dev::TreeArgs &, float *opacity, unsigned char *sel) {
		S.opacity = opacity; S.sel = sel;
		SNAIL_ITRANSP_LAUNCH(sse, grid, st, S, k_imat_sample_transp_rays);
		return launched("k_imat_sample_transp_rays");
	}
	int lightsBegin(dev::MatArgs &, int) { return 0; }   // (the instanced lights walk the BLASes' own records: no origin-relative copy is taken)
	int nestedLights(dev::TreeArgs &) {
		SNAIL_LEVELS_LAUNCH_DEEP(ITranspArgs, lgrid, S, k_imat_light_transp);
		return launched("k_imat_light_transp");
	}
	int lights(dev::TreeArgs &) {
		SNAIL_LEVELS_LAUNCH_DEEP(IMatArgs, lgrid, S.a, k_imat_light);
		return launched("k_imat_light");
	}
	// the handle's part of levelsStore and of the host calls
	static int nextSet(SnailInstancesMaterials *m, int np, int nLights, hipStream_t st, Set **out) { return imatNextSet(m, np, nLights, false, st, out); }
	static int setDone(Set &W, const char *fn, int rc, hipStream_t st) { return imatSetDone(W, fn, rc, st); }
	// (the hit distances of k_inst_frame alone)
	static int depthStore(SnailInstancesMaterials *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *, int,
						  const float ambient[3], int flags, const float *tint, uint8_t *bgrPackets, const InstTileJob *J, uint64_t *dStats, hipStream_t st) {
		const float white[3] = {1.0f, 1.0f, 1.0f};
		return instancesShadeStore(m->inst, fn, cam, resx, resy, dXY, np, nullptr, 0, ambient, white, flags & (SNAIL_RENDER_DEPTH | SNAIL_RENDER_AA4), tint, bgrPackets, J, dStats, st);
	}
	static SnailScene *scene(SnailInstancesMaterials *m) { return m->inst->blas[0]; }   // (the arithmetic and its tables are the BLAS scenes'; it lends a host call its free list)
	static std::mutex &mu(SnailInstancesMaterials *m) { return m->inst->mu; }
	static int frameList(SnailInstancesMaterials *m, int resx, int resy, const int32_t **dXY, int *np) { return imatFrameList(m, resx, resy, dXY, np); }
};

// _dev / _packets_dev (the handle's mu held): the next group of intermediates with its levels' part, grown if need be
int imatTranspDev(SnailInstancesMaterials *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights,
				  const float ambient[3], uint8_t *frame, int pitch, uint8_t *bgrPackets, int maxDepth, uint64_t *dTrunc, uint64_t *dStats, hipStream_t st) {
	if(!dXY) { if(int rc = imatFrameList(m, resx, resy, &dXY, &np)) return rc; }
	SnailInstancesMaterials::Set *Wp = nullptr;
	if(int rc = imatNextSet(m, np, nLights, false, st, &Wp)) return rc;
	SnailInstancesMaterials::Set &W = *Wp;
	const size_t want = levelsBytes<SnailInstancesMaterials::BounceBufs>((size_t)np, nLights, maxDepth, false);
	if(int rc = levelsGrow(W, W.transp, W.transpBytes, want, want)) return rc;
	SnailInstancesMaterials::Bufs B;
	B.carve(W.base, (size_t)np);
	const int rc = shadeLevels<IMatLevels>(m, fn, cam, resx, resy, dXY, np, lights7, nLights, ambient, frame, pitch, bgrPackets, nullptr, B, W.transp, maxDepth, false, dTrunc, dStats, st);
	return imatSetDone(W, fn, rc, st);
}

} // namespace

extern "C" {

SnailInstancesMaterials *snail_instances_materials_create_transparent(SnailInstances *h, const SnailBlasShading *perBlas, int nBlas, const SnailMaterial *mats,
																	  int nMats, const int32_t *opacityTexture, const SnailTexture *textures, int nTex) {
	return imatCreate("snail_instances_materials_create_transparent", true, h, perBlas, nBlas, mats, nMats, opacityTexture, textures, nTex);
}

int snail_instances_materials_can_select_transparent(const SnailInstancesMaterials *m) {
	if(!m) { snail_set_error("snail_instances_materials_can_select_transparent: invalid instanced material set handle"); return -1; }
	if(m->dyn && imatDynCheckFresh(m, "snail_instances_materials_can_select_transparent")) return -1;   // (include/snail_instances_materials_dynamic.h, "staleness")
	return m->canSelectTransparent ? 1 : 0;
}

int snail_instances_materials_shade_packets_transp_dev(SnailInstancesMaterials *m, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets,
													   const float *dT, const float *dU, const float *dV, const int32_t *dInst, const int32_t *dTriId, float *dSamples,
													   float *dOpacity, uint8_t *dSel, void *stream) {
	const char *fn = "snail_instances_materials_shade_packets_transp_dev";
	// the arguments first, the handle last: what is refused here needs no device
	if(nPackets <= 0) return 0;
	if(!cam || resx <= 0 || resy <= 0 || !dPacketXY || !dT || !dU || !dV || !dInst || !dTriId || !dSamples || !dOpacity || !dSel ||
	   !matAligned16({dT, dU, dV, dInst, dTriId, dSamples, dOpacity})) {
		snail_set_error("%s: bad camera or resolution, a null buffer, or a buffer not 16-byte aligned", fn);
		return 1;
	}
	if(int rc = checkIMatAny(m, fn)) return rc;
	SnailInstances *h = m->inst;
	hipStream_t st = (hipStream_t)stream;
	DeviceGuard guard(m->device);
	std::lock_guard<std::mutex> lock(h->mu);
	dev::InstArgs I;
	bool sse, deep;
	if(int rc = instancesBegin(h, fn, I, &sse, &deep, st)) return rc;   // (the stage reads the instance records: ordered against updates as a walk is)
	dev::ITranspArgs S;
	memset(&S, 0, sizeof(S));
	imatFillArgs(m, S.a, I, cam, resx, resy, dPacketXY, nPackets);
	S.a.m.s.hitT = dT; S.a.m.s.hitId = dTriId; S.a.m.hitU = dU; S.a.m.hitV = dV; S.a.hitInst = dInst;
	S.a.m.samples = dSamples;
	S.opacity = dOpacity; S.sel = dSel;
	SNAIL_ITRANSP_LAUNCH(sse, dim3(nPackets), st, S, k_imat_sample_transp);
	return instancesEnd(h, st);
}

int snail_instances_materials_shade_rays_transp_dev(SnailInstancesMaterials *m, int nPackets, const float *dDir, const uint8_t *dMask, const float *dT,
													const float *dBary, const int32_t *dInst, const int32_t *dTriId, float *dSamples, float *dOpacity, uint8_t *dSel,
													void *stream) {
	const char *fn = "snail_instances_materials_shade_rays_transp_dev";
	if(nPackets <= 0) return 0;
	if(!dDir || !dT || !dBary || !dInst || !dTriId || !dSamples || !dOpacity || !dSel || !matAligned16({dDir, dT, dBary, dInst, dTriId, dSamples, dOpacity})) {
		snail_set_error("%s: a null buffer, or a buffer not 16-byte aligned", fn);
		return 1;
	}
	if(int rc = checkIMatAny(m, fn)) return rc;
	SnailInstances *h = m->inst;
	hipStream_t st = (hipStream_t)stream;
	DeviceGuard guard(m->device);
	std::lock_guard<std::mutex> lock(h->mu);
	dev::InstArgs I;
	bool sse, deep;
	if(int rc = instancesBegin(h, fn, I, &sse, &deep, st)) return rc;
	dev::ITranspArgs S;
	memset(&S, 0, sizeof(S));
	const float noCam[13] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 1};   // (generic packets carry their rays: no stage of this call generates any)
	imatFillArgs(m, S.a, I, noCam, 16, 16, nullptr, nPackets);
	S.a.m.s.rDir = const_cast<float *>(dDir); S.a.m.s.rMask = const_cast<uint8_t *>(dMask); S.a.m.s.rDist = const_cast<float *>(dT);
	S.a.m.s.rObj = const_cast<int32_t *>(dTriId);
	S.a.m.rU = dBary; S.a.m.rV = dBary + 4; S.a.m.rUVStride = 8;
	S.a.m.nSamples = dSamples;
	S.rInst = dInst;
	S.opacity = dOpacity; S.sel = dSel;
	SNAIL_ITRANSP_LAUNCH(sse, dim3(nPackets), st, S, k_imat_sample_transp_rays);
	return instancesEnd(h, st);
}

int snail_instances_materials_continue_packets_dev(SnailInstancesMaterials *m, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets,
												   const float *dOriginIn, const float *dDirIn, const float *dIDirIn, const float *dT, const uint8_t *dSel, float *dOrigin,
												   float *dDir, float *dIDir, uint8_t *dMask, float *dDistance, int32_t *dObject, int32_t *dElement, float *dBary,
												   int32_t *dOrder, uint64_t *dStats, void *stream) {
	const char *fn = "snail_instances_materials_continue_packets_dev";
	if(nPackets <= 0) return 0;
	const bool generic = dOriginIn || dDirIn || dIDirIn;
	if(generic && (!dOriginIn || !dDirIn || !dIDirIn)) { snail_set_error("%s: origin, direction and inverse direction of the level's packets go together (all three, or none for the primary level)", fn); return 1; }
	if(!generic && (!cam || resx <= 0 || resy <= 0 || !dPacketXY)) { snail_set_error("%s: the primary level needs a camera, a resolution and a packet list", fn); return 1; }
	if(!dT || !dSel || !dOrigin || !dDir || !dIDir || !dMask || !dDistance || !dObject || !dElement || !dBary || !dOrder ||
	   !matAligned16({dOriginIn, dDirIn, dIDirIn, dT, dOrigin, dDir, dIDir, dDistance, dObject, dElement, dBary})) {
		snail_set_error("%s: a null buffer, or a buffer not 16-byte aligned", fn);
		return 1;
	}
	if(dOrigin == dOriginIn || dDir == dDirIn || dIDir == dIDirIn) { snail_set_error("%s: the next level's packets must not be written over the level's own", fn); return 1; }
	if(int rc = checkIMatAny(m, fn)) return rc;
	SnailInstances *h = m->inst;
	hipStream_t st = (hipStream_t)stream;
	DeviceGuard guard(m->device);
	std::lock_guard<std::mutex> lock(h->mu);
	dev::InstArgs I;
	bool sse, deep;
	if(int rc = instancesBegin(h, fn, I, &sse, &deep, st)) return rc;   // (the arithmetic and its tables are the BLAS scenes'; ordered as every launch of the handle)
	dev::IMatArgs A;
	const float noCam[13] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 1};
	if(generic) imatFillArgs(m, A, I, noCam, 16, 16, nullptr, nPackets);
	else imatFillArgs(m, A, I, cam, resx, resy, dPacketXY, nPackets);
	dev::TranspArgs T;
	memset(&T, 0, sizeof(T));
	T.m = A.m;
	T.cOrg = dOriginIn; T.cDir = dDirIn; T.cIDir = dIDirIn; T.cT = dT; T.cSel = dSel;
	T.m.s.rOrg = dOrigin; T.m.s.rDir = dDir; T.m.s.rIDir = dIDir; T.m.s.rMask = dMask; T.m.s.rDist = dDistance; T.m.s.rObj = dObject;
	T.order = dOrder;
	T.m.s.stats = (dev::u64 *)dStats;
	if(generic) SNAIL_LAUNCH(sse, TranspArgs, dim3(nPackets), dim3(64), 0, st, T, k_mat_continue_rays);
	else SNAIL_LAUNCH(sse, TranspArgs, dim3(nPackets), dim3(64), 0, st, T, k_mat_continue);
	hipError_t e = hipMemsetAsync(dElement, 0, (size_t)nPackets * 256 * 4, st);
	if(e == hipSuccess) e = hipMemsetAsync(dBary, 0, (size_t)nPackets * 256 * 8, st);
	const int rc = instancesEnd(h, st);   // (the kernel is enqueued: booked as every launch of the handle is, whatever the clears did)
	if(e != hipSuccess) { snail_set_error("%s: clearing the element and bary buffers failed: %s", fn, hipGetErrorString(e)); return 100 + (int)e; }
	return rc;
}

int snail_instances_materials_transparent_dev(SnailInstancesMaterials *m, const float cam[13], int resx, int resy, const float *lights7, int nLights,
											  const float ambient[3], int flags, uint8_t *frame, int pitch, int maxDepth, uint64_t *dTruncated, uint64_t *dStats,
											  void *stream) {
	const char *fn = "snail_instances_materials_transparent_dev";
	if(int rc = checkTranspFrameArgs(fn, cam, resx, resy, lights7, nLights, ambient, flags, maxDepth, dTruncated)) return rc;
	if(int rc = checkIMatAny(m, fn)) return rc;
	if(!frame || pitch < resx * 3) { snail_set_error("%s: null frame or a pitch below 3 * resx", fn); return 1; }
	DeviceGuard guard(m->device);
	std::lock_guard<std::mutex> lock(m->inst->mu);
	return imatTranspDev(m, fn, cam, resx, resy, nullptr, 0, lights7, nLights, ambient, frame, pitch, nullptr, maxDepth, dTruncated, dStats, (hipStream_t)stream);
}

int snail_instances_materials_transparent_packets_dev(SnailInstancesMaterials *m, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets,
													  const float *lights7, int nLights, const float ambient[3], int flags, uint8_t *bgrPackets, int maxDepth,
													  uint64_t *dTruncated, uint64_t *dStats, void *stream) {
	const char *fn = "snail_instances_materials_transparent_packets_dev";
	if(int rc = checkTranspFrameArgs(fn, cam, resx, resy, lights7, nLights, ambient, flags, maxDepth, dTruncated)) return rc;
	if(int rc = checkIMatAny(m, fn)) return rc;
	if(!dPacketXY && nPackets > 0) { snail_set_error("%s: null packet list", fn); return 1; }
	if(nPackets <= 0) return 0;
	if(!bgrPackets || ((unsigned long long)bgrPackets & 3)) { snail_set_error("%s: null or unaligned output", fn); return 1; }
	DeviceGuard guard(m->device);
	std::lock_guard<std::mutex> lock(m->inst->mu);
	return imatTranspDev(m, fn, cam, resx, resy, dPacketXY, nPackets, lights7, nLights, ambient, nullptr, 0, bgrPackets, maxDepth, dTruncated, dStats, (hipStream_t)stream);
}

int snail_instances_materials_transparent_image(SnailInstancesMaterials *m, const float cam[13], int resx, int resy, const float *lights7, int nLights,
												const float ambient[3], int flags, uint8_t *image, int pitch, int maxDepth, uint64_t *truncated, uint64_t stats[4]) {
	const char *fn = "snail_instances_materials_transparent_image";
	if(int rc = checkTranspFrameArgs(fn, cam, resx, resy, lights7, nLights, ambient, flags, maxDepth, truncated)) return rc;
	if(int rc = checkIMatAny(m, fn)) return rc;
	if(!image || pitch < resx * 3) { snail_set_error("%s: null image or a pitch below 3 * resx", fn); return 1; }
	SnailInstances *h = m->inst;
	DeviceGuard guard(m->device);
	HostCallScope hc(h->blas[0], fn);   // (a stream, counters and staging arena of the call's own; the BLAS handle only lends its free list)
	if(hc.rc) return hc.rc;
	if(int rc = hc.zeroStats()) return rc;
	const int pw = (resx + 15) / 16, ph = (resy + 15) / 16, np = pw * ph;
	std::vector<int32_t> xy((size_t)np * 2);
	for(int y = 0; y < ph; y++)
		for(int x = 0; x < pw; x++) { xy[((size_t)y * pw + x) * 2] = x * 16; xy[((size_t)y * pw + x) * 2 + 1] = y * 16; }
	typedef HostCallScope H;
	const size_t imgBytes = (size_t)pitch * resy, bufBytes = SnailInstancesMaterials::Bufs::bytes((size_t)np, nLights),
				 levelBytes = levelsBytes<SnailInstancesMaterials::BounceBufs>((size_t)np, nLights, maxDepth, false);
	if(int rc = hc.reserve(H::pad(xy.size() * 4) + H::pad(bufBytes) + H::pad(levelBytes) + H::pad(imgBytes + 4) + H::pad(8))) return rc;
	void *dXY = nullptr;
	if(int rc = hc.put(&dXY, xy.data(), xy.size() * 4)) return rc;
	SnailInstancesMaterials::Bufs W;
	W.carve((char *)hc.carve(bufBytes), (size_t)np);
	char *arena = (char *)hc.carve(levelBytes);
	uint8_t *dImg = (uint8_t *)hc.carve(imgBytes + 4);
	uint64_t *dTrunc = (uint64_t *)hc.carve(8);
	HIP_TRY(hipMemsetAsync(dTrunc, 0, 8, hc.stream()));
	{
		std::lock_guard<std::mutex> lock(h->mu);
		if(int rc = shadeLevels<IMatLevels>(m, fn, cam, resx, resy, (const int32_t *)dXY, np, lights7, nLights, ambient, dImg, pitch, nullptr, nullptr, W, arena, maxDepth, false, dTrunc,
											hc.stats(), hc.stream()))
			return rc;
	}
	HIP_TRY(hipMemcpy2DAsync(image, (size_t)pitch, dImg, (size_t)pitch, (size_t)resx * 3, (size_t)resy, hipMemcpyDeviceToHost, hc.stream()));
	uint64_t got = 0;
	if(int rc = hc.get(&got, dTrunc, 8)) return rc;
	if(int rc = hc.finish(stats)) return rc;
	*truncated += got;
	return 0;
}

} // extern "C"
