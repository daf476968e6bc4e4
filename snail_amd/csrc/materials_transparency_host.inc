// materials_transparency_host.inc -- the C-ABI of include/snail_materials_transparency.h: the creator that accepts the kinds which can select a
// transparent lane (one body with snail_materials_create: matCreate, materials_host.inc), the query, and the launches of
// materials_transparency.inc (k_mat_sample_transp / _rays, k_mat_continue / _rays), and the frames that run them level by level (shadeLevels,
// materials_levels_host.inc, without the bounce: way down, truncation count, way back up with k_mat_blend_transp / k_mat_light_transp /
// k_mat_colour_transp and the primary k_mat_light / k_mat_final), with MatLevels, what the level driver asks of a plain scene.
// These entry points take ANY set (checkMaterialsAny); the older ones refuse a set that answers the query with 1 (checkMaterials).
#include "../../include/snail_materials_transparency.h"

namespace {

bool matAligned16(std::initializer_list<const void *> ps) {
	unsigned long long a = 0;
	for(const void *p : ps) a |= (unsigned long long)p;
	return (a & 15) == 0;
}

int checkTranspFrameArgs(const char *fn, const float cam[13], int resx, int resy, const float *lights7, int nLights, const float ambient[3], int flags, int maxDepth,
						 const uint64_t *trunc) {
	if(flags) {
		snail_set_error("%s: flags must be 0 (got 0x%x): the bounce (SNAIL_RENDER_REFLECTIONS), depth shading and antialiasing are not combined with the transparency continuation", fn, flags);
		return 1;
	}
	if(maxDepth < 1 || maxDepth > SNAIL_MAT_TRANSP_MAX_DEPTH) { snail_set_error("%s: maxDepth %d outside 1..%d", fn, maxDepth, SNAIL_MAT_TRANSP_MAX_DEPTH); return 1; }
	if(!trunc) { snail_set_error("%s: null truncated-lane counter", fn); return 1; }
	return checkMatFrameArgs(fn, cam, resx, resy, lights7, nLights, ambient, 0);
}

// The plain scene's kind of the level driver (materials_levels_host.inc); the scene's mu held.  The scene-free stages' TreeArgs is the only
// argument record: its MatArgs is the frame's, and the sample and light stages take its TranspArgs.
struct MatLevels : LevelsFrame {
	typedef SnailMaterials Handle;
	typedef SnailMaterials::Bufs Bufs;
	typedef SnailMaterials::BounceBufs BounceBufs;
	typedef SnailMaterials::Set Set;
	SnailMaterials *m;
	SnailScene *s;
	SceneUse use;
	int relWhich[SNAIL_MAX_LIGHTS];   // the origin-relative copies taken by lightsBegin
	MatLevels(SnailMaterials *m_, const char *fn_, hipStream_t st_, uint32_t *pstats_, int np_, int nLights) : LevelsFrame(fn_, st_, pstats_, np_, nLights), m(m_), s(m_->scene), use(s, st_) {
		for(int n = 0; n < SNAIL_MAX_LIGHTS; n++) relWhich[n] = -1;
	}
	int begin() {
		sse = s->arith == SNAIL_ARITH_HOST_SSE; deep = useDeep(s);
		return use.rc;
	}
	// every origin-relative copy taken is booked as used on st on EVERY way out, first error kept (matShade's rule)
	int end() {
		int rc = 0;
		for(int n = 0; n < SNAIL_MAX_LIGHTS; n++)
			if(relWhich[n] >= 0) { const int urc = relUsed(s, relWhich[n], st); if(!rc) rc = urc; }
		return rc;
	}
	int primary(const float cam[13], int resx, int resy, const int32_t *dXY, const Bufs &W, uint64_t *dStats) {
		return launchPrimary(s, cam, resx, resy, 0, 0, 0, 0, dXY, np, W.hitT, W.hitU, W.hitV, W.hitId, dStats, st, nullptr, false, nullptr, nullptr, nullptr, nullptr, 0, pstats);
	}
	dev::MatArgs &frameArgs(dev::TreeArgs &G, const float cam[13], int resx, int resy, const int32_t *dXY, const Bufs &W) {
		dev::MatArgs &A = G.t.m;
		matFillArgs(m, A, cam, resx, resy, dXY, np);
		A.s.hitId = W.hitId;
		return A;
	}
	static int *object(const BounceBufs &R) { return R.rObj; }
	void level(dev::TreeArgs &G, const BounceBufs &R, const int32_t *, bool) { G.t.m.s.rObj = R.rObj; }
	int walk(const BounceBufs &R, const int32_t *order, uint64_t *dStats) {
		// the walk reads the barycentrics it was given and writes them back for lanes without a hit: zeros, not what the buffer last held
		const hipError_t e = hipMemsetAsync(R.bary, 0, (size_t)np * 256 * 8, st);
		if(e != hipSuccess) return failed("hipMemsetAsync", e);
		return launchRays(s, false, np, 64, 0, R.rOrg, R.rDir, R.rIDir, R.rMask, R.rDist, R.rObj, R.bary, dStats, st, order, nullptr, order ? np : 0, nullptr, 0, pstats);
	}
	int samplePrimary(dev::TreeArgs &G, float *opacity, unsigned char *sel) {
		G.t.opacity = opacity; G.t.sel = sel;
		SNAIL_LAUNCH(sse, TranspArgs, grid, dim3(64), 0, st, G.t, k_mat_sample_transp);
		return launched("k_mat_sample_transp");
	}
	int sampleRays(dev::TreeArgs &G, float *opacity, unsigned char *sel) {
		G.t.opacity = opacity; G.t.sel = sel;
		SNAIL_LAUNCH(sse, TranspArgs, grid, dim3(64), 0, st, G.t, k_mat_sample_transp_rays);
		return launched("k_mat_sample_transp_rays");
	}
	// (the lights of every level of both chains walk from the same origins: the same copies)
	int lightsBegin(dev::MatArgs &A, int nLights) {
		int rc = 0;
		if(nLights && A.s.pack && !deep)
			for(int n = 0; n < nLights && !rc; n++) rc = relFor(s, A.s.lights[n], st, &A.s.relLight[n], &relWhich[n]);
		return rc;
	}
	int nestedLights(dev::TreeArgs &G) {
		SNAIL_LEVELS_LAUNCH_DEEP(TranspArgs, lgrid, G.t, k_mat_light_transp);
		return launched("k_mat_light_transp");
	}
	int lights(dev::TreeArgs &G) {
		SNAIL_LEVELS_LAUNCH_DEEP(MatArgs, lgrid, G.t.m, k_mat_light);
		return launched("k_mat_light");
	}
	// the handle's part of levelsStore and of the host calls
	static int nextSet(SnailMaterials *m, int np, int nLights, hipStream_t st, Set **out) { return matNextSet(m, np, nLights, false, false, st, out); }
	static int setDone(Set &W, const char *fn, int rc, hipStream_t st) { return matSetDone(W, fn, rc, st); }
	static int depthStore(SnailMaterials *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights,
						  const float ambient[3], int flags, const float *tint, uint8_t *bgrPackets, const InstTileJob *J, uint64_t *dStats, hipStream_t st) {
		return matShadeStore(m, fn, cam, resx, resy, dXY, np, lights7, nLights, ambient, flags, tint, bgrPackets, J, dStats, st);
	}
	static SnailScene *scene(SnailMaterials *m) { return m->scene; }
	static std::mutex &mu(SnailMaterials *m) { return m->scene->mu; }
	static int frameList(SnailMaterials *m, int resx, int resy, const int32_t **dXY, int *np) { return matFrameList(m, resx, resy, dXY, np); }
};

// _dev / _packets_dev (the scene's mu held): the next group of intermediates with its fourth part, grown if need be
int matTranspDev(SnailMaterials *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights,
				 const float ambient[3], uint8_t *frame, int pitch, uint8_t *bgrPackets, int maxDepth, uint64_t *dTrunc, uint64_t *dStats, hipStream_t st) {
	if(!dXY) { if(int rc = matFrameList(m, resx, resy, &dXY, &np)) return rc; }
	SnailMaterials::Set *Wp = nullptr;
	if(int rc = matNextSet(m, np, nLights, false, false, st, &Wp)) return rc;
	SnailMaterials::Set &W = *Wp;
	const size_t want = levelsBytes<SnailMaterials::BounceBufs>((size_t)np, nLights, maxDepth, false);
	if(int rc = levelsGrow(W, W.transp, W.transpBytes, want, want)) return rc;
	SnailMaterials::Bufs B;
	B.carve(W.base, (size_t)np);
	const int rc = shadeLevels<MatLevels>(m, fn, cam, resx, resy, dXY, np, lights7, nLights, ambient, frame, pitch, bgrPackets, nullptr, B, W.transp, maxDepth, false, dTrunc, dStats, st);
	return matSetDone(W, fn, rc, st);
}

} // namespace

extern "C" {

SnailMaterials *snail_materials_create_transparent(SnailScene *scene, const void *shtris64, int nTris, const int32_t *matMap, int nMap, const SnailMaterial *mats,
												   int nMats, const int32_t *opacityTexture, const SnailTexture *textures, int nTex) {
	return matCreate("snail_materials_create_transparent", true, scene, shtris64, nTris, matMap, nMap, mats, nMats, opacityTexture, textures, nTex);
}

int snail_materials_can_select_transparent(const SnailMaterials *m) {
	if(!m) { snail_set_error("snail_materials_can_select_transparent: invalid material set handle"); return -1; }
	return m->canSelectTransparent ? 1 : 0;
}

int snail_materials_shade_packets_transp_dev(SnailMaterials *m, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets, const float *dT,
											 const float *dU, const float *dV, const int32_t *dTriId, float *dSamples, float *dOpacity, uint8_t *dSel, void *stream) {
	const char *fn = "snail_materials_shade_packets_transp_dev";
	if(int rc = checkMaterialsAny(m, fn)) return rc;
	if(nPackets <= 0) return 0;
	if(!cam || resx <= 0 || resy <= 0 || !dPacketXY || !dT || !dU || !dV || !dTriId || !dSamples || !dOpacity || !dSel || !matAligned16({dT, dU, dV, dTriId, dSamples, dOpacity})) {
		snail_set_error("%s: bad camera or resolution, a null buffer, or a buffer not 16-byte aligned", fn);
		return 1;
	}
	DeviceGuard guard(m->device);
	SNAIL_LOCK(m->scene);
	dev::TranspArgs T;
	memset(&T, 0, sizeof(T));
	matFillArgs(m, T.m, cam, resx, resy, dPacketXY, nPackets);
	T.m.s.hitT = dT; T.m.s.hitId = dTriId; T.m.hitU = dU; T.m.hitV = dV;
	T.m.samples = dSamples;
	T.opacity = dOpacity; T.sel = dSel;
	const bool sse = m->scene->arith == SNAIL_ARITH_HOST_SSE;
	SNAIL_LAUNCH(sse, TranspArgs, dim3(nPackets), dim3(64), 0, (hipStream_t)stream, T, k_mat_sample_transp);
	HIP_TRY(hipGetLastError());
	return 0;
}

int snail_materials_shade_rays_transp_dev(SnailMaterials *m, int nPackets, const float *dDir, const uint8_t *dMask, const float *dT, const float *dU, const float *dV,
										  const int32_t *dTriId, float *dSamples, float *dOpacity, uint8_t *dSel, void *stream) {
	const char *fn = "snail_materials_shade_rays_transp_dev";
	if(int rc = checkMaterialsAny(m, fn)) return rc;
	if(nPackets <= 0) return 0;
	if(!dDir || !dT || !dU || !dV || !dTriId || !dSamples || !dOpacity || !dSel || !matAligned16({dDir, dT, dU, dV, dTriId, dSamples, dOpacity})) {
		snail_set_error("%s: a null buffer, or a buffer not 16-byte aligned", fn);
		return 1;
	}
	DeviceGuard guard(m->device);
	SNAIL_LOCK(m->scene);
	dev::TranspArgs T;
	memset(&T, 0, sizeof(T));
	const float noCam[13] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 1};   // (generic packets carry their rays: no stage of this call generates any)
	matFillArgs(m, T.m, noCam, 16, 16, nullptr, nPackets);
	T.m.s.rDir = const_cast<float *>(dDir); T.m.s.rMask = const_cast<uint8_t *>(dMask); T.m.s.rDist = const_cast<float *>(dT); T.m.s.rObj = const_cast<int32_t *>(dTriId);
	T.m.rU = dU; T.m.rV = dV; T.m.rUVStride = 4;
	T.m.nSamples = dSamples;
	T.opacity = dOpacity; T.sel = dSel;
	const bool sse = m->scene->arith == SNAIL_ARITH_HOST_SSE;
	SNAIL_LAUNCH(sse, TranspArgs, dim3(nPackets), dim3(64), 0, (hipStream_t)stream, T, k_mat_sample_transp_rays);
	HIP_TRY(hipGetLastError());
	return 0;
}

int snail_materials_continue_packets_dev(SnailMaterials *m, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets, const float *dOriginIn,
										 const float *dDirIn, const float *dIDirIn, const float *dT, const uint8_t *dSel, float *dOrigin, float *dDir, float *dIDir,
										 uint8_t *dMask, float *dDistance, int32_t *dObject, int32_t *dOrder, uint64_t *dStats, void *stream) {
	const char *fn = "snail_materials_continue_packets_dev";
	if(int rc = checkMaterialsAny(m, fn)) return rc;
	if(nPackets <= 0) return 0;
	const bool generic = dOriginIn || dDirIn || dIDirIn;
	if(generic && (!dOriginIn || !dDirIn || !dIDirIn)) { snail_set_error("%s: origin, direction and inverse direction of the level's packets go together (all three, or none for the primary level)", fn); return 1; }
	if(!generic && (!cam || resx <= 0 || resy <= 0 || !dPacketXY)) { snail_set_error("%s: the primary level needs a camera, a resolution and a packet list", fn); return 1; }
	if(!dT || !dSel || !dOrigin || !dDir || !dIDir || !dMask || !dDistance || !dObject || !dOrder ||
	   !matAligned16({dOriginIn, dDirIn, dIDirIn, dT, dOrigin, dDir, dIDir, dDistance, dObject})) {
		snail_set_error("%s: a null buffer, or a buffer not 16-byte aligned", fn);
		return 1;
	}
	if(dOrigin == dOriginIn || dDir == dDirIn || dIDir == dIDirIn) { snail_set_error("%s: the next level's packets must not be written over the level's own", fn); return 1; }
	DeviceGuard guard(m->device);
	SNAIL_LOCK(m->scene);
	dev::TranspArgs T;
	memset(&T, 0, sizeof(T));
	const float noCam[13] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 1};
	if(generic) matFillArgs(m, T.m, noCam, 16, 16, nullptr, nPackets);
	else matFillArgs(m, T.m, cam, resx, resy, dPacketXY, nPackets);
	T.cOrg = dOriginIn; T.cDir = dDirIn; T.cIDir = dIDirIn; T.cT = dT; T.cSel = dSel;
	T.m.s.rOrg = dOrigin; T.m.s.rDir = dDir; T.m.s.rIDir = dIDir; T.m.s.rMask = dMask; T.m.s.rDist = dDistance; T.m.s.rObj = dObject;
	T.order = dOrder;
	T.m.s.stats = (dev::u64 *)dStats;
	const bool sse = m->scene->arith == SNAIL_ARITH_HOST_SSE;
	if(generic) SNAIL_LAUNCH(sse, TranspArgs, dim3(nPackets), dim3(64), 0, (hipStream_t)stream, T, k_mat_continue_rays);
	else SNAIL_LAUNCH(sse, TranspArgs, dim3(nPackets), dim3(64), 0, (hipStream_t)stream, T, k_mat_continue);
	HIP_TRY(hipGetLastError());
	return 0;
}

int snail_materials_transparent_dev(SnailMaterials *m, const float cam[13], int resx, int resy, const float *lights7, int nLights, const float ambient[3], int flags,
									uint8_t *frame, int pitch, int maxDepth, uint64_t *dTruncated, uint64_t *dStats, void *stream) {
	const char *fn = "snail_materials_transparent_dev";
	if(int rc = checkTranspFrameArgs(fn, cam, resx, resy, lights7, nLights, ambient, flags, maxDepth, dTruncated)) return rc;
	if(int rc = checkMaterialsAny(m, fn)) return rc;
	if(!frame || pitch < resx * 3) { snail_set_error("%s: null frame or a pitch below 3 * resx", fn); return 1; }
	DeviceGuard guard(m->device);
	SNAIL_LOCK(m->scene);
	return matTranspDev(m, fn, cam, resx, resy, nullptr, 0, lights7, nLights, ambient, frame, pitch, nullptr, maxDepth, dTruncated, dStats, (hipStream_t)stream);
}

int snail_materials_transparent_packets_dev(SnailMaterials *m, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets, const float *lights7,
											int nLights, const float ambient[3], int flags, uint8_t *bgrPackets, int maxDepth, uint64_t *dTruncated, uint64_t *dStats,
											void *stream) {
	const char *fn = "snail_materials_transparent_packets_dev";
	if(int rc = checkTranspFrameArgs(fn, cam, resx, resy, lights7, nLights, ambient, flags, maxDepth, dTruncated)) return rc;
	if(int rc = checkMaterialsAny(m, fn)) return rc;
	if(!dPacketXY && nPackets > 0) { snail_set_error("%s: null packet list", fn); return 1; }
	if(nPackets <= 0) return 0;
	if(!bgrPackets || ((unsigned long long)bgrPackets & 3)) { snail_set_error("%s: null or unaligned output", fn); return 1; }
	DeviceGuard guard(m->device);
	SNAIL_LOCK(m->scene);
	return matTranspDev(m, fn, cam, resx, resy, dPacketXY, nPackets, lights7, nLights, ambient, nullptr, 0, bgrPackets, maxDepth, dTruncated, dStats, (hipStream_t)stream);
}

int snail_materials_transparent_image(SnailMaterials *m, const float cam[13], int resx, int resy, const float *lights7, int nLights, const float ambient[3], int flags,
									  uint8_t *image, int pitch, int maxDepth, uint64_t *truncated, uint64_t stats[4]) {
	const char *fn = "snail_materials_transparent_image";
	if(int rc = checkTranspFrameArgs(fn, cam, resx, resy, lights7, nLights, ambient, flags, maxDepth, truncated)) return rc;
	if(int rc = checkMaterialsAny(m, fn)) return rc;
	if(!image || pitch < resx * 3) { snail_set_error("%s: null image or a pitch below 3 * resx", fn); return 1; }
	DeviceGuard guard(m->device);
	HostCallScope hc(m->scene, fn);
	if(hc.rc) return hc.rc;
	if(int rc = hc.zeroStats()) return rc;
	const int pw = (resx + 15) / 16, ph = (resy + 15) / 16, np = pw * ph;
	std::vector<int32_t> xy((size_t)np * 2);
	for(int y = 0; y < ph; y++)
		for(int x = 0; x < pw; x++) { xy[((size_t)y * pw + x) * 2] = x * 16; xy[((size_t)y * pw + x) * 2 + 1] = y * 16; }
	typedef HostCallScope H;
	const size_t imgBytes = (size_t)pitch * resy, bufBytes = SnailMaterials::Bufs::bytes((size_t)np, nLights),
				 levelBytes = levelsBytes<SnailMaterials::BounceBufs>((size_t)np, nLights, maxDepth, false);
	if(int rc = hc.reserve(H::pad(xy.size() * 4) + H::pad(bufBytes) + H::pad(levelBytes) + H::pad(imgBytes + 4) + H::pad(8))) return rc;
	void *dXY = nullptr;
	if(int rc = hc.put(&dXY, xy.data(), xy.size() * 4)) return rc;
	SnailMaterials::Bufs W;
	W.carve((char *)hc.carve(bufBytes), (size_t)np);
	char *arena = (char *)hc.carve(levelBytes);
	uint8_t *dImg = (uint8_t *)hc.carve(imgBytes + 4);
	uint64_t *dTrunc = (uint64_t *)hc.carve(8);
	HIP_TRY(hipMemsetAsync(dTrunc, 0, 8, hc.stream()));
	{
		SNAIL_LOCK(m->scene);
		if(int rc = shadeLevels<MatLevels>(m, fn, cam, resx, resy, (const int32_t *)dXY, np, lights7, nLights, ambient, dImg, pitch, nullptr, nullptr, W, arena, maxDepth, false, dTrunc,
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
