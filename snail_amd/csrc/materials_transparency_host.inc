// materials_transparency_host.inc -- the C-ABI of include/snail_materials_transparency.h: the creator that accepts the kinds which can select a
// transparent lane (one body with snail_materials_create: matCreate, materials_host.inc), the query, and the launches of
// materials_transparency.inc (k_mat_sample_transp / _rays, k_mat_continue / _rays), and the frames that run them level by level (matShadeTransp:
// way down, truncation count, way back up with k_mat_blend_transp / k_mat_light_transp / k_mat_colour_transp and the primary k_mat_light /
// k_mat_final).  These entry points take ANY set (checkMaterialsAny); the older ones refuse a set that answers the query with 1 (checkMaterials).
// BUILD NOTE: the Makefile's source list does not name this file; after editing it alone, touch materials_host.inc (or make clean).
#include "../../include/snail_materials_transparency.h"

namespace {

bool matAligned16(std::initializer_list<const void *> ps) {
	unsigned long long a = 0;
	for(const void *p : ps) a |= (unsigned long long)p;
	return (a & 15) == 0;
}

// ---- frames: the levels of the transparency continuation -----------------------------------------------------------------------------------
// One level's intermediates: the generic packets and everything of the bounce's part (BounceBufs: rays, mask, hits, barycentrics, samples,
// colour, shadow distances) + opacity, selector and the level's order list.  Level 0 (the primary packets, SnailMaterials::Bufs) has the
// last three alone.
struct TranspLevel {
	SnailMaterials::BounceBufs R;
	float *opacity = nullptr;
	unsigned char *sel = nullptr;
	int32_t *order = nullptr;
	static size_t extra(size_t np) { return np * 1024 + ((np * 64 + 255) & ~(size_t)255) + ((np * 4 + 255) & ~(size_t)255); }
	static size_t bytes(size_t np, int nLights) { return ((SnailMaterials::BounceBufs::bytes(np, nLights) + 255) & ~(size_t)255) + extra(np); }
	char *carveExtra(char *p, size_t np) {
		opacity = (float *)p; p += np * 1024;
		sel = (unsigned char *)p; p += (np * 64 + 255) & ~(size_t)255;
		order = (int32_t *)p; p += (np * 4 + 255) & ~(size_t)255;
		return p;
	}
	char *carve(char *p, size_t np, int nLights) {
		R.carve(p, np, nLights);
		return carveExtra(p + ((SnailMaterials::BounceBufs::bytes(np, nLights) + 255) & ~(size_t)255), np);
	}
};
size_t transpBytes(size_t np, int nLights, int depth) { return TranspLevel::extra(np) + (size_t)depth * TranspLevel::bytes(np, nLights); }

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

// the stages of one frame with the continuation over the packet list dXY (the scene's mu held); W: level 0, `levels`: maxDepth levels carved at `arena`
int matShadeTransp(SnailMaterials *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights,
				   const float ambient[3], uint8_t *frame, int pitch, uint8_t *bgrPackets, const SnailMaterials::Bufs &W, char *arena, int maxDepth, uint64_t *dTrunc,
				   uint64_t *dStats, hipStream_t st) {
	SnailScene *s = m->scene;
	SceneUse use(s, st);
	if(use.rc) return use.rc;
	TranspLevel L[SNAIL_MAT_TRANSP_MAX_DEPTH + 1];
	char *p = L[0].carveExtra(arena, (size_t)np);
	for(int k = 1; k <= maxDepth; k++) p = L[k].carve(p, (size_t)np, nLights);
	if(int rc = launchPrimary(s, cam, resx, resy, 0, 0, 0, 0, dXY, np, W.hitT, W.hitU, W.hitV, W.hitId, dStats, st)) return rc;
	dev::TranspArgs T;
	memset(&T, 0, sizeof(T));
	dev::MatArgs &A = T.m;
	matFillArgs(m, A, cam, resx, resy, dXY, np);
	A.s.nLights = nLights;
	for(int n = 0; n < nLights; n++) for(int k = 0; k < 7; k++) A.s.lights[n][k] = lights7[n * 7 + k];
	for(int c = 0; c < 3; c++) { A.s.ambient[c] = ambient[c]; A.s.color[c] = 1.0f; }
	A.s.hitT = W.hitT; A.s.hitId = W.hitId; A.hitU = W.hitU; A.hitV = W.hitV;
	A.samples = W.samples; A.s.sDist = W.sDist;
	A.s.frame = frame; A.s.pitch = pitch; A.s.bgrPackets = bgrPackets;
	A.s.stats = (dev::u64 *)dStats;
	A.rUVStride = 8;
	const bool sse = s->arith == SNAIL_ARITH_HOST_SSE;
	const dim3 grid(np), wave(64);
	// a level's generic packets as the stages' source
	auto level = [&](int k) {
		const SnailMaterials::BounceBufs &R = L[k].R;
		A.s.rOrg = R.rOrg; A.s.rDir = R.rDir; A.s.rIDir = R.rIDir; A.s.rMask = R.rMask; A.s.rDist = R.rDist; A.s.rObj = R.rObj; A.s.rCol = R.rCol;
		A.rU = R.bary; A.rV = R.bary + 4;
		A.nSamples = R.nSamples; A.nSDist = R.nSDist;
		T.inOrder = L[k].order;
	};
	// ---- the way down: sample, then per level generator -> ordered walk -> nested sample ----
	T.opacity = L[0].opacity; T.sel = L[0].sel; T.inOrder = nullptr;
	SNAIL_LAUNCH(sse, TranspArgs, grid, wave, 0, st, T, k_mat_sample_transp);
	HIP_TRY(hipGetLastError());
	for(int k = 1; k <= maxDepth; k++) {
		// generator: from level k - 1 (its rays, hits, selector and own order list) into level k's packets and order list
		level(k);
		T.order = L[k].order;
		T.cT = k == 1 ? W.hitT : L[k - 1].R.rDist; T.cSel = L[k - 1].sel;
		T.inOrder = k == 1 ? nullptr : L[k - 1].order;
		if(k == 1) { T.cOrg = T.cDir = T.cIDir = nullptr; SNAIL_LAUNCH(sse, TranspArgs, grid, wave, 0, st, T, k_mat_continue); }
		else {
			T.cOrg = L[k - 1].R.rOrg; T.cDir = L[k - 1].R.rDir; T.cIDir = L[k - 1].R.rIDir;
			SNAIL_LAUNCH(sse, TranspArgs, grid, wave, 0, st, T, k_mat_continue_rays);
		}
		HIP_TRY(hipGetLastError());
		// the walk reads the barycentrics it was given and writes them back for lanes without a hit: zeros, not what the buffer last held
		HIP_TRY(hipMemsetAsync(L[k].R.bary, 0, (size_t)np * 256 * 8, st));
		if(int rc = launchRays(s, false, np, 64, 0, L[k].R.rOrg, L[k].R.rDir, L[k].R.rIDir, L[k].R.rMask, L[k].R.rDist, L[k].R.rObj, L[k].R.bary, dStats, st, L[k].order, nullptr, np))
			return rc;
		level(k);
		T.opacity = L[k].opacity; T.sel = L[k].sel;
		SNAIL_LAUNCH(sse, TranspArgs, grid, wave, 0, st, T, k_mat_sample_transp_rays);
		HIP_TRY(hipGetLastError());
	}
	// the lanes the deepest level would still select: counted, then treated as not selected
	level(maxDepth);
	T.bSel = L[maxDepth].sel; T.trunc = (unsigned long long *)dTrunc;
	SNAIL_LAUNCH(sse, TranspArgs, grid, wave, 0, st, T, k_mat_truncated);
	HIP_TRY(hipGetLastError());
	// ---- the way back up: per level (blend from the deeper level,) nested lights, nested colour; then the primary blend, lights and store ----
	int relWhich[SNAIL_MAX_LIGHTS];
	for(int n = 0; n < SNAIL_MAX_LIGHTS; n++) { relWhich[n] = -1; A.s.relLight[n] = nullptr; }
	int lrc = 0;
	// (every origin-relative copy taken here is booked as used on st on EVERY way out, first error kept: matShade's rule)
	if(nLights && A.s.pack && !useDeep(s))
		for(int n = 0; n < nLights && !lrc; n++) lrc = relFor(s, A.s.lights[n], st, &A.s.relLight[n], &relWhich[n]);
	const dim3 lgrid(np, nLights > 0 ? nLights : 1);
	auto launched = [&](const char *what) {
		const hipError_t e = hipGetLastError();
		if(e != hipSuccess && !lrc) { snail_set_error("%s: %s: %s", fn, what, hipGetErrorString(e)); lrc = 100 + (int)e; }
	};
	for(int k = maxDepth; k >= 1 && !lrc; k--) {
		level(k);
		if(k < maxDepth) {
			T.bSamples = L[k].R.nSamples; T.bOpacity = L[k].opacity; T.bSel = L[k].sel; T.bCol = L[k + 1].R.rCol;
			SNAIL_LAUNCH(sse, TranspArgs, grid, wave, 0, st, T, k_mat_blend_transp);
			launched("k_mat_blend_transp");
		}
		if(nLights && !lrc) {
			if(useDeep(s)) SNAIL_LAUNCH(sse, TranspArgs, lgrid, wave, 0, st, T, k_mat_light_transp<true>);
			else SNAIL_LAUNCH(sse, TranspArgs, lgrid, wave, 0, st, T, k_mat_light_transp<false>);
			launched("k_mat_light_transp");
		}
		if(!lrc) { SNAIL_LAUNCH(sse, TranspArgs, grid, wave, 0, st, T, k_mat_colour_transp); launched("k_mat_colour_transp"); }
	}
	if(!lrc) {
		T.inOrder = nullptr;
		T.bSamples = W.samples; T.bOpacity = L[0].opacity; T.bSel = L[0].sel; T.bCol = L[1].R.rCol;
		SNAIL_LAUNCH(sse, TranspArgs, grid, wave, 0, st, T, k_mat_blend_transp);
		launched("k_mat_blend_transp");
	}
	if(nLights && !lrc) {
		if(useDeep(s)) SNAIL_LAUNCH(sse, MatArgs, lgrid, wave, 0, st, A, k_mat_light<true>);
		else SNAIL_LAUNCH(sse, MatArgs, lgrid, wave, 0, st, A, k_mat_light<false>);
		launched("k_mat_light");
	}
	for(int n = 0; n < nLights; n++)
		if(relWhich[n] >= 0) { const int urc = relUsed(s, relWhich[n], st); if(!lrc) lrc = urc; }
	if(lrc) return lrc;
	SNAIL_LAUNCH(sse, MatArgs, grid, wave, 0, st, A, k_mat_final);
	HIP_TRY(hipGetLastError());
	return 0;
}

// _dev / _packets_dev (the scene's mu held): the next group of intermediates with its fourth part, grown if need be
int matTranspDev(SnailMaterials *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights,
				 const float ambient[3], uint8_t *frame, int pitch, uint8_t *bgrPackets, int maxDepth, uint64_t *dTrunc, uint64_t *dStats, hipStream_t st) {
	if(!dXY) { if(int rc = matFrameList(m, resx, resy, &dXY, &np)) return rc; }
	SnailMaterials::Set *Wp = nullptr;
	if(int rc = matNextSet(m, np, nLights, false, false, st, &Wp)) return rc;
	SnailMaterials::Set &W = *Wp;
	const size_t want = transpBytes((size_t)np, nLights, maxDepth);
	if(!W.transp || W.transpBytes < want) {   // grown: its previous user may still be running
		HIP_TRY(hipDeviceSynchronize());
		if(W.transp) (void)hipFree(W.transp);
		W.transp = nullptr; W.transpBytes = 0; W.used = false;
		HIP_TRY(hipMalloc((void **)&W.transp, want));
		W.transpBytes = want;
	}
	SnailMaterials::Bufs B;
	B.carve(W.base, (size_t)np);
	const int rc = matShadeTransp(m, fn, cam, resx, resy, dXY, np, lights7, nLights, ambient, frame, pitch, bgrPackets, B, W.transp, maxDepth, dTrunc, dStats, st);
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
	const size_t imgBytes = (size_t)pitch * resy, bufBytes = SnailMaterials::Bufs::bytes((size_t)np, nLights), levelBytes = transpBytes((size_t)np, nLights, maxDepth);
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
		if(int rc = matShadeTransp(m, fn, cam, resx, resy, (const int32_t *)dXY, np, lights7, nLights, ambient, dImg, pitch, nullptr, W, arena, maxDepth, dTrunc, hc.stats(), hc.stream()))
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
