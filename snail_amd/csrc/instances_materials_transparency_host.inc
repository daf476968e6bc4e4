// instances_materials_transparency_host.inc -- the C-ABI of include/snail_instances_materials_transparency.h: the creator that accepts the kinds which
// can select a transparent lane (one body with snail_instances_materials_create: imatCreate, instances_materials_host.inc), the query, the launches
// of instances_materials_transparency.inc on their own (k_imat_sample_transp / _rays) and of the scene-free generator (k_mat_continue / _rays,
// materials_transparency.inc), and the frames that run them level by level: the frame bodies of materials_levels_host.inc at a depth (shadeLevels
// without the bounce: way down with k_imat_trace_level, truncation count, way back up with k_mat_blend_transp / k_imat_light_transp /
// k_mat_colour_transp and the primary k_imat_light / k_mat_final) over IMatLevels (instances_materials_host.inc).  These entry points take ANY set
// (checkIMatAny); the older ones refuse a set that answers the query with 1 (checkIMat).  Included after instances_materials_bounce_host.inc and
// materials_transparency_host.inc, whose checkTranspFrameArgs and matAligned16 it calls.
#include "../../include/snail_instances_materials_transparency.h"

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
	return frameDev<IMatLevels>(m, fn, cam, resx, resy, lights7, nLights, ambient, false, maxDepth, frame, pitch, dTruncated, dStats, stream);
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
	return framePacketsDev<IMatLevels>(m, fn, cam, resx, resy, dPacketXY, nPackets, lights7, nLights, ambient, false, maxDepth, bgrPackets, dTruncated, dStats, stream);
}

int snail_instances_materials_transparent_image(SnailInstancesMaterials *m, const float cam[13], int resx, int resy, const float *lights7, int nLights,
												const float ambient[3], int flags, uint8_t *image, int pitch, int maxDepth, uint64_t *truncated, uint64_t stats[4]) {
	const char *fn = "snail_instances_materials_transparent_image";
	if(int rc = checkTranspFrameArgs(fn, cam, resx, resy, lights7, nLights, ambient, flags, maxDepth, truncated)) return rc;
	if(int rc = checkIMatAny(m, fn)) return rc;
	if(!image || pitch < resx * 3) { snail_set_error("%s: null image or a pitch below 3 * resx", fn); return 1; }
	return frameImage<IMatLevels>(m, fn, cam, resx, resy, lights7, nLights, ambient, false, maxDepth, image, pitch, truncated, stats);
}

} // extern "C"
