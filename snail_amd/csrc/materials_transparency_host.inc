// materials_transparency_host.inc -- the C-ABI of include/snail_materials_transparency.h: the creator that accepts the kinds which can select a
// transparent lane (one body with snail_materials_create: matCreate, materials_host.inc), the query, and the launches of
// materials_transparency.inc (k_mat_sample_transp / _rays, k_mat_continue / _rays), and the frames that run them level by level: the frame
// bodies of materials_levels_host.inc at a depth (shadeLevels without the bounce: way down, truncation count, way back up with k_mat_blend_transp /
// k_mat_light_transp / k_mat_colour_transp and the primary k_mat_light / k_mat_final) over MatLevels (materials_host.inc).
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
	return frameDev<MatLevels>(m, fn, cam, resx, resy, lights7, nLights, ambient, false, maxDepth, frame, pitch, dTruncated, dStats, stream);
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
	return framePacketsDev<MatLevels>(m, fn, cam, resx, resy, dPacketXY, nPackets, lights7, nLights, ambient, false, maxDepth, bgrPackets, dTruncated, dStats, stream);
}

int snail_materials_transparent_image(SnailMaterials *m, const float cam[13], int resx, int resy, const float *lights7, int nLights, const float ambient[3], int flags,
									  uint8_t *image, int pitch, int maxDepth, uint64_t *truncated, uint64_t stats[4]) {
	const char *fn = "snail_materials_transparent_image";
	if(int rc = checkTranspFrameArgs(fn, cam, resx, resy, lights7, nLights, ambient, flags, maxDepth, truncated)) return rc;
	if(int rc = checkMaterialsAny(m, fn)) return rc;
	if(!image || pitch < resx * 3) { snail_set_error("%s: null image or a pitch below 3 * resx", fn); return 1; }
	return frameImage<MatLevels>(m, fn, cam, resx, resy, lights7, nLights, ambient, false, maxDepth, image, pitch, truncated, stats);
}

} // extern "C"
