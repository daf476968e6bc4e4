// instances_materials_tree_host.inc -- the C-ABI of include/snail_instances_materials_tree.h: the transparency continuation of an instanced scene
// together with the mirrored bounce, the tile renderer, 4x antialiasing, depth shading and the tint; included by snail_hip.hip after
// instances_materials_transparency_host.inc.  The frames are the level driver's (materials_levels_host.inc) for an instanced scene (IMatLevels,
// instances_materials_host.inc): shadeLevels with chain B under SNAIL_RENDER_REFLECTIONS, run by levelsStore over a packet list in
// slices that keep the levels within the set's budget.  No stage is new: the kernels are those of instances*.inc, materials*.inc and
// instances_shade.inc, unchanged (instances_materials_tree.inc).  The arguments are judged by matTreeArgsOk (materials_tree_host.inc).
#include "../../include/snail_instances_materials_tree.h"

extern "C" {

int snail_instances_materials_mirror_rays_dev(SnailInstancesMaterials *m, int nPackets, const float *dOriginIn, const float *dDirIn, const uint8_t *dMaskIn,
											  const float *dT, const float *dSamples, const int32_t *dOrderIn, float *dOrigin, float *dDir, float *dIDir, uint8_t *dMask,
											  float *dDistance, int32_t *dObject, int32_t *dElement, float *dBary, int32_t *dOrder, uint64_t *dStats, void *stream) {
	const char *fn = "snail_instances_materials_mirror_rays_dev";
	// the arguments first, the handle last: what is refused here needs no device
	if(nPackets <= 0) return 0;
	if(!dOriginIn || !dDirIn || !dT || !dSamples || !dOrigin || !dDir || !dIDir || !dMask || !dDistance || !dObject || !dElement || !dBary || !dOrder ||
	   !matAligned16({dOriginIn, dDirIn, dT, dSamples, dOrigin, dDir, dIDir, dDistance, dObject, dElement, dBary})) {
		snail_set_error("%s: a null buffer, or a buffer not 16-byte aligned", fn);
		return 1;
	}
	if(dOrigin == dOriginIn || dDir == dDirIn || dDistance == dT || dMask == dMaskIn) { snail_set_error("%s: the mirrored packets must not be written over the level's own", fn); return 1; }
	if(int rc = checkIMatAny(m, fn)) return rc;
	SnailInstances *h = m->inst;
	hipStream_t st = (hipStream_t)stream;
	DeviceGuard guard(m->device);
	std::lock_guard<std::mutex> lock(h->mu);
	dev::InstArgs I;
	bool sse, deep;
	if(int rc = instancesBegin(h, fn, I, &sse, &deep, st)) return rc;   // (the arithmetic and its tables are the BLAS scenes'; ordered as every launch of the handle)
	dev::IMatArgs A;
	const float noCam[13] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 1};   // (generic packets carry their rays: no stage of this call generates any)
	imatFillArgs(m, A, I, noCam, 16, 16, nullptr, nPackets);
	dev::TreeArgs G;
	memset(&G, 0, sizeof(G));
	G.t.m = A.m;
	dev::MatArgs &M = G.t.m;
	M.s.rOrg = const_cast<float *>(dOriginIn); M.s.rDir = const_cast<float *>(dDirIn); M.s.rMask = const_cast<uint8_t *>(dMaskIn); M.s.rDist = const_cast<float *>(dT);
	M.nSamples = const_cast<float *>(dSamples);
	G.t.inOrder = dOrderIn;
	G.oOrg = dOrigin; G.oDir = dDir; G.oIDir = dIDir; G.oMask = dMask; G.oDist = dDistance; G.oObj = dObject; G.oOrder = dOrder;
	M.s.stats = (dev::u64 *)dStats;
	SNAIL_LAUNCH(sse, TreeArgs, dim3(nPackets), dim3(64), 0, st, G, k_mat_mirror_rays);
	// zeros for the walk, in the packets that are part of the level alone
	hipLaunchKernelGGL(dev::k_imat_clear_hits, dim3(nPackets), dim3(64), 0, st, (int *)dElement, dBary, (const int *)dOrderIn, nPackets);
	const hipError_t e = hipGetLastError();
	const int rc = instancesEnd(h, st);   // (the kernels are enqueued: booked as every launch of the handle is)
	if(e != hipSuccess) { snail_set_error("%s: a launch failed: %s", fn, hipGetErrorString(e)); return 100 + (int)e; }
	return rc;
}

int snail_instances_materials_tree_frame_packets_dev(SnailInstancesMaterials *m, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets,
													 const float *lights7, int nLights, const float ambient[3], int flags, const float *tint, uint8_t *bgrPackets,
													 int maxDepth, uint64_t *dTruncated, uint64_t *dStats, void *stream) {
	const char *fn = "snail_instances_materials_tree_frame_packets_dev";
	if(int rc = matTreeArgsOk(fn, cam, resx, resy, lights7, nLights, ambient, flags, tint, maxDepth, dTruncated)) return rc;
	if(nPackets > 0 && !dPacketXY) { snail_set_error("%s: null packet list", fn); return 1; }
	if(nPackets > (1 << 24)) { snail_set_error("%s: more than 2^24 packets", fn); return 1; }
	if(nPackets > 0 && (!bgrPackets || ((unsigned long long)bgrPackets & 3))) { snail_set_error("%s: null or unaligned output", fn); return 1; }
	if(int rc = checkIMatAny(m, fn)) return rc;
	if(nPackets <= 0) return 0;
	DeviceGuard guard(m->device);
	std::lock_guard<std::mutex> lock(m->inst->mu);
	return levelsStore<IMatLevels>(m, fn, cam, resx, resy, dPacketXY, nPackets, lights7, nLights, ambient, flags, tint, bgrPackets, nullptr, maxDepth, dTruncated, dStats, (hipStream_t)stream);
}

int snail_instances_materials_tree_render_tiles(SnailInstancesMaterials *m, const float cam[13], int resx, int resy, const int32_t *coords, const int64_t *offsets,
												int nTiles, const float *lights7, int nLights, const float ambient[3], int flags, const float *tint, uint8_t *data,
												int maxDepth, uint64_t *truncated, uint64_t stats[4]) {
	const char *fn = "snail_instances_materials_tree_render_tiles";
	if(int rc = matTreeArgsOk(fn, cam, resx, resy, lights7, nLights, ambient, flags, tint, maxDepth, truncated)) return rc;
	if(nTiles > 0 && (!coords || !offsets || !data)) { snail_set_error("%s: null buffer", fn); return 1; }
	if(int rc = tileRectsOk(fn, coords, nTiles)) return rc;
	if(int rc = checkIMatAny(m, fn)) return rc;
	if(nTiles <= 0) return 0;
	return renderTilesHost<IMatLevels>(m, fn, cam, resx, resy, coords, offsets, nTiles, lights7, nLights, ambient, flags, tint, data, maxDepth, truncated, stats, false, levelsStore<IMatLevels>);
}

int snail_instances_materials_tree_render_frame(SnailInstancesMaterials *m, const float cam[13], int resx, int resy, const float *lights7, int nLights,
												const float ambient[3], int flags, uint8_t *image, int pitch, int maxDepth, uint64_t *truncated, uint64_t stats[4]) {
	const char *fn = "snail_instances_materials_tree_render_frame";
	if(int rc = matTreeArgsOk(fn, cam, resx, resy, lights7, nLights, ambient, flags, nullptr, maxDepth, truncated)) return rc;
	if(!image || pitch < resx * 3) { snail_set_error("%s: null image or a pitch below 3 * resx", fn); return 1; }
	if(int rc = checkIMatAny(m, fn)) return rc;
	return renderFrameHost<IMatLevels>(m, fn, cam, resx, resy, lights7, nLights, ambient, flags, image, pitch, maxDepth, truncated, stats, false, levelsStore<IMatLevels>);
}

int snail_instances_materials_set_level_budget(SnailInstancesMaterials *m, uint64_t bytes) {
	const char *fn = "snail_instances_materials_set_level_budget";
	if(!bytes) { snail_set_error("%s: a budget of 0 bytes", fn); return 1; }
	if(int rc = checkIMatAny(m, fn)) return rc;
	std::lock_guard<std::mutex> lock(m->inst->mu);
	m->levelBudget = bytes;
	return 0;
}

int64_t snail_instances_materials_level_bytes(int nLights, int flags, int maxDepth) {
	if((flags & ~kMatTreeFlags) || nLights < 0 || nLights > SNAIL_MAX_LIGHTS || maxDepth < 1 || maxDepth > SNAIL_MAT_TRANSP_MAX_DEPTH) {
		snail_set_error("snail_instances_materials_level_bytes: unknown bits in flags (0x%x), more than %d lights, or maxDepth %d outside 1..%d", flags, SNAIL_MAX_LIGHTS, maxDepth,
						SNAIL_MAT_TRANSP_MAX_DEPTH);
		return -1;
	}
	return levelsBytesPerPacket<IMatLevels>(nLights, flags, maxDepth);
}

} // extern "C"
