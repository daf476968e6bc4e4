// materials_tree_host.inc -- the C-ABI of include/snail_materials_tree.h: the transparency continuation together with the mirrored bounce, the
// tile renderer, 4x antialiasing, depth shading and the tint; included by snail_hip.hip after materials_transparency_host.inc.  The frames are
// the level driver's (materials_levels_host.inc) for a plain scene (MatLevels, materials_host.inc): shadeLevels with chain B under
// SNAIL_RENDER_REFLECTIONS, run by levelsStore over a packet list in slices that keep the levels within the set's budget.

namespace {

const int kMatTreeFlags = SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_DEPTH | SNAIL_RENDER_AA4;

// everything that can be judged without the handle; the flags first
int matTreeArgsOk(const char *fn, const float *cam, int resx, int resy, const float *lights7, int nLights, const float *ambient, int flags, const float *tint, int maxDepth,
				  const uint64_t *trunc) {
	if(flags & ~kMatTreeFlags) {
		snail_set_error("%s: unknown bits in flags (got 0x%x): SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_DEPTH | SNAIL_RENDER_AA4", fn, flags);
		return 1;
	}
	if(maxDepth < 1 || maxDepth > SNAIL_MAT_TRANSP_MAX_DEPTH) { snail_set_error("%s: maxDepth %d outside 1..%d", fn, maxDepth, SNAIL_MAT_TRANSP_MAX_DEPTH); return 1; }
	if(!trunc) { snail_set_error("%s: null truncated-lane counter", fn); return 1; }
	return matTilesArgsOk(fn, cam, resx, resy, lights7, nLights, ambient, flags, tint);
}

} // namespace

extern "C" {

int snail_materials_mirror_rays_dev(SnailMaterials *m, int nPackets, const float *dOriginIn, const float *dDirIn, const uint8_t *dMaskIn, const float *dT,
									const float *dSamples, const int32_t *dOrderIn, float *dOrigin, float *dDir, float *dIDir, uint8_t *dMask, float *dDistance,
									int32_t *dObject, int32_t *dOrder, uint64_t *dStats, void *stream) {
	const char *fn = "snail_materials_mirror_rays_dev";
	if(int rc = checkMaterialsAny(m, fn)) return rc;
	if(nPackets <= 0) return 0;
	if(!dOriginIn || !dDirIn || !dT || !dSamples || !dOrigin || !dDir || !dIDir || !dMask || !dDistance || !dObject || !dOrder ||
	   !matAligned16({dOriginIn, dDirIn, dT, dSamples, dOrigin, dDir, dIDir, dDistance, dObject})) {
		snail_set_error("%s: a null buffer, or a buffer not 16-byte aligned", fn);
		return 1;
	}
	if(dOrigin == dOriginIn || dDir == dDirIn || dDistance == dT || dMask == dMaskIn) { snail_set_error("%s: the mirrored packets must not be written over the level's own", fn); return 1; }
	DeviceGuard guard(m->device);
	SNAIL_LOCK(m->scene);
	dev::TreeArgs G;
	memset(&G, 0, sizeof(G));
	const float noCam[13] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 1};   // (generic packets carry their rays: no stage of this call generates any)
	matFillArgs(m, G.t.m, noCam, 16, 16, nullptr, nPackets);
	dev::MatArgs &A = G.t.m;
	A.s.rOrg = const_cast<float *>(dOriginIn); A.s.rDir = const_cast<float *>(dDirIn); A.s.rMask = const_cast<uint8_t *>(dMaskIn); A.s.rDist = const_cast<float *>(dT);
	A.nSamples = const_cast<float *>(dSamples);
	G.t.inOrder = dOrderIn;
	G.oOrg = dOrigin; G.oDir = dDir; G.oIDir = dIDir; G.oMask = dMask; G.oDist = dDistance; G.oObj = dObject; G.oOrder = dOrder;
	A.s.stats = (dev::u64 *)dStats;
	const bool sse = m->scene->arith == SNAIL_ARITH_HOST_SSE;
	SNAIL_LAUNCH(sse, TreeArgs, dim3(nPackets), dim3(64), 0, (hipStream_t)stream, G, k_mat_mirror_rays);
	HIP_TRY(hipGetLastError());
	return 0;
}

int snail_materials_tree_frame_packets_dev(SnailMaterials *m, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets, const float *lights7,
										   int nLights, const float ambient[3], int flags, const float *tint, uint8_t *bgrPackets, int maxDepth, uint64_t *dTruncated,
										   uint64_t *dStats, void *stream) {
	const char *fn = "snail_materials_tree_frame_packets_dev";
	if(int rc = matTreeArgsOk(fn, cam, resx, resy, lights7, nLights, ambient, flags, tint, maxDepth, dTruncated)) return rc;
	if(nPackets > 0 && !dPacketXY) { snail_set_error("%s: null packet list", fn); return 1; }
	if(nPackets > (1 << 24)) { snail_set_error("%s: more than 2^24 packets", fn); return 1; }
	if(nPackets > 0 && (!bgrPackets || ((unsigned long long)bgrPackets & 3))) { snail_set_error("%s: null or unaligned output", fn); return 1; }
	if(int rc = checkMaterialsAny(m, fn)) return rc;
	if(nPackets <= 0) return 0;
	DeviceGuard guard(m->device);
	SNAIL_LOCK(m->scene);
	return levelsStore<MatLevels>(m, fn, cam, resx, resy, dPacketXY, nPackets, lights7, nLights, ambient, flags, tint, bgrPackets, nullptr, maxDepth, dTruncated, dStats, (hipStream_t)stream);
}

int snail_materials_tree_render_tiles(SnailMaterials *m, const float cam[13], int resx, int resy, const int32_t *coords, const int64_t *offsets, int nTiles,
									  const float *lights7, int nLights, const float ambient[3], int flags, const float *tint, uint8_t *data, int maxDepth,
									  uint64_t *truncated, uint64_t stats[4]) {
	const char *fn = "snail_materials_tree_render_tiles";
	if(int rc = matTreeArgsOk(fn, cam, resx, resy, lights7, nLights, ambient, flags, tint, maxDepth, truncated)) return rc;
	if(nTiles > 0 && (!coords || !offsets || !data)) { snail_set_error("%s: null buffer", fn); return 1; }
	if(int rc = tileRectsOk(fn, coords, nTiles)) return rc;
	if(int rc = checkMaterialsAny(m, fn)) return rc;
	if(nTiles <= 0) return 0;
	return renderTilesHost<MatLevels>(m, fn, cam, resx, resy, coords, offsets, nTiles, lights7, nLights, ambient, flags, tint, data, maxDepth, truncated, stats, false, levelsStore<MatLevels>);
}

int snail_materials_tree_render_frame(SnailMaterials *m, const float cam[13], int resx, int resy, const float *lights7, int nLights, const float ambient[3], int flags,
									  uint8_t *image, int pitch, int maxDepth, uint64_t *truncated, uint64_t stats[4]) {
	const char *fn = "snail_materials_tree_render_frame";
	if(int rc = matTreeArgsOk(fn, cam, resx, resy, lights7, nLights, ambient, flags, nullptr, maxDepth, truncated)) return rc;
	if(!image || pitch < resx * 3) { snail_set_error("%s: null image or a pitch below 3 * resx", fn); return 1; }
	if(int rc = checkMaterialsAny(m, fn)) return rc;
	return renderFrameHost<MatLevels>(m, fn, cam, resx, resy, lights7, nLights, ambient, flags, image, pitch, maxDepth, truncated, stats, false, levelsStore<MatLevels>);
}

int snail_materials_set_level_budget(SnailMaterials *m, uint64_t bytes) {
	const char *fn = "snail_materials_set_level_budget";
	if(int rc = checkMaterialsAny(m, fn)) return rc;
	if(!bytes) { snail_set_error("%s: a budget of 0 bytes", fn); return 1; }
	SNAIL_LOCK(m->scene);
	m->levelBudget = bytes;
	return 0;
}

int64_t snail_materials_level_bytes(int nLights, int flags, int maxDepth) {
	if((flags & ~kMatTreeFlags) || nLights < 0 || nLights > SNAIL_MAX_LIGHTS || maxDepth < 1 || maxDepth > SNAIL_MAT_TRANSP_MAX_DEPTH) {
		snail_set_error("snail_materials_level_bytes: unknown bits in flags (0x%x), more than %d lights, or maxDepth %d outside 1..%d", flags, SNAIL_MAX_LIGHTS, maxDepth, SNAIL_MAT_TRANSP_MAX_DEPTH);
		return -1;
	}
	return levelsBytesPerPacket<MatLevels>(nLights, flags, maxDepth);
}

} // extern "C"
