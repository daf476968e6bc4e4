// materials_host.inc -- the C-ABI of include/snail_materials.h: ShTriangle records and mip chains on the host, the material set of a plain
// scene, and the staged launches of materials.inc (primary hits -> k_mat_sample -> k_mat_light per (packet, light) -> k_mat_final); and the
// C-ABI of include/snail_materials_bounce.h: the same frames with the one mirrored bounce of gVals[7] (-> k_mat_mirror -> launchRays with
// barycentrics -> k_mat_sample_rays -> k_mat_light_rays -> k_mat_colour_rays between the sample stage and the primary lights, k_mat_final_blend last).
// The handle's sets of intermediates and frame lists are shading_sets_host.inc's; the frames' bodies from DeviceGuard on are materials_levels_host.inc's
// (frameDev, framePacketsDev, frameImage), included ahead of this file, over MatLevels, the plain scene's kind, defined here beside matShade.
#include "../../include/snail_materials.h"
#include "../../include/snail_materials_bounce.h"
#include "../../include/snail_materials_tiles.h"

struct SnailMaterialsDyn;   // materials_dynamic_host.inc: what a set of snail_materials_create_dev carries besides the set
namespace { int dynCheckFresh(const SnailMaterials *, const char *fn); void dynFree(SnailMaterialsDyn *); }
struct SnailMaterials : ShadeSets {   // (shading_sets_host.inc: the sets of intermediates, the frame lists, the tile job, the level budget)
	SnailScene *scene = nullptr;
	SnailMaterialsDyn *dyn = nullptr;   // snail_materials_create_dev: the records are packed on the device and follow the scene's rebuilds
	int device = 0;
	int nTris = 0, nMap = 0, nMats = 0, nTex = 0;
	bool canSelectTransparent = false;   // holds SNAIL_MAT_TRANSPARENT or UBER with 0 < dissolve < 1 (snail_materials_create_transparent alone makes such a set)
	char *dBase = nullptr;   // ONE allocation: records, map, materials, texture descriptors, texels
	const uint4 *dShTris = nullptr;
	const int *dMap = nullptr;
	const dev::MatRec *dMats = nullptr;
	const dev::TexRec *dTex = nullptr;
	const unsigned char *dTexels = nullptr;
	// a set's base part: the intermediates of the lit frames
	struct Bufs {
		float *hitT = nullptr, *hitU = nullptr, *hitV = nullptr, *samples = nullptr, *sDist = nullptr;
		int *hitId = nullptr;
		static size_t bytes(size_t np, int nLights) { return np * 256 * 4 * (size_t)(4 + 9 + (nLights > 0 ? nLights : 0)); }
		void carve(char *base, size_t np) {
			const size_t plane = np * 256 * 4;
			hitT = (float *)base; hitU = (float *)(base + plane); hitV = (float *)(base + 2 * plane); hitId = (int *)(base + 3 * plane);
			samples = (float *)(base + 4 * plane); sDist = (float *)(base + 13 * plane);
		}
	};
	// ... and those of the bounce: the mirrored packets (rays, mask, distance, object, bary), the nested samples, colour and shadow distances
	struct BounceBufs {
		float *rOrg = nullptr, *rDir = nullptr, *rIDir = nullptr, *rDist = nullptr, *bary = nullptr, *nSamples = nullptr, *rCol = nullptr, *nSDist = nullptr;
		int *rObj = nullptr;
		unsigned char *rMask = nullptr;
		static size_t bytes(size_t np, int nLights) { return np * 256 * 4 * (size_t)(25 + (nLights > 0 ? nLights : 0)) + ((np * 64 + 255) & ~(size_t)255); }
		void carve(char *base, size_t np, int nLights) {
			const size_t plane = np * 256 * 4;
			rOrg = (float *)base; rDir = (float *)(base + 3 * plane); rIDir = (float *)(base + 6 * plane); rDist = (float *)(base + 9 * plane);
			rObj = (int *)(base + 10 * plane); bary = (float *)(base + 11 * plane); nSamples = (float *)(base + 13 * plane); rCol = (float *)(base + 22 * plane);
			nSDist = (float *)(base + 25 * plane);
			rMask = (unsigned char *)(base + (size_t)(25 + (nLights > 0 ? nLights : 0)) * plane);
		}
	};
	// ... and the tile renderer's (materials_tiles_host.inc, levelsStore): the packets' float colours and, under 4x antialiasing, the sub-packet list
	struct TileBufs {
		float *col = nullptr;
		int32_t *xy2 = nullptr;
		static size_t bytes(size_t np) { return np * 256 * 12 + np * 8; }
		void carve(char *base, size_t np) { col = (float *)base; xy2 = (int32_t *)(base + np * 256 * 12); }
	};
};

namespace {

bool matPow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
int matTexLevels(int w, int h) {
	int m = w > h ? w : h, l = 0;
	while((1 << l) < m) l++;
	return l + 1;   // min(32, Log2(max(w, h)) + 1), src/mipmap_texture.cpp:106
}
size_t matLevelBytes(int w, int h, int m) {
	const size_t lw = (size_t)std::max(w >> m, 1), lh = (size_t)std::max(h >> m, 1);
	return 3 * lw * lh;
}
bool matTexShapeOK(int w, int h) { return matPow2(w) && matPow2(h) && w <= 8192 && h <= 8192; }

// any set: the entry points of include/snail_materials_transparency.h
int checkMaterialsAny(const SnailMaterials *m, const char *fn) {
	if(!m || !m->scene || !m->dBase) { snail_set_error("%s: invalid material set handle", fn); return 1; }
	if(int rc = checkScene(m->scene, fn)) return rc;
	return m->dyn ? dynCheckFresh(m, fn) : 0;   // (include/snail_materials_dynamic.h, "staleness"; the scene's mu is not held here)
}
// the entry points of snail_materials.h, _bounce.h and _tiles.h: their kernels know neither the transparent kind nor the selector
int checkMaterials(const SnailMaterials *m, const char *fn) {
	if(m && m->canSelectTransparent) {
		snail_set_error("%s: the set holds a material that can select a transparent lane, which this function's kernels do not know (include/snail_materials_transparency.h)", fn);
		return 1;
	}
	return checkMaterialsAny(m, fn);
}
int checkMatFrameArgs(const char *fn, const float cam[13], int resx, int resy, const float *lights7, int nLights, const float ambient[3], int flags) {
	if(flags) { snail_set_error("%s: flags must be 0 (got 0x%x): no bounce, transparency or antialiasing under full shading yet", fn, flags); return 1; }
	if(!cam || resx <= 0 || resy <= 0 || nLights < 0 || nLights > SNAIL_MAX_LIGHTS || (nLights && !lights7) || !ambient) {
		snail_set_error("%s: bad arguments (camera, resolution, at most %d lights, ambient)", fn, SNAIL_MAX_LIGHTS);
		return 1;
	}
	return 0;
}

void matFillArgs(const SnailMaterials *m, dev::MatArgs &A, const float cam[13], int resx, int resy, const int32_t *dXY, int np) {
	const SnailScene *s = m->scene;
	memset(&A, 0, sizeof(A));
	A.s.hostTab = s->arith == SNAIL_ARITH_HOST_SSE ? s->dTab : nullptr;
	A.s.nodes = s->dNodes; A.s.tris = s->dTris; A.s.pf = (const uint4 *)s->dPF;
	A.s.g = makeGen(cam, resx, resy);
	A.s.resx = resx; A.s.resy = resy; A.s.pw = (resx + 15) / 16; A.s.ph = (resy + 15) / 16;
	A.s.fastOK = s->fastOK && originSane(cam);
	A.s.pack = stackPack(s);
	A.s.packetXY = (const int2 *)dXY; A.s.nPackets = np; A.s.nBlocks = np;
	A.shtris = m->dShTris; A.nTris = m->nTris;
	A.matMap = m->dMap; A.nMap = m->nMap;
	A.mats = m->dMats; A.nMats = m->nMats;
	A.tex = m->dTex; A.texels = m->dTexels;
}

// the stages of one lit frame over the packet list dXY into `frame` (or packet-major `bgrPackets`), intermediates in W; the scene's mu held.
// R (or null): the intermediates of the one mirrored bounce -- primary -> sample -> mirror -> launchRays -> nested sample -> nested lights ->
// nested colour -> primary lights -> blend and store.
int matShade(SnailMaterials *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights,
			 const float ambient[3], uint8_t *frame, int pitch, uint8_t *bgrPackets, const SnailMaterials::Bufs &W, const SnailMaterials::BounceBufs *R,
			 uint64_t *dStats, hipStream_t st, float *colPackets = nullptr) {
	SnailScene *s = m->scene;
	SceneUse use(s, st);
	if(use.rc) return use.rc;
	if(int rc = launchPrimary(s, cam, resx, resy, 0, 0, 0, 0, dXY, np, W.hitT, W.hitU, W.hitV, W.hitId, dStats, st)) return rc;
	dev::MatArgs A;
	matFillArgs(m, A, cam, resx, resy, dXY, np);
	A.s.nLights = nLights;
	for(int n = 0; n < nLights; n++) for(int k = 0; k < 7; k++) A.s.lights[n][k] = lights7[n * 7 + k];
	for(int c = 0; c < 3; c++) { A.s.ambient[c] = ambient[c]; A.s.color[c] = 1.0f; }
	A.s.hitT = W.hitT; A.s.hitId = W.hitId; A.hitU = W.hitU; A.hitV = W.hitV;
	A.samples = W.samples; A.s.sDist = W.sDist;
	A.s.frame = frame; A.s.pitch = pitch; A.s.bgrPackets = bgrPackets;
	A.s.colPackets = colPackets;   // the float colours k_inst_store goes on from, instead of bytes (k_mat_colour / k_mat_colour_blend)
	A.s.stats = (dev::u64 *)dStats;
	if(R) {
		A.s.rOrg = R->rOrg; A.s.rDir = R->rDir; A.s.rIDir = R->rIDir; A.s.rMask = R->rMask; A.s.rDist = R->rDist; A.s.rObj = R->rObj; A.s.rCol = R->rCol;
		A.rU = R->bary; A.rV = R->bary + 4; A.rUVStride = 8;
		A.nSamples = R->nSamples; A.nSDist = R->nSDist;
		A.s.blend = 1;
	}
	const bool sse = s->arith == SNAIL_ARITH_HOST_SSE;
	const dim3 grid(np), wave(64);
	SNAIL_LAUNCH(sse, MatArgs, grid, wave, 0, st, A, k_mat_sample);
	HIP_TRY(hipGetLastError());
	if(R) {
		SNAIL_LAUNCH(sse, MatArgs, grid, wave, 0, st, A, k_mat_mirror);
		HIP_TRY(hipGetLastError());
		// the walk reads the barycentrics it was given and writes them back for lanes without a hit: zeros, not what the buffer last held
		HIP_TRY(hipMemsetAsync(R->bary, 0, (size_t)np * 256 * 8, st));
		if(int rc = launchRays(s, false, np, 64, 0, R->rOrg, R->rDir, R->rIDir, R->rMask, R->rDist, R->rObj, R->bary, dStats, st)) return rc;
		SNAIL_LAUNCH(sse, MatArgs, grid, wave, 0, st, A, k_mat_sample_rays);
		HIP_TRY(hipGetLastError());
	}
	int lrc = 0;
	if(nLights) {
		int relWhich[SNAIL_MAX_LIGHTS];
		for(int n = 0; n < SNAIL_MAX_LIGHTS; n++) { relWhich[n] = -1; A.s.relLight[n] = nullptr; }
		// every origin-relative copy taken here is booked as used on st on EVERY way out (first error kept): a copy whose fill was enqueued must not
		// be recycled under it, whether or not the walk that wanted it was launched.  The nested lights walk from the same origins: the same copies.
		if(A.s.pack && !useDeep(s))
			for(int n = 0; n < nLights && !lrc; n++) lrc = relFor(s, A.s.lights[n], st, &A.s.relLight[n], &relWhich[n]);
		const dim3 lgrid(np, nLights);
		if(!lrc && R) {
			if(useDeep(s)) SNAIL_LAUNCH(sse, MatArgs, lgrid, wave, 0, st, A, k_mat_light_rays<true>);
			else SNAIL_LAUNCH(sse, MatArgs, lgrid, wave, 0, st, A, k_mat_light_rays<false>);
			const hipError_t e = hipGetLastError();
			if(e != hipSuccess) { snail_set_error("%s: k_mat_light_rays: %s", fn, hipGetErrorString(e)); lrc = 100 + (int)e; }
		}
		if(!lrc && R) {
			SNAIL_LAUNCH(sse, MatArgs, grid, wave, 0, st, A, k_mat_colour_rays);
			const hipError_t e = hipGetLastError();
			if(e != hipSuccess) { snail_set_error("%s: k_mat_colour_rays: %s", fn, hipGetErrorString(e)); lrc = 100 + (int)e; }
		}
		if(!lrc) {
			if(useDeep(s)) SNAIL_LAUNCH(sse, MatArgs, lgrid, wave, 0, st, A, k_mat_light<true>);
			else SNAIL_LAUNCH(sse, MatArgs, lgrid, wave, 0, st, A, k_mat_light<false>);
			const hipError_t e = hipGetLastError();
			if(e != hipSuccess) { snail_set_error("%s: k_mat_light: %s", fn, hipGetErrorString(e)); lrc = 100 + (int)e; }
		}
		for(int n = 0; n < nLights; n++)
			if(relWhich[n] >= 0) { const int urc = relUsed(s, relWhich[n], st); if(!lrc) lrc = urc; }
		if(lrc) return lrc;
	} else if(R) {
		SNAIL_LAUNCH(sse, MatArgs, grid, wave, 0, st, A, k_mat_colour_rays);
		HIP_TRY(hipGetLastError());
	}
	if(colPackets) {
		if(R) SNAIL_LAUNCH(sse, MatArgs, grid, wave, 0, st, A, k_mat_colour_blend);
		else SNAIL_LAUNCH(sse, MatArgs, grid, wave, 0, st, A, k_mat_colour);
	} else if(R) SNAIL_LAUNCH(sse, MatArgs, grid, wave, 0, st, A, k_mat_final_blend);
	else SNAIL_LAUNCH(sse, MatArgs, grid, wave, 0, st, A, k_mat_final);
	HIP_TRY(hipGetLastError());
	return 0;
}

// materials_tiles_host.inc: the opaque stages with any flags and tint into packet-major bytes or a tile job's planes
int matShadeStore(SnailMaterials *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights,
				  const float ambient[3], int flags, const float *tint, uint8_t *bgrPackets, const InstTileJob *J, uint64_t *dStats, hipStream_t st);

// The plain scene's kind of the frame bodies and the level driver (materials_levels_host.inc); the scene's mu held.  The scene-free stages'
// TreeArgs is the only argument record: its MatArgs is the frame's, and the sample and light stages take its TranspArgs.
struct MatLevels : LevelsFrame {
	typedef SnailMaterials Handle;
	typedef SnailMaterials::Bufs Bufs;
	typedef SnailMaterials::BounceBufs BounceBufs;
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
	// the handle's part of the frame bodies, of levelsStore and of the host calls
	static int opaque(SnailMaterials *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights,
					  const float ambient[3], uint8_t *frame, int pitch, uint8_t *bgrPackets, const Bufs &W, const BounceBufs *R, uint64_t *dStats, hipStream_t st) {
		return matShade(m, fn, cam, resx, resy, dXY, np, lights7, nLights, ambient, frame, pitch, bgrPackets, W, R, dStats, st);
	}
	static int depthStore(SnailMaterials *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights,
						  const float ambient[3], int flags, const float *tint, uint8_t *bgrPackets, const InstTileJob *J, uint64_t *dStats, hipStream_t st) {
		return matShadeStore(m, fn, cam, resx, resy, dXY, np, lights7, nLights, ambient, flags, tint, bgrPackets, J, dStats, st);
	}
	static SnailScene *scene(SnailMaterials *m) { return m->scene; }
	static std::mutex &mu(SnailMaterials *m) { return m->scene->mu; }
};

} // namespace

extern "C" {

int snail_shtris_pack(const float *uv6, const float *nrm9, const int32_t *matIdx, const uint8_t *flat, int n, const int32_t *perm, void *out64) {
	if(n < 0 || (n && (!uv6 || !nrm9 || !matIdx || !out64))) { snail_set_error("snail_shtris_pack: null array"); return 1; }
	for(int i = 0; i < n; i++) {
		const int src = perm ? perm[i] : i;
		if(src < 0 || src >= n) { snail_set_error("snail_shtris_pack: perm[%d] = %d is outside 0..%d", i, src, n - 1); return 1; }
		const float *uv = uv6 + (size_t)src * 6, *nr = nrm9 + (size_t)src * 9;
		for(int k = 0; k < 6; k++)
			if(!(std::fabs(uv[k]) < 1048576.0f)) { snail_set_error("snail_shtris_pack: triangle %d: texture coordinate not finite or not below 2^20", src); return 1; }
		for(int k = 0; k < 9; k++)
			if(!std::isfinite(nr[k])) { snail_set_error("snail_shtris_pack: triangle %d: normal not finite", src); return 1; }
		if(matIdx[src] < 0) { snail_set_error("snail_shtris_pack: triangle %d: negative material index", src); return 1; }
		float o[15];
		// the ShTriangle constructor (src/triangle.h:188-208): elements 1 and 2 minus element 0, in fp32
		o[0] = uv[0]; o[1] = uv[1];
		o[2] = uv[2] - uv[0]; o[3] = uv[3] - uv[1];
		o[4] = uv[4] - uv[0]; o[5] = uv[5] - uv[1];
		for(int c = 0; c < 3; c++) { o[6 + c] = nr[c]; o[9 + c] = nr[3 + c] - nr[c]; o[12 + c] = nr[6 + c] - nr[c]; }
		char *rec = (char *)out64 + (size_t)i * 64;
		memcpy(rec, o, 60);
		const uint32_t id = (uint32_t)matIdx[src] | ((flat && flat[src]) ? 0x80000000u : 0u);
		memcpy(rec + 60, &id, 4);
	}
	return 0;
}

int64_t snail_texture_size(int w, int h, int *nLevels) {
	if(nLevels) *nLevels = 0;
	if(!matTexShapeOK(w, h)) return 0;
	const int levels = matTexLevels(w, h);
	size_t total = 0;
	for(int m = 0; m < levels; m++) total += matLevelBytes(w, h, m);
	if(nLevels) *nLevels = levels;
	return (int64_t)total;
}

int snail_texture_build(const uint8_t *level0, int w, int h, uint8_t *out, int64_t cap, int *nLevels) {
	if(!matTexShapeOK(w, h)) { snail_set_error("snail_texture_build: %d x %d: width and height must be powers of two of at most 8192", w, h); return 1; }
	int levels = 0;
	const int64_t total = snail_texture_size(w, h, &levels);
	if(!level0 || !out || cap < total) { snail_set_error("snail_texture_build: null buffer, or fewer than the %lld bytes of a %d x %d texture", (long long)total, w, h); return 1; }
	memcpy(out, level0, (size_t)w * h * 3);
	// What MipmapTexture::GenMip computes for rgb8 (src/mipmap_texture.cpp:256-285), level by level inside the one buffer, by byte index:
	//   one row on both levels (:259-265)   pixel x, channel c = (lo[6x + c] + lo[6x + 4 + c]) / 2 -- the partner byte is 4 on, not 3 (the rgba8
	//                                        stride), so channels mix across the pair and the last pair's blue reads lo[6x + 6]: the first byte of
	//                                        the level being written (already stored: channels go in order), which follows in this buffer
	//   one column on both levels (:266-272) the byte and the one a row below, / 2
	//   otherwise (:273-283)                 the 2 x 2 block's four bytes of the channel, / 4
	// Sums in unsigned, integer division.  (lo and hi alias one buffer on purpose: no restrict, stores in the order x, then channel.)
	size_t at = 0;   // first byte of the level read
	for(int m = 1; m < levels; m++) {
		const size_t loW = (size_t)std::max(w >> (m - 1), 1), loH = (size_t)std::max(h >> (m - 1), 1);
		const size_t hiW = (size_t)std::max(w >> m, 1), hiH = (size_t)std::max(h >> m, 1);
		const size_t loRow = 3 * loW, hiRow = 3 * hiW;
		const uint8_t *lo = out + at;
		uint8_t *hi = out + at + loRow * loH;
		if(loH == hiH) {
			for(size_t x = 0; x < hiW; x++)
				for(size_t c = 0; c < 3; c++) hi[3 * x + c] = (uint8_t)(((unsigned)lo[6 * x + c] + (unsigned)lo[6 * x + 4 + c]) / 2u);
		} else if(loW == hiW) {
			for(size_t y = 0; y < hiH; y++)
				for(size_t c = 0; c < 3; c++) hi[y * hiRow + c] = (uint8_t)(((unsigned)lo[2 * y * loRow + c] + (unsigned)lo[(2 * y + 1) * loRow + c]) / 2u);
		} else {
			for(size_t y = 0; y < hiH; y++)
				for(size_t x = 0; x < hiW; x++) {
					const uint8_t *q = lo + 2 * y * loRow + 6 * x;   // the block's upper left pixel
					for(size_t c = 0; c < 3; c++)
						hi[y * hiRow + 3 * x + c] = (uint8_t)(((unsigned)q[c] + (unsigned)q[3 + c] + (unsigned)q[loRow + c] + (unsigned)q[loRow + 3 + c]) / 4u);
				}
		}
		at += loRow * loH;
	}
	if(nLevels) *nLevels = levels;
	return 0;
}

} // extern "C"

// the creators: snail_materials_create (transp = false: its refusals), snail_materials_create_transparent (include/snail_materials_transparency.h)
// and snail_materials_create_dev (include/snail_materials_dynamic.h).  matCheckHost: what they judge on the caller's HOST data, before a device
// is touched (dynamic: the records are made on the device, there is no shtris64); matUpload: the device copy.
static bool matCheckHost(const char *fn, bool transp, bool dynamic, const void *shtris64, int nTris, const int32_t *matMap, int nMap, const SnailMaterial *mats, int nMats,
						 const int32_t *opacityTexture, const SnailTexture *textures, int nTex, bool *canSelectOut) {
	bool canSelect = false;
	if(nTris <= 0 || nMap <= 0 || nMats < 0 || nTex < 0 || (!dynamic && !shtris64) || !matMap || (nMats && !mats) || (nTex && !textures)) {
		snail_set_error("%s: bad counts or null arrays (at least one triangle and one map entry)", fn);
		return false;
	}
	for(int k = 0; k < nTex; k++) {
		if(!matTexShapeOK(textures[k].width, textures[k].height)) {
			snail_set_error("%s: texture %d is %d x %d: width and height must be powers of two of at most 8192", fn, k, textures[k].width, textures[k].height);
			return false;
		}
		if(!textures[k].levels) { snail_set_error("%s: texture %d has no texels", fn, k); return false; }
	}
	for(int k = 0; k < nMats; k++) {
		const SnailMaterial &M = mats[k];
		if(M.kind == SNAIL_MAT_TRANSPARENT && !transp) { snail_set_error("%s: material %d is of the transparent kind: transparency under full shading stays with the host renderer", fn, k); return false; }
		if(M.kind != SNAIL_MAT_SIMPLE && M.kind != SNAIL_MAT_TEX && M.kind != SNAIL_MAT_UBER && M.kind != SNAIL_MAT_TRANSPARENT) { snail_set_error("%s: material %d: unknown kind %d", fn, k, M.kind); return false; }
		if(M.kind == SNAIL_MAT_UBER && !transp && !(M.dissolve <= 0.0f || M.dissolve >= 1.0f)) {
			snail_set_error("%s: material %d: UBER with dissolve %g could select a transparent lane (accepted: dissolve <= 0 or >= 1)", fn, k, (double)M.dissolve);
			return false;
		}
		if(M.kind == SNAIL_MAT_UBER && std::isnan(M.dissolve)) { snail_set_error("%s: material %d: UBER with a NaN dissolve", fn, k); return false; }   // (transp: the other creator has refused it above)
		if(M.kind == SNAIL_MAT_TRANSPARENT) {
			if(M.texture < 0 || M.texture >= nTex) { snail_set_error("%s: material %d: texture index %d outside 0..%d", fn, k, M.texture, nTex - 1); return false; }
			if(!opacityTexture) { snail_set_error("%s: material %d is of the transparent kind and the opacity texture array is null", fn, k); return false; }
			if(opacityTexture[k] < 0 || opacityTexture[k] >= nTex) { snail_set_error("%s: material %d: opacity texture index %d outside 0..%d", fn, k, opacityTexture[k], nTex - 1); return false; }
			canSelect = true;
		}
		if(M.kind == SNAIL_MAT_UBER && M.dissolve > 0.0f && M.dissolve < 1.0f) canSelect = true;
		if(M.kind == SNAIL_MAT_TEX && (M.texture < 0 || M.texture >= nTex)) { snail_set_error("%s: material %d: texture index %d outside 0..%d", fn, k, M.texture, nTex - 1); return false; }
	}
	for(int k = 0; k < nMap; k++)
		if(matMap[k] < -1 || matMap[k] >= nMats) { snail_set_error("%s: map entry %d = %d is outside -1..%d", fn, k, matMap[k], nMats - 1); return false; }
	for(int i = 0; i < nTris && !dynamic; i++) {
		uint32_t id;
		memcpy(&id, (const char *)shtris64 + (size_t)i * 64 + 60, 4);
		if((int)(id & 0x7fffffffu) >= nMap) { snail_set_error("%s: record %d: material index %u outside the map of %d entries", fn, i, id & 0x7fffffffu, nMap); return false; }
	}
	*canSelectOut = canSelect;
	return true;
}

// The device form of a checked material and texture list (the creators here and snail_instances_materials_create): one MatRec per material, one
// TexRec per texture with its levels' offsets -> the bytes the texels take, every texture's base set.  opacityTexture: read for the
// transparent kind alone.
static size_t matPackLists(const SnailMaterial *mats, int nMats, const int32_t *opacityTexture, const SnailTexture *textures, int nTex, std::vector<dev::MatRec> &recs,
						   std::vector<dev::TexRec> &trecs) {
	recs.assign((size_t)std::max(nMats, 1), dev::MatRec());
	memset(recs.data(), 0, recs.size() * sizeof(dev::MatRec));
	for(int k = 0; k < nMats; k++) {
		dev::MatRec &R = recs[k];
		R.kind = mats[k].kind; R.ndotr = mats[k].nDotR ? 1 : 0; R.tex = (mats[k].kind == SNAIL_MAT_TEX || mats[k].kind == SNAIL_MAT_TRANSPARENT) ? mats[k].texture : 0;
		// the padding, read by the kernels of materials_transparency.inc alone: the opacity map, and the dissolve factor's bits
		R.pad[0] = mats[k].kind == SNAIL_MAT_TRANSPARENT ? opacityTexture[k] : 0;
		memcpy(&R.pad[1], &mats[k].dissolve, 4);
		for(int c = 0; c < 3; c++) { R.col[c] = mats[k].diffuse[c]; R.spec[c] = mats[k].specular[c]; }
		if(mats[k].kind == SNAIL_MAT_UBER) std::swap(R.col[0], R.col[2]);   // UberMaterial::UberMaterial: Swap(diffuse.x, diffuse.z)
	}
	trecs.assign((size_t)std::max(nTex, 1), dev::TexRec());
	memset(trecs.data(), 0, trecs.size() * sizeof(dev::TexRec));
	size_t texelBytes = 0;
	for(int k = 0; k < nTex; k++) {
		dev::TexRec &T = trecs[k];
		T.base = texelBytes; T.w = textures[k].width; T.h = textures[k].height; T.mips = matTexLevels(T.w, T.h);
		size_t off = 0;
		for(int l = 0; l < T.mips; l++) { T.lvl[l] = (unsigned)off; off += matLevelBytes(T.w, T.h, l); }
		texelBytes += (off + 4 + 15) & ~(size_t)15;   // 4 bytes of padding: a tap may be read as 4 bytes
	}
	return texelBytes;
}

// shtris64 null: the records' room is left zeroed (snail_materials_create_dev packs them on the device)
static SnailMaterials *matUpload(const char *fn, bool canSelect, SnailScene *scene, const void *shtris64, int nTris, const int32_t *matMap, int nMap, const SnailMaterial *mats,
								 int nMats, const int32_t *opacityTexture, const SnailTexture *textures, int nTex) {
	if(checkScene(scene, fn)) return nullptr;
	if(nTris != scene->nTris) { snail_set_error("%s: %d records for a scene of %d triangles", fn, nTris, scene->nTris); return nullptr; }

	// the device copy
	std::vector<dev::MatRec> recs;
	std::vector<dev::TexRec> trecs;
	const size_t texelBytes = matPackLists(mats, nMats, opacityTexture, textures, nTex, recs, trecs);
	typedef HostCallScope H;
	const size_t oTris = 0, oMap = oTris + H::pad((size_t)nTris * 64), oMats = oMap + H::pad((size_t)nMap * 4), oTex = oMats + H::pad(recs.size() * sizeof(dev::MatRec)),
				 oTexels = oTex + H::pad(trecs.size() * sizeof(dev::TexRec)), total = oTexels + H::pad(texelBytes + 16);
	DeviceGuard guard(scene->device);
	char *base = nullptr;
	hipError_t e = hipMalloc((void **)&base, total);
	if(e == hipSuccess) e = hipMemset(base, 0, total);
	if(e == hipSuccess && shtris64) e = hipMemcpy(base + oTris, shtris64, (size_t)nTris * 64, hipMemcpyHostToDevice);
	if(e == hipSuccess) e = hipMemcpy(base + oMap, matMap, (size_t)nMap * 4, hipMemcpyHostToDevice);
	if(e == hipSuccess) e = hipMemcpy(base + oMats, recs.data(), recs.size() * sizeof(dev::MatRec), hipMemcpyHostToDevice);
	if(e == hipSuccess) e = hipMemcpy(base + oTex, trecs.data(), trecs.size() * sizeof(dev::TexRec), hipMemcpyHostToDevice);
	for(int k = 0; k < nTex && e == hipSuccess; k++)
		e = hipMemcpy(base + oTexels + trecs[k].base, textures[k].levels, (size_t)snail_texture_size(trecs[k].w, trecs[k].h, nullptr), hipMemcpyHostToDevice);
	if(e != hipSuccess) {
		snail_set_error("%s: device copy failed: %s", fn, hipGetErrorString(e));
		if(base) (void)hipFree(base);
		return nullptr;
	}
	SnailMaterials *m = new SnailMaterials();
	m->scene = scene; m->device = scene->device;
	m->nTris = nTris; m->nMap = nMap; m->nMats = nMats; m->nTex = nTex;
	m->dBase = base;
	m->canSelectTransparent = canSelect;
	m->dShTris = (const uint4 *)(base + oTris); m->dMap = (const int *)(base + oMap); m->dMats = (const dev::MatRec *)(base + oMats);
	m->dTex = (const dev::TexRec *)(base + oTex); m->dTexels = (const unsigned char *)(base + oTexels);
	return m;
}

static SnailMaterials *matCreate(const char *fn, bool transp, SnailScene *scene, const void *shtris64, int nTris, const int32_t *matMap, int nMap, const SnailMaterial *mats,
								 int nMats, const int32_t *opacityTexture, const SnailTexture *textures, int nTex) {
	bool canSelect = false;
	if(!matCheckHost(fn, transp, false, shtris64, nTris, matMap, nMap, mats, nMats, opacityTexture, textures, nTex, &canSelect)) return nullptr;
	return matUpload(fn, canSelect, scene, shtris64, nTris, matMap, nMap, mats, nMats, opacityTexture, textures, nTex);
}

extern "C" {

SnailMaterials *snail_materials_create(SnailScene *scene, const void *shtris64, int nTris, const int32_t *matMap, int nMap, const SnailMaterial *mats, int nMats,
									   const SnailTexture *textures, int nTex) {
	return matCreate("snail_materials_create", false, scene, shtris64, nTris, matMap, nMap, mats, nMats, nullptr, textures, nTex);
}

void snail_materials_destroy(SnailMaterials *m) {
	if(!m) return;
	DeviceGuard guard(m->device);
	(void)hipDeviceSynchronize();
	m->release();
	if(m->dBase) (void)hipFree(m->dBase);
	dynFree(m->dyn);
	delete m;
}

int snail_materials_shade_packets_dev(SnailMaterials *m, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets, const float *dT,
									  const float *dU, const float *dV, const int32_t *dTriId, float *dSamples, void *stream) {
	const char *fn = "snail_materials_shade_packets_dev";
	if(int rc = checkMaterials(m, fn)) return rc;
	if(nPackets <= 0) return 0;
	if(!cam || resx <= 0 || resy <= 0 || !dPacketXY || !dT || !dU || !dV || !dTriId || !dSamples || ((unsigned long long)dSamples & 15)) {
		snail_set_error("%s: bad camera or resolution, a null buffer, or samples not 16-byte aligned", fn);
		return 1;
	}
	DeviceGuard guard(m->device);
	SNAIL_LOCK(m->scene);
	dev::MatArgs A;
	matFillArgs(m, A, cam, resx, resy, dPacketXY, nPackets);
	A.s.hitT = dT; A.s.hitId = dTriId; A.hitU = dU; A.hitV = dV;
	A.samples = dSamples;
	const bool sse = m->scene->arith == SNAIL_ARITH_HOST_SSE;
	SNAIL_LAUNCH(sse, MatArgs, dim3(nPackets), dim3(64), 0, (hipStream_t)stream, A, k_mat_sample);
	HIP_TRY(hipGetLastError());
	return 0;
}

} // extern "C"

// include/snail_materials_bounce.h: flags = 0 or SNAIL_RENDER_REFLECTIONS, judged before anything else
static int checkBounceFrameArgs(const char *fn, const float cam[13], int resx, int resy, const float *lights7, int nLights, const float ambient[3], int flags) {
	if(flags & ~SNAIL_RENDER_REFLECTIONS) {
		snail_set_error("%s: flags must be 0 or SNAIL_RENDER_REFLECTIONS (got 0x%x): no depth shading, transparency or antialiasing under full shading", fn, flags);
		return 1;
	}
	return checkMatFrameArgs(fn, cam, resx, resy, lights7, nLights, ambient, 0);
}

extern "C" {

int snail_render_materials_dev(SnailMaterials *m, const float cam[13], int resx, int resy, const float *lights7, int nLights, const float ambient[3], int flags,
							   uint8_t *frame, int pitch, uint64_t *dStats, void *stream) {
	const char *fn = "snail_render_materials_dev";
	if(int rc = checkMatFrameArgs(fn, cam, resx, resy, lights7, nLights, ambient, flags)) return rc;
	if(int rc = checkMaterials(m, fn)) return rc;
	if(!frame || pitch < resx * 3) { snail_set_error("%s: null frame or a pitch below 3 * resx", fn); return 1; }
	return frameDev<MatLevels>(m, fn, cam, resx, resy, lights7, nLights, ambient, false, 0, frame, pitch, nullptr, dStats, stream);
}

int snail_render_materials_packets_dev(SnailMaterials *m, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets, const float *lights7,
									   int nLights, const float ambient[3], int flags, uint8_t *bgrPackets, uint64_t *dStats, void *stream) {
	const char *fn = "snail_render_materials_packets_dev";
	if(int rc = checkMatFrameArgs(fn, cam, resx, resy, lights7, nLights, ambient, flags)) return rc;
	if(int rc = checkMaterials(m, fn)) return rc;
	if(!dPacketXY && nPackets > 0) { snail_set_error("%s: null packet list", fn); return 1; }
	if(nPackets <= 0) return 0;
	if(!bgrPackets || ((unsigned long long)bgrPackets & 3)) { snail_set_error("%s: null or unaligned output", fn); return 1; }
	return framePacketsDev<MatLevels>(m, fn, cam, resx, resy, dPacketXY, nPackets, lights7, nLights, ambient, false, 0, bgrPackets, nullptr, dStats, stream);
}

int snail_render_materials_image(SnailMaterials *m, const float cam[13], int resx, int resy, const float *lights7, int nLights, const float ambient[3], int flags,
								 uint8_t *image, int pitch, uint64_t stats[4]) {
	const char *fn = "snail_render_materials_image";
	if(int rc = checkMatFrameArgs(fn, cam, resx, resy, lights7, nLights, ambient, flags)) return rc;
	if(int rc = checkMaterials(m, fn)) return rc;
	if(!image || pitch < resx * 3) { snail_set_error("%s: null image or a pitch below 3 * resx", fn); return 1; }
	return frameImage<MatLevels>(m, fn, cam, resx, resy, lights7, nLights, ambient, false, 0, image, pitch, nullptr, stats);
}

// ---- include/snail_materials_bounce.h ----
int snail_materials_bounce_dev(SnailMaterials *m, const float cam[13], int resx, int resy, const float *lights7, int nLights, const float ambient[3], int flags,
							   uint8_t *frame, int pitch, uint64_t *dStats, void *stream) {
	const char *fn = "snail_materials_bounce_dev";
	if(int rc = checkBounceFrameArgs(fn, cam, resx, resy, lights7, nLights, ambient, flags)) return rc;
	if(int rc = checkMaterials(m, fn)) return rc;
	if(!frame || pitch < resx * 3) { snail_set_error("%s: null frame or a pitch below 3 * resx", fn); return 1; }
	return frameDev<MatLevels>(m, fn, cam, resx, resy, lights7, nLights, ambient, (flags & SNAIL_RENDER_REFLECTIONS) != 0, 0, frame, pitch, nullptr, dStats, stream);
}

int snail_materials_bounce_packets_dev(SnailMaterials *m, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets, const float *lights7,
									   int nLights, const float ambient[3], int flags, uint8_t *bgrPackets, uint64_t *dStats, void *stream) {
	const char *fn = "snail_materials_bounce_packets_dev";
	if(int rc = checkBounceFrameArgs(fn, cam, resx, resy, lights7, nLights, ambient, flags)) return rc;
	if(int rc = checkMaterials(m, fn)) return rc;
	if(!dPacketXY && nPackets > 0) { snail_set_error("%s: null packet list", fn); return 1; }
	if(nPackets <= 0) return 0;
	if(!bgrPackets || ((unsigned long long)bgrPackets & 3)) { snail_set_error("%s: null or unaligned output", fn); return 1; }
	return framePacketsDev<MatLevels>(m, fn, cam, resx, resy, dPacketXY, nPackets, lights7, nLights, ambient, (flags & SNAIL_RENDER_REFLECTIONS) != 0, 0, bgrPackets, nullptr, dStats, stream);
}

int snail_materials_bounce_image(SnailMaterials *m, const float cam[13], int resx, int resy, const float *lights7, int nLights, const float ambient[3], int flags,
								 uint8_t *image, int pitch, uint64_t stats[4]) {
	const char *fn = "snail_materials_bounce_image";
	if(int rc = checkBounceFrameArgs(fn, cam, resx, resy, lights7, nLights, ambient, flags)) return rc;
	if(int rc = checkMaterials(m, fn)) return rc;
	if(!image || pitch < resx * 3) { snail_set_error("%s: null image or a pitch below 3 * resx", fn); return 1; }
	return frameImage<MatLevels>(m, fn, cam, resx, resy, lights7, nLights, ambient, (flags & SNAIL_RENDER_REFLECTIONS) != 0, 0, image, pitch, nullptr, stats);
}

int snail_materials_mirror_packets_dev(SnailMaterials *m, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets, const float *dT,
									   const float *dSamples, float *dOrigin, float *dDir, float *dIDir, uint8_t *dMask, float *dDistance, int32_t *dObject,
									   uint64_t *dStats, void *stream) {
	const char *fn = "snail_materials_mirror_packets_dev";
	if(int rc = checkMaterials(m, fn)) return rc;
	if(nPackets <= 0) return 0;
	if(!cam || resx <= 0 || resy <= 0 || !dPacketXY || !dT || !dSamples || !dOrigin || !dDir || !dIDir || !dMask || !dDistance || !dObject ||
	   (((unsigned long long)dSamples | (unsigned long long)dOrigin | (unsigned long long)dDir | (unsigned long long)dIDir | (unsigned long long)dDistance | (unsigned long long)dObject) & 15)) {
		snail_set_error("%s: bad camera or resolution, a null buffer, or a buffer not 16-byte aligned", fn);
		return 1;
	}
	DeviceGuard guard(m->device);
	SNAIL_LOCK(m->scene);
	dev::MatArgs A;
	matFillArgs(m, A, cam, resx, resy, dPacketXY, nPackets);
	A.s.hitT = dT; A.samples = const_cast<float *>(dSamples);
	A.s.rOrg = dOrigin; A.s.rDir = dDir; A.s.rIDir = dIDir; A.s.rMask = dMask; A.s.rDist = dDistance; A.s.rObj = dObject;
	A.s.stats = (dev::u64 *)dStats;
	const bool sse = m->scene->arith == SNAIL_ARITH_HOST_SSE;
	SNAIL_LAUNCH(sse, MatArgs, dim3(nPackets), dim3(64), 0, (hipStream_t)stream, A, k_mat_mirror);
	HIP_TRY(hipGetLastError());
	return 0;
}

int snail_materials_shade_rays_dev(SnailMaterials *m, int nPackets, const float *dDir, const uint8_t *dMask, const float *dT, const float *dU, const float *dV,
								   const int32_t *dTriId, float *dSamples, void *stream) {
	const char *fn = "snail_materials_shade_rays_dev";
	if(int rc = checkMaterials(m, fn)) return rc;
	if(nPackets <= 0) return 0;
	if(!dDir || !dT || !dU || !dV || !dTriId || !dSamples ||
	   (((unsigned long long)dDir | (unsigned long long)dT | (unsigned long long)dU | (unsigned long long)dV | (unsigned long long)dTriId | (unsigned long long)dSamples) & 15)) {
		snail_set_error("%s: a null buffer, or a buffer not 16-byte aligned", fn);
		return 1;
	}
	DeviceGuard guard(m->device);
	SNAIL_LOCK(m->scene);
	dev::MatArgs A;
	const float noCam[13] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 1};   // (generic packets carry their rays: no stage of this call generates any)
	matFillArgs(m, A, noCam, 16, 16, nullptr, nPackets);
	A.s.rDir = const_cast<float *>(dDir); A.s.rMask = const_cast<uint8_t *>(dMask); A.s.rDist = const_cast<float *>(dT); A.s.rObj = const_cast<int32_t *>(dTriId);
	A.rU = dU; A.rV = dV; A.rUVStride = 4;
	A.nSamples = dSamples;
	const bool sse = m->scene->arith == SNAIL_ARITH_HOST_SSE;
	SNAIL_LAUNCH(sse, MatArgs, dim3(nPackets), dim3(64), 0, (hipStream_t)stream, A, k_mat_sample_rays);
	HIP_TRY(hipGetLastError());
	return 0;
}

} // extern "C"
