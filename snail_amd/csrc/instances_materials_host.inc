// instances_materials_host.inc -- the C-ABI of include/snail_instances_materials.h: the material set of an instanced scene (per-BLAS ShTriangle
// records and maps, ONE material and texture list) and the staged launches of instances_materials.inc (k_inst_frame with barycentrics ->
// k_imat_sample -> k_imat_light per (packet, light) -> k_mat_final).  Included after materials_host.inc, whose host-side checks it calls.  With the
// one mirrored bounce (instances_materials_bounce_host.inc, included next) the nested call stands between the sample stage and the lights.
// The handle's sets of intermediates and frame lists are shading_sets_host.inc's; the frames' bodies from DeviceGuard on are materials_levels_host.inc's
// (frameDev, framePacketsDev, frameImage) over IMatLevels, the instanced scene's kind, defined here beside imatShade.
#include "../../include/snail_instances_materials.h"

struct SnailInstancesMaterialsDyn;   // instances_materials_dynamic_host.inc: what a set of snail_instances_materials_create_dev carries besides
struct SnailInstancesMaterials : ShadeSets {   // (shading_sets_host.inc: the sets of intermediates, the frame lists, the tile job, the level budget)
	SnailInstances *inst = nullptr;
	SnailInstancesMaterialsDyn *dyn = nullptr;   // (null: no BLAS whose records are packed on the device -- the two older creators' sets)
	int device = 0;
	int nBlas = 0, nMats = 0, nTex = 0;
	bool canSelectTransparent = false;   // holds SNAIL_MAT_TRANSPARENT or UBER with 0 < dissolve < 1 (snail_instances_materials_create_transparent alone makes such a set)
	char *dBase = nullptr;   // ONE allocation: the per-BLAS table, every BLAS's records and map, materials, texture descriptors, texels
	const dev::IMatBlas *dTab = nullptr;
	std::vector<dev::IMatBlas> hTab;   // the host's copy of dTab (device addresses): where a BLAS's records stand, for the device pack
	const dev::MatRec *dMats = nullptr;
	const dev::TexRec *dTex = nullptr;
	const unsigned char *dTexels = nullptr;
	// a set's base part: the intermediates of the lit frames
	struct Bufs {
		float *hitT = nullptr, *hitU = nullptr, *hitV = nullptr, *samples = nullptr, *sDist = nullptr;
		int *hitInst = nullptr, *hitTri = nullptr;
		static size_t bytes(size_t np, int nLights) { return np * 256 * 4 * (size_t)(5 + 9 + (nLights > 0 ? nLights : 0)); }
		void carve(char *base, size_t np) {
			const size_t plane = np * 256 * 4;
			hitT = (float *)base; hitU = (float *)(base + plane); hitV = (float *)(base + 2 * plane); hitInst = (int *)(base + 3 * plane);
			hitTri = (int *)(base + 4 * plane); samples = (float *)(base + 5 * plane); sDist = (float *)(base + 14 * plane);
		}
	};
	// ... and those of the bounce (instances_materials_bounce_host.inc): the mirrored packets (rays, mask, distance, instance slot, triId, bary), the
	// nested samples, colour and shadow distances.  rTri and bary are neighbours: ONE memset defines both before the walk.
	struct BounceBufs {
		float *rOrg = nullptr, *rDir = nullptr, *rIDir = nullptr, *rDist = nullptr, *bary = nullptr, *nSamples = nullptr, *rCol = nullptr, *nSDist = nullptr;
		int *rInst = nullptr, *rTri = nullptr;
		unsigned char *rMask = nullptr;
		static size_t bytes(size_t np, int nLights) { return np * 256 * 4 * (size_t)(26 + (nLights > 0 ? nLights : 0)) + ((np * 64 + 255) & ~(size_t)255); }
		void carve(char *base, size_t np, int nLights) {
			const size_t plane = np * 256 * 4;
			rOrg = (float *)base; rDir = (float *)(base + 3 * plane); rIDir = (float *)(base + 6 * plane); rDist = (float *)(base + 9 * plane);
			rInst = (int *)(base + 10 * plane); rTri = (int *)(base + 11 * plane); bary = (float *)(base + 12 * plane); nSamples = (float *)(base + 14 * plane);
			rCol = (float *)(base + 23 * plane); nSDist = (float *)(base + 26 * plane);
			rMask = (unsigned char *)(base + (size_t)(26 + (nLights > 0 ? nLights : 0)) * plane);
		}
	};
	typedef SnailMaterials::TileBufs TileBufs;   // (the tile renderer's part holds colours and a sub-packet list: no instance data)
};

namespace {

// instances_materials_dynamic_host.inc: whether the records of every dynamic BLAS are those of the tree that BLAS holds now (a refusal that names
// the rebuild otherwise), and the end of what the set carries for them
int imatDynCheckFresh(const SnailInstancesMaterials *m, const char *fn);
void imatDynFree(SnailInstancesMaterialsDyn *d);

// any set: the entry points of include/snail_instances_materials_transparency.h
int checkIMatAny(const SnailInstancesMaterials *m, const char *fn) {
	if(!m || !m->inst || !m->dBase) { snail_set_error("%s: invalid instanced material set handle", fn); return 1; }
	if(int rc = checkInstances(m->inst, fn)) return rc;
	return m->dyn ? imatDynCheckFresh(m, fn) : 0;
}
// the entry points of snail_instances_materials.h and _bounce.h: their kernels know neither the transparent kind nor the selector
int checkIMat(const SnailInstancesMaterials *m, const char *fn) {
	if(m && m->canSelectTransparent) {
		snail_set_error("%s: the set holds a material that can select a transparent lane, which this function's kernels do not know (include/snail_instances_materials_transparency.h)", fn);
		return 1;
	}
	return checkIMatAny(m, fn);
}

#define SNAIL_IMAT_LAUNCH(SSE, GRID, STREAM, A, ...) SNAIL_LAUNCH(SSE, IMatArgs, GRID, dim3(64), 0, STREAM, A, __VA_ARGS__)

// the part of the argument record that every stage reads (the instances handle's mu held, I from instancesBegin)
void imatFillArgs(const SnailInstancesMaterials *m, dev::IMatArgs &A, const dev::InstArgs &I, const float cam[13], int resx, int resy, const int32_t *dXY, int np) {
	memset(&A, 0, sizeof(A));
	A.m.s.hostTab = I.hostTab;
	A.m.s.g = makeGen(cam, resx, resy);
	A.m.s.resx = resx; A.m.s.resy = resy; A.m.s.pw = (resx + 15) / 16; A.m.s.ph = (resy + 15) / 16;
	A.m.s.packetXY = (const int2 *)dXY; A.m.s.nPackets = np; A.m.s.nBlocks = np;
	A.m.mats = m->dMats; A.m.nMats = m->nMats;
	A.m.tex = m->dTex; A.m.texels = m->dTexels;
	A.i = I;
	A.tab = m->dTab; A.nBlas = m->nBlas;
	A.nSlots = m->inst->instCap;   // (the record count itself is the device's after a rebuild there: a slot is kept inside the buffer)
}

// instances_materials_bounce_host.inc: the nested call of the one mirrored bounce on the primary samples of A -- mirrored packets, their walk, nested
// samples, lights and colour -- with its intermediates R entered into A
int imatNested(SnailInstances *h, const char *fn, dev::IMatArgs &A, const dev::InstArgs &I, bool sse, bool deep, const SnailInstancesMaterials::BounceBufs &R,
			   hipStream_t st);

// the stages of one lit frame over the packet list dXY into `frame` (or packet-major `bgrPackets`), intermediates in W; the handle's mu held.
// R (or null): the intermediates of the one mirrored bounce -- the nested call between the sample stage and the primary lights, the blend last.
int imatShade(SnailInstancesMaterials *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights,
			  const float ambient[3], uint8_t *frame, int pitch, uint8_t *bgrPackets, const SnailInstancesMaterials::Bufs &W,
			  const SnailInstancesMaterials::BounceBufs *R, uint64_t *dStats, hipStream_t st) {
	SnailInstances *h = m->inst;
	dev::InstArgs I;
	bool sse, deep;
	if(int rc = instancesBegin(h, fn, I, &sse, &deep, st)) return rc;
	const dim3 grid(np);
	// primary hits, with their barycentrics
	dev::InstArgs P = I;
	P.g = makeGen(cam, resx, resy);
	P.resx = resx; P.resy = resy;
	P.packetXY = (const int2 *)dXY; P.nPackets = np;
	P.t = W.hitT; P.u = W.hitU; P.v = W.hitV; P.instOut = W.hitInst; P.triOut = W.hitTri;
	P.stats = (dev::u64 *)dStats;
	if(deep) SNAIL_INST_LAUNCH(sse, grid, st, P, k_inst_frame<true>);
	else SNAIL_INST_LAUNCH(sse, grid, st, P, k_inst_frame<false>);

	dev::IMatArgs A;
	imatFillArgs(m, A, I, cam, resx, resy, dXY, np);
	A.m.s.nLights = nLights;
	for(int n = 0; n < nLights; n++) for(int k = 0; k < 7; k++) A.m.s.lights[n][k] = lights7[n * 7 + k];
	for(int c = 0; c < 3; c++) { A.m.s.ambient[c] = ambient[c]; A.m.s.color[c] = 1.0f; }
	A.m.s.hitT = W.hitT; A.m.s.hitId = W.hitTri; A.m.hitU = W.hitU; A.m.hitV = W.hitV; A.hitInst = W.hitInst;
	A.m.samples = W.samples; A.m.s.sDist = W.sDist;
	A.m.s.frame = frame; A.m.s.pitch = pitch; A.m.s.bgrPackets = bgrPackets;
	A.m.s.stats = (dev::u64 *)dStats;
	SNAIL_IMAT_LAUNCH(sse, grid, st, A, k_imat_sample);
	if(R) { if(int rc = imatNested(h, fn, A, I, sse, deep, *R, st)) return rc; }
	if(nLights) {
		const dim3 lgrid(np, nLights);
		if(deep) SNAIL_IMAT_LAUNCH(sse, lgrid, st, A, k_imat_light<true>);
		else SNAIL_IMAT_LAUNCH(sse, lgrid, st, A, k_imat_light<false>);
	}
	// (samples, hits and the surviving distances: the plain scenes' colour stage as it is)
	if(R) SNAIL_LAUNCH(sse, MatArgs, grid, dim3(64), 0, st, A.m, k_mat_final_blend);
	else SNAIL_LAUNCH(sse, MatArgs, grid, dim3(64), 0, st, A.m, k_mat_final);
	return instancesEnd(h, st);
}

#define SNAIL_ITRANSP_LAUNCH(SSE, GRID, STREAM, A, ...) SNAIL_LAUNCH(SSE, ITranspArgs, GRID, dim3(64), 0, STREAM, A, __VA_ARGS__)

// The instanced scene's kind of the frame bodies and the level driver (materials_levels_host.inc); the handle's mu held.  Every launch is booked through
// instancesBegin / instancesEnd, so the frame is ordered against snail_instances_update and snail_instances_rebuild_dev as a walk is.  The sample
// and light stages take an ITranspArgs of the kind's own: its MatArgs is the frame's, copied into the scene-free stages' record whenever a level
// changes it.
struct IMatLevels : LevelsFrame {
	typedef SnailInstancesMaterials Handle;
	typedef SnailInstancesMaterials::Bufs Bufs;
	typedef SnailInstancesMaterials::BounceBufs BounceBufs;
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
	// the handle's part of the frame bodies, of levelsStore and of the host calls
	static int opaque(SnailInstancesMaterials *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights,
					  const float ambient[3], uint8_t *frame, int pitch, uint8_t *bgrPackets, const Bufs &W, const BounceBufs *R, uint64_t *dStats, hipStream_t st) {
		return imatShade(m, fn, cam, resx, resy, dXY, np, lights7, nLights, ambient, frame, pitch, bgrPackets, W, R, dStats, st);
	}
	// (the hit distances of k_inst_frame alone)
	static int depthStore(SnailInstancesMaterials *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *, int,
						  const float ambient[3], int flags, const float *tint, uint8_t *bgrPackets, const InstTileJob *J, uint64_t *dStats, hipStream_t st) {
		const float white[3] = {1.0f, 1.0f, 1.0f};
		return instancesShadeStore(m->inst, fn, cam, resx, resy, dXY, np, nullptr, 0, ambient, white, flags & (SNAIL_RENDER_DEPTH | SNAIL_RENDER_AA4), tint, bgrPackets, J, dStats, st);
	}
	static SnailScene *scene(SnailInstancesMaterials *m) { return m->inst->blas[0]; }   // (the arithmetic and its tables are the BLAS scenes'; it lends a host call its free list)
	static std::mutex &mu(SnailInstancesMaterials *m) { return m->inst->mu; }
};

// the creators: snail_instances_materials_create (transp = false: its refusals) and snail_instances_materials_create_transparent
// (include/snail_instances_materials_transparency.h), one body as matCreate is for plain scenes
SnailInstancesMaterials *imatUpload(const char *fn, bool canSelectAny, SnailInstances *h, const SnailBlasShading *perBlas, int nBlas, const SnailMaterial *mats,
									int nMats, const int32_t *opacityTexture, const SnailTexture *textures, int nTex);
SnailInstancesMaterials *imatCreate(const char *fn, bool transp, SnailInstances *h, const SnailBlasShading *perBlas, int nBlas, const SnailMaterial *mats, int nMats,
									const int32_t *opacityTexture, const SnailTexture *textures, int nTex) {
	// the caller's HOST data first, by snail_materials_create's own check (once per BLAS: its words name the record, entry, material or texture)
	if(!perBlas || nBlas <= 0) { snail_set_error("%s: no per-BLAS shading data", fn); return nullptr; }
	bool canSelectAny = false;
	for(int b = 0; b < nBlas; b++) {
		bool canSelect = false;
		if(!matCheckHost(fn, transp, false, perBlas[b].shtris64, perBlas[b].nTris, perBlas[b].matMap, perBlas[b].nMap, mats, nMats, opacityTexture, textures, nTex, &canSelect)) {
			char why[400];
			snprintf(why, sizeof(why), "%s", snail_last_error());
			snail_set_error("%s (the shading data of BLAS %d)", why, b);
			return nullptr;
		}
		canSelectAny = canSelectAny || canSelect;
	}
	if(checkInstances(h, fn)) return nullptr;
	if(nBlas != (int)h->blas.size()) { snail_set_error("%s: shading data of %d BLASes (nBlas) for a handle of %d", fn, nBlas, (int)h->blas.size()); return nullptr; }
	for(int b = 0; b < nBlas; b++) {
		if(checkScene(h->blas[b], fn)) return nullptr;
		if(h->blas[b]->fast) { snail_set_error("%s: BLAS %d is rebuilt on the device, which renumbers its triangles: no records for such a BLAS here", fn, b); return nullptr; }
		if(perBlas[b].nTris != h->blas[b]->nTris) { snail_set_error("%s: BLAS %d: %d records (nTris) for a scene of %d triangles", fn, b, perBlas[b].nTris, h->blas[b]->nTris); return nullptr; }
	}
	return imatUpload(fn, canSelectAny, h, perBlas, nBlas, mats, nMats, opacityTexture, textures, nTex);
}

// the second half of the creators, after every check: the set on the device.  A BLAS with shtris64 == NULL (snail_instances_materials_create_dev's
// alone: the checks above let none pass) gets zeroed records, which that creator packs on the device
SnailInstancesMaterials *imatUpload(const char *fn, bool canSelectAny, SnailInstances *h, const SnailBlasShading *perBlas, int nBlas, const SnailMaterial *mats,
									int nMats, const int32_t *opacityTexture, const SnailTexture *textures, int nTex) {
	// the device copy (materials and textures as matUpload lays them out; opacityTexture is read for the transparent kind alone, which only the
	// transparent creator's check lets pass)
	std::vector<dev::MatRec> recs;
	std::vector<dev::TexRec> trecs;
	const size_t texelBytes = matPackLists(mats, nMats, opacityTexture, textures, nTex, recs, trecs);
	typedef HostCallScope H;
	std::vector<size_t> oTris((size_t)nBlas), oMap((size_t)nBlas);
	size_t total = H::pad((size_t)nBlas * sizeof(dev::IMatBlas));
	for(int b = 0; b < nBlas; b++) {
		oTris[b] = total; total += H::pad((size_t)perBlas[b].nTris * 64);
		oMap[b] = total; total += H::pad((size_t)perBlas[b].nMap * 4);
	}
	const size_t oMats = total, oTex = oMats + H::pad(recs.size() * sizeof(dev::MatRec)), oTexels = oTex + H::pad(trecs.size() * sizeof(dev::TexRec));
	total = oTexels + H::pad(texelBytes + 16);
	DeviceGuard guard(h->device);
	char *base = nullptr;
	hipError_t e = hipMalloc((void **)&base, total);
	if(e == hipSuccess) e = hipMemset(base, 0, total);
	std::vector<dev::IMatBlas> tab((size_t)nBlas);
	for(int b = 0; b < nBlas && e == hipSuccess; b++) {
		tab[b].shtris = (const uint4 *)(base + oTris[b]); tab[b].matMap = (const int *)(base + oMap[b]);
		tab[b].nTris = perBlas[b].nTris; tab[b].nMap = perBlas[b].nMap;
		if(perBlas[b].shtris64) e = hipMemcpy(base + oTris[b], perBlas[b].shtris64, (size_t)perBlas[b].nTris * 64, hipMemcpyHostToDevice);
		if(e == hipSuccess) e = hipMemcpy(base + oMap[b], perBlas[b].matMap, (size_t)perBlas[b].nMap * 4, hipMemcpyHostToDevice);
	}
	if(e == hipSuccess) e = hipMemcpy(base, tab.data(), tab.size() * sizeof(dev::IMatBlas), hipMemcpyHostToDevice);
	if(e == hipSuccess) e = hipMemcpy(base + oMats, recs.data(), recs.size() * sizeof(dev::MatRec), hipMemcpyHostToDevice);
	if(e == hipSuccess) e = hipMemcpy(base + oTex, trecs.data(), trecs.size() * sizeof(dev::TexRec), hipMemcpyHostToDevice);
	for(int k = 0; k < nTex && e == hipSuccess; k++)
		e = hipMemcpy(base + oTexels + trecs[k].base, textures[k].levels, (size_t)snail_texture_size(trecs[k].w, trecs[k].h, nullptr), hipMemcpyHostToDevice);
	if(e != hipSuccess) {
		snail_set_error("%s: device copy failed: %s", fn, hipGetErrorString(e));
		if(base) (void)hipFree(base);
		return nullptr;
	}
	SnailInstancesMaterials *m = new SnailInstancesMaterials();
	m->inst = h; m->device = h->device;
	m->nBlas = nBlas; m->nMats = nMats; m->nTex = nTex;
	m->dBase = base;
	m->canSelectTransparent = canSelectAny;
	m->hTab = tab;
	m->dTab = (const dev::IMatBlas *)base; m->dMats = (const dev::MatRec *)(base + oMats);
	m->dTex = (const dev::TexRec *)(base + oTex); m->dTexels = (const unsigned char *)(base + oTexels);
	return m;
}

} // namespace

extern "C" {

SnailInstancesMaterials *snail_instances_materials_create(SnailInstances *h, const SnailBlasShading *perBlas, int nBlas, const SnailMaterial *mats, int nMats,
														  const SnailTexture *textures, int nTex) {
	return imatCreate("snail_instances_materials_create", false, h, perBlas, nBlas, mats, nMats, nullptr, textures, nTex);
}

void snail_instances_materials_destroy(SnailInstancesMaterials *m) {
	if(!m) return;
	DeviceGuard guard(m->device);
	(void)hipDeviceSynchronize();
	m->release();
	if(m->dBase) (void)hipFree(m->dBase);
	imatDynFree(m->dyn);
	delete m;
}

int snail_instances_materials_shade_packets_dev(SnailInstancesMaterials *m, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets,
												const float *dT, const float *dU, const float *dV, const int32_t *dInst, const int32_t *dTriId, float *dSamples,
												void *stream) {
	const char *fn = "snail_instances_materials_shade_packets_dev";
	if(int rc = checkIMat(m, fn)) return rc;
	if(nPackets <= 0) return 0;
	if(!cam || resx <= 0 || resy <= 0 || !dPacketXY || !dT || !dU || !dV || !dInst || !dTriId || !dSamples || ((unsigned long long)dSamples & 15)) {
		snail_set_error("%s: bad camera or resolution, a null buffer, or samples not 16-byte aligned", fn);
		return 1;
	}
	SnailInstances *h = m->inst;
	hipStream_t st = (hipStream_t)stream;
	DeviceGuard guard(m->device);
	std::lock_guard<std::mutex> lock(h->mu);
	dev::InstArgs I;
	bool sse, deep;
	if(int rc = instancesBegin(h, fn, I, &sse, &deep, st)) return rc;   // (the stage reads the instance records: ordered against updates as a walk is)
	dev::IMatArgs A;
	imatFillArgs(m, A, I, cam, resx, resy, dPacketXY, nPackets);
	A.m.s.hitT = dT; A.m.s.hitId = dTriId; A.m.hitU = dU; A.m.hitV = dV; A.hitInst = dInst;
	A.m.samples = dSamples;
	SNAIL_IMAT_LAUNCH(sse, dim3(nPackets), st, A, k_imat_sample);
	return instancesEnd(h, st);
}

int snail_instances_render_materials_dev(SnailInstancesMaterials *m, const float cam[13], int resx, int resy, const float *lights7, int nLights,
										 const float ambient[3], int flags, uint8_t *frame, int pitch, uint64_t *dStats, void *stream) {
	const char *fn = "snail_instances_render_materials_dev";
	if(int rc = checkMatFrameArgs(fn, cam, resx, resy, lights7, nLights, ambient, flags)) return rc;
	if(int rc = checkIMat(m, fn)) return rc;
	if(!frame || pitch < resx * 3) { snail_set_error("%s: null frame or a pitch below 3 * resx", fn); return 1; }
	return frameDev<IMatLevels>(m, fn, cam, resx, resy, lights7, nLights, ambient, false, 0, frame, pitch, nullptr, dStats, stream);
}

int snail_instances_render_materials_packets_dev(SnailInstancesMaterials *m, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets,
												 const float *lights7, int nLights, const float ambient[3], int flags, uint8_t *bgrPackets, uint64_t *dStats,
												 void *stream) {
	const char *fn = "snail_instances_render_materials_packets_dev";
	if(int rc = checkMatFrameArgs(fn, cam, resx, resy, lights7, nLights, ambient, flags)) return rc;
	if(int rc = checkIMat(m, fn)) return rc;
	if(!dPacketXY && nPackets > 0) { snail_set_error("%s: null packet list", fn); return 1; }
	if(nPackets <= 0) return 0;
	if(!bgrPackets || ((unsigned long long)bgrPackets & 3)) { snail_set_error("%s: null or unaligned output", fn); return 1; }
	return framePacketsDev<IMatLevels>(m, fn, cam, resx, resy, dPacketXY, nPackets, lights7, nLights, ambient, false, 0, bgrPackets, nullptr, dStats, stream);
}

int snail_instances_render_materials_image(SnailInstancesMaterials *m, const float cam[13], int resx, int resy, const float *lights7, int nLights,
										   const float ambient[3], int flags, uint8_t *image, int pitch, uint64_t stats[4]) {
	const char *fn = "snail_instances_render_materials_image";
	if(int rc = checkMatFrameArgs(fn, cam, resx, resy, lights7, nLights, ambient, flags)) return rc;
	if(int rc = checkIMat(m, fn)) return rc;
	if(!image || pitch < resx * 3) { snail_set_error("%s: null image or a pitch below 3 * resx", fn); return 1; }
	return frameImage<IMatLevels>(m, fn, cam, resx, resy, lights7, nLights, ambient, false, 0, image, pitch, nullptr, stats);
}

} // extern "C"
