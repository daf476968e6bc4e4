// instances_materials_host.inc -- the C-ABI of include/snail_instances_materials.h: the material set of an instanced scene (per-BLAS ShTriangle
// records and maps, ONE material and texture list) and the staged launches of instances_materials.inc (k_inst_frame with barycentrics ->
// k_imat_sample -> k_imat_light per (packet, light) -> k_mat_final).  Included after materials_host.inc, whose host-side checks it calls.  With the
// one mirrored bounce (instances_materials_bounce_host.inc, included next) the nested call stands between the sample stage and the lights.
#include "../../include/snail_instances_materials.h"

struct SnailInstancesMaterialsDyn;   // instances_materials_dynamic_host.inc: what a set of snail_instances_materials_create_dev carries besides
struct SnailInstancesMaterials {
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
	// intermediates of the lit frames, one set per launch in flight (round-robin, each guarded by an event; booked under the instances handle's mu)
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
	struct Set {
		char *base = nullptr;
		size_t packets = 0;
		int lights = 0;
		char *bounce = nullptr;   // allocated only once a bounce has been asked for; grown under the same rule
		size_t bouncePackets = 0;
		int bounceLights = 0;
		char *transp = nullptr;   // the levels of the transparency continuation (instances_materials_transparency_host.inc): only once asked for, sized by the depth
		size_t transpBytes = 0;
		char *tiles = nullptr;    // the tile renderer's part (instances_materials_tree_host.inc): the float colours of a whole packet list and, under 4x
		size_t tilesPackets = 0;  // antialiasing, its sub-packet list; only once asked for, grown under the same rule
		uint32_t *pstats = nullptr;   // snail_instances_materials_heatmap.h: the launch's per-packet TreeStats [packets][4] when the caller keeps none of its
		size_t pstatsPackets = 0;     // own; only once asked for, grown under the same rule
		hipEvent_t done = nullptr;
		bool used = false;
	};
	enum { kSets = 8 };
	Set set[kSets];
	unsigned setCount = 0;
	struct FrameList { int pw, ph; int32_t *d; };
	std::vector<FrameList> frameLists;   // a whole frame's packet list, cached by packet-grid size
	// snail_instances_materials_tree_render_tiles: ONE cached tile job per set (the structure of instances_tiles_host.inc); its calls take turns under
	// renderMu, which is taken before the instances handle's mu
	std::mutex renderMu;
	InstTileJob *tileJob = nullptr;
	// snail_instances_materials_set_level_budget (instances_materials_tree_host.inc): the bytes the levels of one group of intermediates may take;
	// 0 = SNAIL_MAT_LEVEL_BUDGET
	uint64_t levelBudget = 0;
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

// the packet list of a whole frame, cached in the set by packet-grid size as instancesFrameList caches it in the handle (the handle's mu held)
int imatFrameList(SnailInstancesMaterials *m, int resx, int resy, const int32_t **dXY, int *np) {
	const int pw = (resx + 15) / 16, ph = (resy + 15) / 16;
	*np = pw * ph;
	for(auto &f : m->frameLists)
		if(f.pw == pw && f.ph == ph) { *dXY = f.d; return 0; }
	if(m->frameLists.size() >= 16) {
		HIP_TRY(hipDeviceSynchronize());
		for(auto &f : m->frameLists) (void)hipFree(f.d);
		m->frameLists.clear();
	}
	std::vector<int32_t> xy((size_t)pw * ph * 2);
	for(int y = 0; y < ph; y++)
		for(int x = 0; x < pw; x++) { xy[((size_t)y * pw + x) * 2] = x * 16; xy[((size_t)y * pw + x) * 2 + 1] = y * 16; }
	SnailInstancesMaterials::FrameList f = {pw, ph, nullptr};
	HIP_TRY(hipMalloc((void **)&f.d, xy.size() * 4));
	if(hipMemcpy(f.d, xy.data(), xy.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(f.d); snail_set_error("frame packet list: upload failed"); return 1; }
	m->frameLists.push_back(f);
	*dXY = f.d;
	return 0;
}

// the next set of intermediates for np packets (the handle's mu held), grown if need be, its previous user waited for on st; refl: with the
// bounce's part
int imatNextSet(SnailInstancesMaterials *m, int np, int nLights, bool refl, hipStream_t st, SnailInstancesMaterials::Set **out) {
	SnailInstancesMaterials::Set &W = m->set[m->setCount++ % SnailInstancesMaterials::kSets];
	if(!W.base || W.packets < (size_t)np || W.lights < nLights) {   // grown: its previous user may still be running
		HIP_TRY(hipDeviceSynchronize());
		if(W.base) (void)hipFree(W.base);
		const size_t packets = std::max(W.packets, (size_t)np);
		const int lights = std::max(W.lights, nLights);
		W.base = nullptr; W.packets = 0; W.lights = 0; W.used = false;
		HIP_TRY(hipMalloc((void **)&W.base, SnailInstancesMaterials::Bufs::bytes(packets, lights)));
		W.packets = packets; W.lights = lights;
	}
	if(refl && (!W.bounce || W.bouncePackets < (size_t)np || W.bounceLights < nLights)) {   // the bounce's part: only when asked for, grown the same way
		HIP_TRY(hipDeviceSynchronize());
		if(W.bounce) (void)hipFree(W.bounce);
		const size_t packets = std::max(W.bouncePackets, (size_t)np);
		const int lights = std::max(W.bounceLights, nLights);
		W.bounce = nullptr; W.bouncePackets = 0; W.bounceLights = 0; W.used = false;
		HIP_TRY(hipMalloc((void **)&W.bounce, SnailInstancesMaterials::BounceBufs::bytes(packets, lights)));
		W.bouncePackets = packets; W.bounceLights = lights;
	}
	if(!W.done) HIP_TRY(hipEventCreateWithFlags(&W.done, hipEventDisableTiming));
	if(W.used) HIP_TRY(hipStreamWaitEvent(st, W.done, 0));
	*out = &W;
	return 0;
}
// after the set's user has enqueued its stages (rc: how that went): the event is recorded also when a stage failed after earlier ones were
// enqueued (matSetDone's rule)
int imatSetDone(SnailInstancesMaterials::Set &W, const char *fn, int rc, hipStream_t st) {
	if(hipEventRecord(W.done, st) == hipSuccess) W.used = true;
	else {
		W.packets = 0; W.bouncePackets = 0; W.tilesPackets = 0; W.pstatsPackets = 0; W.used = false;   // its next user synchronises the device
		if(!rc) { snail_set_error("%s: hipEventRecord failed", fn); return 1; }
	}
	return rc;
}

// snail_instances_render_materials_dev / _packets_dev and, with refl, snail_instances_materials_bounce_dev / _packets_dev (the handle's mu held)
int imatShadeDev(SnailInstancesMaterials *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights,
				 const float ambient[3], uint8_t *frame, int pitch, uint8_t *bgrPackets, uint64_t *dStats, hipStream_t st, bool refl = false) {
	if(!dXY) { if(int rc = imatFrameList(m, resx, resy, &dXY, &np)) return rc; }
	SnailInstancesMaterials::Set *Wp = nullptr;
	if(int rc = imatNextSet(m, np, nLights, refl, st, &Wp)) return rc;
	SnailInstancesMaterials::Bufs B;
	B.carve(Wp->base, (size_t)np);
	SnailInstancesMaterials::BounceBufs RB;
	if(refl) RB.carve(Wp->bounce, (size_t)np, nLights);
	const int rc = imatShade(m, fn, cam, resx, resy, dXY, np, lights7, nLights, ambient, frame, pitch, bgrPackets, B, refl ? &RB : nullptr, dStats, st);
	return imatSetDone(*Wp, fn, rc, st);
}

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
	for(auto &W : m->set) {
		if(W.base) (void)hipFree(W.base);
		if(W.bounce) (void)hipFree(W.bounce);
		if(W.transp) (void)hipFree(W.transp);
		if(W.tiles) (void)hipFree(W.tiles);
		if(W.pstats) (void)hipFree(W.pstats);
		if(W.done) (void)hipEventDestroy(W.done);
	}
	freeInstTileJob(m->tileJob);
	for(auto &f : m->frameLists) (void)hipFree(f.d);
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
	DeviceGuard guard(m->device);
	std::lock_guard<std::mutex> lock(m->inst->mu);
	return imatShadeDev(m, fn, cam, resx, resy, nullptr, 0, lights7, nLights, ambient, frame, pitch, nullptr, dStats, (hipStream_t)stream);
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
	DeviceGuard guard(m->device);
	std::lock_guard<std::mutex> lock(m->inst->mu);
	return imatShadeDev(m, fn, cam, resx, resy, dPacketXY, nPackets, lights7, nLights, ambient, nullptr, 0, bgrPackets, dStats, (hipStream_t)stream);
}

int snail_instances_render_materials_image(SnailInstancesMaterials *m, const float cam[13], int resx, int resy, const float *lights7, int nLights,
										   const float ambient[3], int flags, uint8_t *image, int pitch, uint64_t stats[4]) {
	const char *fn = "snail_instances_render_materials_image";
	if(int rc = checkMatFrameArgs(fn, cam, resx, resy, lights7, nLights, ambient, flags)) return rc;
	if(int rc = checkIMat(m, fn)) return rc;
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
	const size_t imgBytes = (size_t)pitch * resy, bufBytes = SnailInstancesMaterials::Bufs::bytes((size_t)np, nLights);
	if(int rc = hc.reserve(H::pad(xy.size() * 4) + H::pad(bufBytes) + H::pad(imgBytes + 4))) return rc;
	void *dXY = nullptr;
	if(int rc = hc.put(&dXY, xy.data(), xy.size() * 4)) return rc;
	SnailInstancesMaterials::Bufs W;
	W.carve((char *)hc.carve(bufBytes), (size_t)np);
	uint8_t *dImg = (uint8_t *)hc.carve(imgBytes + 4);
	{
		std::lock_guard<std::mutex> lock(h->mu);
		if(int rc = imatShade(m, fn, cam, resx, resy, (const int32_t *)dXY, np, lights7, nLights, ambient, dImg, pitch, nullptr, W, nullptr, hc.stats(), hc.stream())) return rc;
	}
	HIP_TRY(hipMemcpy2DAsync(image, (size_t)pitch, dImg, (size_t)pitch, (size_t)resx * 3, (size_t)resy, hipMemcpyDeviceToHost, hc.stream()));
	return hc.finish(stats);
}

} // extern "C"
