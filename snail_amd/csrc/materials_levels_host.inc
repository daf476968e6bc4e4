// materials_levels_host.inc -- the frames of full shading, once for plain and instanced scenes; included by snail_hip.hip ahead of
// materials_host.inc and instances_materials_host.inc, which define the two scene kinds next to their handles.
//   shadeLevels      the stages of one transparent frame: the way down of chain A, then for k = D .. 0 the B chain of A_k (mirror, walk, sample,
//                    generator / walk / sample down to level D, truncation count, way back up), the reflection blend into A_k, its transparency
//                    blend, lights and colour.  Without refl: the transparency continuation alone.
//   frameStages      one frame's stages by depth: 0 = the kind's opaque stages (matShade, imatShade), otherwise shadeLevels.
//   frameDev, framePacketsDev, frameImage   the bodies of every _dev, _packets_dev and _image entry point from DeviceGuard on: the first two over
//                    the handle's next set of intermediates (frameSet), the last over a stream, counters and staging of the call's own.
//   levelsStore      runs shadeLevels over a packet list in slices that keep the levels within the set's budget, and hands the float colours to k_inst_store.
//   renderTilesHost, renderFrameHost   the host calls around a store step (levelsStore, or matStoreStep of materials_tiles_host.inc: matShadeStore).
// Each is a template over a scene kind: MatLevels (materials_host.inc) for SnailMaterials, IMatLevels (instances_materials_host.inc) for
// SnailInstancesMaterials.  A kind holds what differs between the two: how a launch is ordered against rebuilds and updates (begin / end), the
// walks, the stages that read the scene's shading records (samples and lights) with their argument records, the opaque stages, and the handle's
// lock and lender.  The scene-free stages are launched here; the sets of intermediates are the handles' ShadeSets (shading_sets_host.inc).
#include "../../include/snail_materials_tree.h"

namespace {

// One level's intermediates: the generic packets and everything of the bounce's part (the kind's BounceBufs: rays, mask, hits, barycentrics,
// samples, colour, shadow distances) + opacity, selector and the level's order list.  Level 0 (the primary packets, the kind's Bufs) has the
// last three alone.
template <class BounceBufs>
struct Level {
	BounceBufs R;
	float *opacity = nullptr;
	unsigned char *sel = nullptr;
	int32_t *order = nullptr;
	static size_t extra(size_t np) { return np * 1024 + ((np * 64 + 255) & ~(size_t)255) + ((np * 4 + 255) & ~(size_t)255); }
	static size_t bytes(size_t np, int nLights) { return ((BounceBufs::bytes(np, nLights) + 255) & ~(size_t)255) + extra(np); }
	char *carveExtra(char *p, size_t np) {
		opacity = (float *)p; p += np * 1024;
		sel = (unsigned char *)p; p += (np * 64 + 255) & ~(size_t)255;
		order = (int32_t *)p; p += (np * 4 + 255) & ~(size_t)255;
		return p;
	}
	char *carve(char *p, size_t np, int nLights) {
		R.carve(p, np, nLights);
		return carveExtra(p + ((BounceBufs::bytes(np, nLights) + 255) & ~(size_t)255), np);
	}
};
// the levels of n packets: L[0]'s opacity / selector / order + D A-levels, and with the bounce D + 1 B-levels
template <class BounceBufs>
size_t levelsBytes(size_t n, int nLights, int depth, bool refl) {
	return Level<BounceBufs>::extra(n) + (size_t)(refl ? 2 * depth + 1 : depth) * Level<BounceBufs>::bytes(n, nLights);
}

// What every stage of one frame's launch shares; the base of both kinds.  pstats (a heat-map launch, include/snail_materials_heatmap.h and
// snail_instances_materials_heatmap.h; cleared by the caller): every stage that books into dStats -- the walks, the lights, the generators and the
// mirrors -- also books per packet there, through its PSTATS / _heat instantiation, at the packet's index in the frame's list.
struct LevelsFrame {
	const char *fn;
	hipStream_t st;
	uint32_t *pstats;
	int np;
	dim3 grid, lgrid;   // one wave per packet; per (packet, light)
	bool sse = false, deep = false;   // (the kind's begin)
	LevelsFrame(const char *fn_, hipStream_t st_, uint32_t *pstats_, int np_, int nLights) : fn(fn_), st(st_), pstats(pstats_), np(np_), grid(np_), lgrid(np_, nLights > 0 ? nLights : 1) {}
	int failed(const char *what, hipError_t e) const {
		snail_set_error("%s: %s: %s", fn, what, hipGetErrorString(e));
		return 100 + (int)e;
	}
	// after a stage's launch
	int launched(const char *what) const {
		const hipError_t e = hipGetLastError();
		return e == hipSuccess ? 0 : failed(what, e);
	}
};
// a stage with a _heat instantiation (sse, pstats, st: the frame's)
#define SNAIL_LEVELS_LAUNCH(ARGS_T, GRID, REC, K)                                                                                            \
	do {                                                                                                                                   \
		if(pstats) SNAIL_LAUNCH(sse, ARGS_T, GRID, dim3(64), 0, st, REC, K##_heat);                                                        \
		else SNAIL_LAUNCH(sse, ARGS_T, GRID, dim3(64), 0, st, REC, K);                                                                     \
	} while(0)
// (... of a kernel with a <DEEP> argument)
#define SNAIL_LEVELS_LAUNCH_DEEP(ARGS_T, GRID, REC, K)                                                                                       \
	do {                                                                                                                                   \
		if(pstats) {                                                                                                                       \
			if(deep) SNAIL_LAUNCH(sse, ARGS_T, GRID, dim3(64), 0, st, REC, K##_heat<true>);                                                \
			else SNAIL_LAUNCH(sse, ARGS_T, GRID, dim3(64), 0, st, REC, K##_heat<false>);                                                   \
		} else if(deep) SNAIL_LAUNCH(sse, ARGS_T, GRID, dim3(64), 0, st, REC, K<true>);                                                    \
		else SNAIL_LAUNCH(sse, ARGS_T, GRID, dim3(64), 0, st, REC, K<false>);                                                              \
	} while(0)

// The stages between the kind's begin and end.  The first failed launch or clear is kept, named "<fn>: <stage>: <hip error>" with 100 + e, and no
// further stage is enqueued after it.  A heat-map launch leaves out the stages that only make colours (both blends, the colour stages,
// k_mat_final), and frame / bgrPackets / colPackets are not written: no selector, normal or position a counter depends on reads a colour.
template <class K>
int levelStages(K &kind, const float cam[13], int resx, int resy, const int32_t *dXY, const float *lights7, int nLights, const float ambient[3], uint8_t *frame, int pitch,
				uint8_t *bgrPackets, float *colPackets, const typename K::Bufs &W, char *arena, int D, bool refl, uint64_t *dTrunc, uint64_t *dStats) {
	typedef Level<typename K::BounceBufs> Lv;
	const int np = kind.np;
	const bool sse = kind.sse;
	const hipStream_t st = kind.st;
	uint32_t *const pstats = kind.pstats;
	const dim3 grid = kind.grid, wave(64);
	Lv L[SNAIL_MAT_TRANSP_MAX_DEPTH + 1], M[SNAIL_MAT_TRANSP_MAX_DEPTH + 1];   // chain A; chain B: ONE set of levels, reused by every k (the stream orders them)
	char *p = L[0].carveExtra(arena, (size_t)np);
	for(int k = 1; k <= D; k++) p = L[k].carve(p, (size_t)np, nLights);
	if(refl) for(int j = 0; j <= D; j++) p = M[j].carve(p, (size_t)np, nLights);
	// primary hits, with their barycentrics
	int lrc = kind.primary(cam, resx, resy, dXY, W, dStats);
	if(lrc) return lrc;
	// the scene-free stages take a MatArgs (materials.inc), a TranspArgs (materials_transparency.inc) or a TreeArgs (materials_tree.inc), each the
	// head of the next; A is the frame's MatArgs, which the kind's own stages read too
	dev::TreeArgs G;
	memset(&G, 0, sizeof(G));
	dev::TranspArgs &T = G.t;
	dev::MatArgs &A = kind.frameArgs(G, cam, resx, resy, dXY, W);
	A.s.nLights = nLights;
	for(int n = 0; n < nLights; n++) for(int k = 0; k < 7; k++) A.s.lights[n][k] = lights7[n * 7 + k];
	for(int c = 0; c < 3; c++) { A.s.ambient[c] = ambient[c]; A.s.color[c] = 1.0f; }
	A.s.hitT = W.hitT; A.hitU = W.hitU; A.hitV = W.hitV;
	A.samples = W.samples; A.s.sDist = W.sDist;
	A.s.frame = frame; A.s.pitch = pitch; A.s.bgrPackets = bgrPackets;
	A.s.colPackets = colPackets;
	A.s.stats = (dev::u64 *)dStats;
	A.s.pstats = pstats;
	A.rUVStride = 8;
	T.trunc = (unsigned long long *)dTrunc;
	auto launched = [&](const char *what) { if(!lrc) lrc = kind.launched(what); };
	// a level's generic packets as the stages' source, under its own order list (null: every packet); slotAsObject: see the instanced kind
	auto level = [&](const Lv &X, const int32_t *order, bool slotAsObject) {
		const typename K::BounceBufs &R = X.R;
		A.s.rOrg = R.rOrg; A.s.rDir = R.rDir; A.s.rIDir = R.rIDir; A.s.rMask = R.rMask; A.s.rDist = R.rDist; A.s.rCol = R.rCol;
		A.rU = R.bary; A.rV = R.bary + 4;
		A.nSamples = R.nSamples; A.nSDist = R.nSDist;
		T.inOrder = order;
		kind.level(G, R, order, slotAsObject);
	};
	// the ordered walk of a level's packets (order null: all of them, as the bounce walks its mirrored packets) and its sample stage
	auto walkSample = [&](const Lv &X, const int32_t *order) {
		if(lrc) return;
		lrc = kind.walk(X.R, order, dStats);
		if(lrc) return;
		level(X, order, false);
		lrc = kind.sampleRays(G, X.opacity, X.sel);
	};
	// the generator: from level `from` (its rays, hits, selector and own order list) into level `to`'s packets and order list; it zeroes the object
	auto generate = [&](const Lv &from, const int32_t *fromOrder, const Lv &to) {
		if(lrc) return;
		level(to, fromOrder, true);
		T.order = to.order;
		T.cT = from.R.rDist; T.cSel = from.sel;
		T.cOrg = from.R.rOrg; T.cDir = from.R.rDir; T.cIDir = from.R.rIDir;
		SNAIL_LEVELS_LAUNCH(TranspArgs, grid, T, k_mat_continue_rays);
		launched("k_mat_continue_rays");
	};
	// the lanes a level D would still select: counted, then treated as not selected
	auto truncated = [&](const Lv &X, const int32_t *order) {
		if(lrc) return;
		level(X, order, false);
		T.bSel = X.sel;
		SNAIL_LAUNCH(sse, TranspArgs, grid, wave, 0, st, T, k_mat_truncated);
		launched("k_mat_truncated");
	};
	// a nested level's way back up: (the blend from the deeper level's colour,) its lights, its colour
	auto lightColour = [&](const Lv &X, const int32_t *order, const Lv *deeper) {
		if(lrc) return;
		level(X, order, false);
		if(deeper && !pstats) {
			T.bSamples = X.R.nSamples; T.bOpacity = X.opacity; T.bSel = X.sel; T.bCol = deeper->R.rCol;
			SNAIL_LAUNCH(sse, TranspArgs, grid, wave, 0, st, T, k_mat_blend_transp);
			launched("k_mat_blend_transp");
		}
		if(nLights && !lrc) lrc = kind.nestedLights(G);
		if(!lrc && !pstats) { SNAIL_LAUNCH(sse, TranspArgs, grid, wave, 0, st, T, k_mat_colour_transp); launched("k_mat_colour_transp"); }
	};

	// ---- the way down of chain A: sample, then per level generator -> ordered walk -> nested sample ----
	lrc = kind.samplePrimary(G, L[0].opacity, L[0].sel);
	for(int k = 1; k <= D; k++) {
		if(k > 1) generate(L[k - 1], L[k - 1].order, L[k]);
		else if(!lrc) {
			level(L[1], nullptr, true);
			T.order = L[1].order;
			T.cT = W.hitT; T.cSel = L[0].sel;
			T.cOrg = T.cDir = T.cIDir = nullptr;
			SNAIL_LEVELS_LAUNCH(TranspArgs, grid, T, k_mat_continue);
			launched("k_mat_continue");
		}
		walkSample(L[k], L[k].order);
	}
	truncated(L[D], L[D].order);

	// ---- the way back up ----
	if(!lrc) lrc = kind.lightsBegin(A, nLights);
	for(int k = D; k >= 0 && !lrc; k--) {
		const int32_t *aOrder = k ? L[k].order : nullptr;
		if(refl) {
			// the B chain of A_k: the mirrored call B_{k,k} (every packet of A_k, hit or not) and its continuations down to level D
			const int32_t *bOrder = k ? M[k].order : nullptr;   // (k = 0: every packet, the bounce's walk)
			if(k) {
				level(L[k], aOrder, false);
				G.oOrg = M[k].R.rOrg; G.oDir = M[k].R.rDir; G.oIDir = M[k].R.rIDir; G.oDist = M[k].R.rDist; G.oObj = K::object(M[k].R); G.oMask = M[k].R.rMask;
				G.oOrder = M[k].order;
				SNAIL_LEVELS_LAUNCH(TreeArgs, grid, G, k_mat_mirror_rays);
				launched("k_mat_mirror_rays");
			} else {
				level(M[0], nullptr, true);
				SNAIL_LEVELS_LAUNCH(MatArgs, grid, A, k_mat_mirror);
				launched("k_mat_mirror");
			}
			walkSample(M[k], bOrder);
			for(int j = k + 1; j <= D; j++) {
				generate(M[j - 1], j - 1 == k ? bOrder : M[j - 1].order, M[j]);
				walkSample(M[j], M[j].order);
			}
			truncated(M[D], D == k ? bOrder : M[D].order);
			for(int j = D; j >= k; j--) lightColour(M[j], j == k ? bOrder : M[j].order, j < D ? &M[j + 1] : nullptr);
			// diffuse += (refl - diffuse) * 0.3 on A_k's hit lanes, before its transparency blend
			if(!lrc && !pstats) {
				if(k) {
					level(L[k], aOrder, false);
					T.bSamples = L[k].R.nSamples; T.bCol = M[k].R.rCol;
					SNAIL_LAUNCH(sse, TranspArgs, grid, wave, 0, st, T, k_mat_blend_refl_rays);
				} else {
					T.inOrder = nullptr;
					T.bSamples = W.samples; T.bCol = M[0].R.rCol;
					SNAIL_LAUNCH(sse, TranspArgs, grid, wave, 0, st, T, k_mat_blend_refl);
				}
				launched("k_mat_blend_refl");
			}
		}
		if(k) lightColour(L[k], aOrder, k < D ? &L[k + 1] : nullptr);
	}
	if(lrc) return lrc;
	level(L[1], nullptr, false);   // (the primary stages read none of a level's packets; rCol must not be left on a B level's)
	if(!pstats) {
		T.bSamples = W.samples; T.bOpacity = L[0].opacity; T.bSel = L[0].sel; T.bCol = L[1].R.rCol;
		SNAIL_LAUNCH(sse, TranspArgs, grid, wave, 0, st, T, k_mat_blend_transp);
		launched("k_mat_blend_transp");
	}
	if(nLights && !lrc) lrc = kind.lights(G);
	if(lrc || pstats) return lrc;   // (a heat launch: the counters alone)
	// both blends are in the sample buffer: the colour stage without one of its own, bytes or the floats k_inst_store goes on from
	if(colPackets) SNAIL_LAUNCH(sse, MatArgs, grid, wave, 0, st, A, k_mat_colour);
	else SNAIL_LAUNCH(sse, MatArgs, grid, wave, 0, st, A, k_mat_final);
	return kind.launched(colPackets ? "k_mat_colour" : "k_mat_final");
}

// The stages of one frame over the np packets of dXY (the kind's lock held) into `frame`, packet-major `bgrPackets` or, when colPackets is given,
// float colours for k_inst_store.  W: level 0; the levels are carved at `arena` (levelsBytes).  The kind's end runs on every way out once its
// begin has succeeded, the first error kept.
template <class K>
int shadeLevels(typename K::Handle *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights,
				const float ambient[3], uint8_t *frame, int pitch, uint8_t *bgrPackets, float *colPackets, const typename K::Bufs &W, char *arena, int maxDepth, bool refl,
				uint64_t *dTrunc, uint64_t *dStats, hipStream_t st, uint32_t *pstats = nullptr) {
	K kind(m, fn, st, pstats, np, nLights);
	if(int rc = kind.begin()) return rc;
	const int rc = levelStages(kind, cam, resx, resy, dXY, lights7, nLights, ambient, frame, pitch, bgrPackets, colPackets, W, arena, maxDepth, refl, dTrunc, dStats);
	const int erc = kind.end();
	return rc ? rc : erc;
}

// One frame's stages into `frame` or packet-major `bgrPackets` (the kind's lock held).  maxDepth 0: the kind's opaque stages, with the one
// mirrored bounce in R (or null); otherwise the levels at `arena`, chain B with refl.
template <class K>
int frameStages(typename K::Handle *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights,
				const float ambient[3], uint8_t *frame, int pitch, uint8_t *bgrPackets, const typename K::Bufs &W, const typename K::BounceBufs *R, char *arena, bool refl,
				int maxDepth, uint64_t *dTrunc, uint64_t *dStats, hipStream_t st) {
	if(!maxDepth) return K::opaque(m, fn, cam, resx, resy, dXY, np, lights7, nLights, ambient, frame, pitch, bgrPackets, W, R, dStats, st);
	return shadeLevels<K>(m, fn, cam, resx, resy, dXY, np, lights7, nLights, ambient, frame, pitch, bgrPackets, nullptr, W, arena, maxDepth, refl, dTrunc, dStats, st);
}

// ... over the handle's next set of intermediates, grown if need be (the kind's lock held); dXY null: the whole frame's cached packet list
template <class K>
int frameSet(typename K::Handle *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights,
			 const float ambient[3], uint8_t *frame, int pitch, uint8_t *bgrPackets, bool refl, int maxDepth, uint64_t *dTrunc, uint64_t *dStats, hipStream_t st) {
	if(!dXY) { if(int rc = m->frameLists.get(resx, resy, &dXY, &np)) return rc; }
	const bool bounce = refl && !maxDepth;
	ShadeSets::Set *Wp = nullptr;
	if(int rc = setsNext(m, np, nLights, bounce, false, st, &Wp)) return rc;
	ShadeSets::Set &W = *Wp;
	if(maxDepth) {
		const size_t want = levelsBytes<typename K::BounceBufs>((size_t)np, nLights, maxDepth, refl);
		if(int rc = levelsGrow(W, W.transp, W.transpBytes, want, want)) return rc;
	}
	typename K::Bufs B;
	B.carve(W.base, (size_t)np);
	typename K::BounceBufs RB;
	if(bounce) RB.carve(W.bounce, (size_t)np, nLights);
	const int rc = frameStages<K>(m, fn, cam, resx, resy, dXY, np, lights7, nLights, ambient, frame, pitch, bgrPackets, B, bounce ? &RB : nullptr, W.transp, refl, maxDepth, dTrunc, dStats, st);
	return setDone(W, fn, rc, st);
}

// The bodies of the _dev and _packets_dev entry points once their arguments and the handle have been judged
template <class K>
int frameDev(typename K::Handle *m, const char *fn, const float cam[13], int resx, int resy, const float *lights7, int nLights, const float ambient[3], bool refl,
			 int maxDepth, uint8_t *frame, int pitch, uint64_t *dTrunc, uint64_t *dStats, void *stream) {
	DeviceGuard guard(m->device);
	std::lock_guard<std::mutex> lock(K::mu(m));
	return frameSet<K>(m, fn, cam, resx, resy, nullptr, 0, lights7, nLights, ambient, frame, pitch, nullptr, refl, maxDepth, dTrunc, dStats, (hipStream_t)stream);
}
template <class K>
int framePacketsDev(typename K::Handle *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets, const float *lights7,
					int nLights, const float ambient[3], bool refl, int maxDepth, uint8_t *bgrPackets, uint64_t *dTrunc, uint64_t *dStats, void *stream) {
	DeviceGuard guard(m->device);
	std::lock_guard<std::mutex> lock(K::mu(m));
	return frameSet<K>(m, fn, cam, resx, resy, dPacketXY, nPackets, lights7, nLights, ambient, nullptr, 0, bgrPackets, refl, maxDepth, dTrunc, dStats, (hipStream_t)stream);
}

// ... and of the _image ones: a whole frame into the caller's pitched host memory.  The arena holds, in this order, the packet list, the kind's
// Bufs, its BounceBufs, the levels, the image and the truncation counter (truncated null: none).
template <class K>
int frameImage(typename K::Handle *m, const char *fn, const float cam[13], int resx, int resy, const float *lights7, int nLights, const float ambient[3], bool refl,
			   int maxDepth, uint8_t *image, int pitch, uint64_t *truncated, uint64_t stats[4]) {
	DeviceGuard guard(m->device);
	HostCallScope hc(K::scene(m), fn);   // (a stream, counters and staging arena of the call's own; the scene handle only lends its free list)
	if(hc.rc) return hc.rc;
	if(int rc = hc.zeroStats()) return rc;
	const int pw = (resx + 15) / 16, ph = (resy + 15) / 16, np = pw * ph;
	const std::vector<int32_t> xy = frameGrid(pw, ph);
	typedef HostCallScope H;
	const bool bounce = refl && !maxDepth;
	const size_t imgBytes = (size_t)pitch * resy, bufBytes = K::Bufs::bytes((size_t)np, nLights), bounceBytes = bounce ? K::BounceBufs::bytes((size_t)np, nLights) : 0,
				 levelBytes = maxDepth ? levelsBytes<typename K::BounceBufs>((size_t)np, nLights, maxDepth, refl) : 0;
	if(int rc = hc.reserve(H::pad(xy.size() * 4) + H::pad(bufBytes) + (bounce ? H::pad(bounceBytes) : 0) + (maxDepth ? H::pad(levelBytes) : 0) + H::pad(imgBytes + 4) +
						   (truncated ? H::pad(8) : 0)))
		return rc;
	void *dXY = nullptr;
	if(int rc = hc.put(&dXY, xy.data(), xy.size() * 4)) return rc;
	typename K::Bufs W;
	W.carve((char *)hc.carve(bufBytes), (size_t)np);
	typename K::BounceBufs RB;
	if(bounce) RB.carve((char *)hc.carve(bounceBytes), (size_t)np, nLights);
	char *arena = maxDepth ? (char *)hc.carve(levelBytes) : nullptr;
	uint8_t *dImg = (uint8_t *)hc.carve(imgBytes + 4);
	uint64_t *dTrunc = truncated ? (uint64_t *)hc.carve(8) : nullptr;
	if(dTrunc) HIP_TRY(hipMemsetAsync(dTrunc, 0, 8, hc.stream()));
	{
		std::lock_guard<std::mutex> lock(K::mu(m));
		if(int rc = frameStages<K>(m, fn, cam, resx, resy, (const int32_t *)dXY, np, lights7, nLights, ambient, dImg, pitch, nullptr, W, bounce ? &RB : nullptr, arena, refl, maxDepth,
								   dTrunc, hc.stats(), hc.stream()))
			return rc;
	}
	HIP_TRY(hipMemcpy2DAsync(image, (size_t)pitch, dImg, (size_t)pitch, (size_t)resx * 3, (size_t)resy, hipMemcpyDeviceToHost, hc.stream()));
	uint64_t got = 0;
	if(truncated) { if(int rc = hc.get(&got, dTrunc, 8)) return rc; }
	if(int rc = hc.finish(stats)) return rc;
	if(truncated) *truncated += got;
	return 0;
}

// the levels one output packet takes under `flags`: snail_materials_level_bytes / snail_instances_materials_level_bytes, and the slicing below
template <class K>
int64_t levelsBytesPerPacket(int nLights, int flags, int maxDepth) {
	if(flags & SNAIL_RENDER_DEPTH) return 0;
	return (int64_t)levelsBytes<typename K::BounceBufs>((flags & SNAIL_RENDER_AA4) ? 4 : 1, nLights, maxDepth, (flags & SNAIL_RENDER_REFLECTIONS) != 0);
}

#define SNAIL_LEVELS_STORE(AA, PL) SNAIL_LAUNCH(sse, InstStoreArgs, dim3(np), dim3(64), 0, st, S, k_inst_store<false, AA, PL>)

// One run of the pipeline over the np packets of dXY with any flags and tint, into packet-major bytes (bgrPackets) or the planes of J's tiles;
// the kind's lock held.  The packet list runs in slices of whole output packets, back to back on st over the same intermediates, so that the
// levels stay within the set's budget (rounding makes the levels of n packets at most n times those of one); the float colours of ALL packets
// and the sub-packet list are kept, and ONE k_inst_store follows the last slice.
// heat (never with SNAIL_RENDER_DEPTH): the per-packet TreeStats instead of the colours -- cleared on st in dPacketStats or, when the caller keeps
// none, in the set's own array; every slice books at its packets' offset in the whole list's array; after the last slice the counters' colours:
// dev_heat::k_heat_store straight into bgrPackets, or with a tint or tile planes dev_heat::k_heat_colours into the set's float colours and the
// same ONE k_inst_store.  No output at all: the counters alone.
template <class K>
int levelsStore(typename K::Handle *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights,
				const float ambient[3], int flags, const float *tint, uint8_t *bgrPackets, const InstTileJob *J, int maxDepth, uint64_t *dTrunc, uint64_t *dStats,
				hipStream_t st, bool heat = false, uint32_t *dPacketStats = nullptr) {
	if(flags & SNAIL_RENDER_DEPTH)   // gVals[1] returns before the full-shading branch: no level runs
		return K::depthStore(m, fn, cam, resx, resy, dXY, np, lights7, nLights, ambient, flags, tint, bgrPackets, J, dStats, st);
	const bool aa = (flags & SNAIL_RENDER_AA4) != 0, refl = (flags & SNAIL_RENDER_REFLECTIONS) != 0;
	const bool floats = heat ? (tint || J) : (aa || tint || J);   // otherwise the lit packets as they are: bytes from k_mat_final (k_heat_store)
	const bool tiles = floats || (heat && aa);   // (a heat launch without colours to reduce: for its sub-packet list alone)
	const int q = aa ? 4 : 1;
	const int rx = aa ? resx * 2 : resx, ry = aa ? resy * 2 : resy;
	const uint64_t one = (uint64_t)levelsBytesPerPacket<K>(nLights, flags, maxDepth);
	const uint64_t budget = std::max(m->levelBudget ? m->levelBudget : (uint64_t)SNAIL_MAT_LEVEL_BUDGET, one);
	const int slice = (int)std::min<uint64_t>(budget / one, (uint64_t)np);   // output packets per slice
	const size_t ns = (size_t)slice * q, n = (size_t)np * q;
	typedef typename K::Handle::TileBufs TileBufs;
	ShadeSets::Set *Wp = nullptr;
	if(int rc = setsNext(m, (int)ns, nLights, false, false, st, &Wp)) return rc;
	ShadeSets::Set &W = *Wp;
	if(tiles) {   // the tile renderer's part for the WHOLE list
		const size_t packets = std::max(W.tilesPackets, n);
		if(int rc = levelsGrow(W, W.tiles, W.tilesPackets, packets, TileBufs::bytes(packets))) return rc;
	}
	{
		const size_t want = std::max(W.transpBytes, levelsBytes<typename K::BounceBufs>(ns, nLights, maxDepth, refl));
		if(int rc = levelsGrow(W, W.transp, W.transpBytes, want, want)) return rc;
	}
	if(heat && !dPacketStats) {
		const size_t packets = std::max(W.pstatsPackets, n);
		if(int rc = levelsGrow(W, W.pstats, W.pstatsPackets, packets, packets * 16)) return rc;
	}
	uint32_t *pst = !heat ? nullptr : dPacketStats ? dPacketStats : W.pstats;
	typename K::Bufs B;
	B.carve(W.base, ns);
	TileBufs T;
	if(tiles) T.carve(W.tiles, n);
	int rc = 0;
	const int32_t *list = dXY;
	if(aa) {
		hipLaunchKernelGGL(dev::k_inst_aa_packets, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const int2 *)dXY, np, (int2 *)T.xy2);
		list = T.xy2;
	}
	if(heat) {
		const hipError_t e = hipMemsetAsync(pst, 0, n * 16, st);
		if(e != hipSuccess) { snail_set_error("%s: hipMemsetAsync: %s", fn, hipGetErrorString(e)); rc = 100 + (int)e; }
	}
	for(int a = 0; a < np && !rc; a += slice) {
		const int cnt = std::min(slice, np - a);
		const size_t at = (size_t)a * q;   // the slice's first packet in `list` and in the colours
		rc = shadeLevels<K>(m, fn, cam, rx, ry, list + at * 2, cnt * q, lights7, nLights, ambient, nullptr, 0, heat || floats ? nullptr : bgrPackets + at * 768,
							!heat && floats ? T.col + at * 768 : nullptr, B, W.transp, maxDepth, refl, dTrunc, dStats, st, heat ? pst + at * 4 : nullptr);
	}
	if(!rc && heat && (floats || bgrPackets)) {   // no new colour arithmetic: the stores of heatmap.inc
		if(floats) hipLaunchKernelGGL(dev_heat::k_heat_colours, dim3((unsigned)n), dim3(64), 0, st, (const unsigned *)pst, (int)n, T.col);
		else if(aa) hipLaunchKernelGGL(dev_heat::k_heat_store<true>, dim3((unsigned)np), dim3(64), 0, st, (const unsigned *)pst, np, bgrPackets);
		else hipLaunchKernelGGL(dev_heat::k_heat_store<false>, dim3((unsigned)np), dim3(64), 0, st, (const unsigned *)pst, np, bgrPackets);
		const hipError_t e = hipGetLastError();
		if(e != hipSuccess) { snail_set_error("%s: the heat store: %s", fn, hipGetErrorString(e)); rc = 100 + (int)e; }
	}
	if(!rc && floats) {
		const SnailScene *s = K::scene(m);   // (the arithmetic and its tables are the scene's: an instanced set's BLASes agree, instancesBegin)
		const bool sse = s->arith == SNAIL_ARITH_HOST_SSE;
		dev::InstStoreArgs S;
		memset(&S, 0, sizeof(S));
		S.hostTab = sse ? s->dTab : nullptr;
		S.in = T.col;
		S.nPackets = np;
		if(tint) { S.tinted = 1; for(int c = 0; c < 3; c++) S.tint[c] = tint[c]; }
		S.bgrPackets = bgrPackets;
		if(J) {
			S.tiles = (const int4 *)J->dTiles; S.packetTile = J->dPacketTile; S.firstPacket = J->dFirst; S.outOff = (const long long *)J->dOff;
			S.out = J->dOut; S.resx = resx; S.resy = resy;
		}
		switch((aa ? 2 : 0) | (J ? 1 : 0)) {
		case 0: SNAIL_LEVELS_STORE(false, false); break;
		case 1: SNAIL_LEVELS_STORE(false, true); break;
		case 2: SNAIL_LEVELS_STORE(true, false); break;
		default: SNAIL_LEVELS_STORE(true, true); break;
		}
		const hipError_t e = hipGetLastError();
		if(e != hipSuccess) { snail_set_error("%s: k_inst_store: %s", fn, hipGetErrorString(e)); rc = 100 + (int)e; }
	}
	return setDone(W, fn, rc, st);
}
#undef SNAIL_LEVELS_STORE

// ---- the host calls around levelsStore; the entry points judge their own arguments first, in their own order ----
int tileRectsOk(const char *fn, const int32_t *coords, int nTiles) {
	for(int k = 0; k < nTiles; k++) {
		const long long x = coords[(size_t)k * 4 + 0], y = coords[(size_t)k * 4 + 1], w = coords[(size_t)k * 4 + 2], hh = coords[(size_t)k * 4 + 3];
		if(w <= 0 || hh <= 0 || x < 0 || y < 0 || x + w > (1 << 24) || y + hh > (1 << 24)) {
			snail_set_error("%s: tile %d: bad rect %lld,%lld %lldx%lld", fn, k, x, y, w, hh);
			return 1;
		}
	}
	return 0;
}

// a tile list (nTiles > 0, rects judged) into the caller's `data` at `offsets`, through the set's ONE cached tile job.  `store`: levelsStore<K>, or
// matStoreStep (matShadeStore, the opaque stages), called with levelsStore's arguments; truncated null: a call without a truncation counter.
template <class K, class Store>
int renderTilesHost(typename K::Handle *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *coords, const int64_t *offsets, int nTiles,
					const float *lights7, int nLights, const float ambient[3], int flags, const float *tint, uint8_t *data, int maxDepth, uint64_t *truncated,
					uint64_t stats[4], bool heat, Store store) {
	std::lock_guard<std::mutex> renderLock(m->renderMu);   // one cached tile job per set: its calls take turns
	DeviceGuard guard(m->device);
	HostCallScope hc(K::scene(m), fn);   // (a stream, counters and staging arena of the call's own; the scene handle only lends its free list)
	if(hc.rc) return hc.rc;
	if(!m->tileJob) m->tileJob = new InstTileJob();
	InstTileJob &J = *m->tileJob;
	if(int rc = buildInstTileJob(J, resx, resy, coords, nTiles)) return rc;
	if(stats) { if(int rc = hc.zeroStats()) return rc; }
	uint64_t *dTrunc = nullptr;
	if(truncated) {
		if(int rc = hc.reserve(HostCallScope::pad(8))) return rc;
		dTrunc = (uint64_t *)hc.carve(8);
		HIP_TRY(hipMemsetAsync(dTrunc, 0, 8, hc.stream()));
	}
	{
		std::lock_guard<std::mutex> lock(K::mu(m));
		if(int rc = store(m, fn, cam, resx, resy, J.dXY, J.nPackets, lights7, nLights, ambient, flags, tint, nullptr, &J, maxDepth, dTrunc, stats ? hc.stats() : nullptr, hc.stream(),
						  heat, nullptr))
			return rc;
	}
	HIP_TRY(hipMemcpyAsync(J.hPinned, J.dOut, J.planarBytes, hipMemcpyDeviceToHost, hc.stream()));
	uint64_t got = 0;
	if(truncated) { if(int rc = hc.get(&got, dTrunc, 8)) return rc; }
	if(int rc = hc.finish(stats)) return rc;
	if(truncated) *truncated += got;
	for(int k = 0; k < nTiles; k++)
		memcpy(data + offsets[k], J.hPinned + J.compactOff[(size_t)k], (size_t)3 * coords[(size_t)k * 4 + 2] * coords[(size_t)k * 4 + 3]);
	return 0;
}

// a whole frame into the caller's pitched `image`, packet-major bytes from `store` first
template <class K, class Store>
int renderFrameHost(typename K::Handle *m, const char *fn, const float cam[13], int resx, int resy, const float *lights7, int nLights, const float ambient[3], int flags,
					uint8_t *image, int pitch, int maxDepth, uint64_t *truncated, uint64_t stats[4], bool heat, Store store) {
	DeviceGuard guard(m->device);
	HostCallScope hc(K::scene(m), fn);
	if(hc.rc) return hc.rc;
	if(stats) { if(int rc = hc.zeroStats()) return rc; }
	const int np = ((resx + 15) / 16) * ((resy + 15) / 16);
	const size_t row = (size_t)resx * 3;
	typedef HostCallScope H;
	if(int rc = hc.reserve(H::pad((size_t)np * 768) + H::pad(row * resy + 4) + (truncated ? H::pad(8) : 0))) return rc;
	uint8_t *bgr = (uint8_t *)hc.carve((size_t)np * 768), *dImg = (uint8_t *)hc.carve(row * resy + 4);
	uint64_t *dTrunc = truncated ? (uint64_t *)hc.carve(8) : nullptr;
	if(dTrunc) HIP_TRY(hipMemsetAsync(dTrunc, 0, 8, hc.stream()));
	{
		std::lock_guard<std::mutex> lock(K::mu(m));
		const int32_t *dXY = nullptr;
		int n = 0;
		if(int rc = m->frameLists.get(resx, resy, &dXY, &n)) return rc;
		// (a heat frame's packets carry no tint and no planes: their bytes come from k_heat_store, which k_heat_colours + k_inst_store equal byte for byte)
		if(int rc = store(m, fn, cam, resx, resy, dXY, np, lights7, nLights, ambient, flags, nullptr, bgr, nullptr, maxDepth, dTrunc, stats ? hc.stats() : nullptr, hc.stream(), heat, nullptr))
			return rc;
		// (under the lock: the cached frame list may be dropped by a later call, which first waits for everything enqueued)
		if(int rc = snail_packets_bgr_to_frame_dev(dXY, np, resx, resy, bgr, dImg, (int)row, hc.stream())) return rc;
	}
	HIP_TRY(hipMemcpy2DAsync(image, (size_t)pitch, dImg, row, row, (size_t)resy, hipMemcpyDeviceToHost, hc.stream()));
	uint64_t got = 0;
	if(truncated) { if(int rc = hc.get(&got, dTrunc, 8)) return rc; }
	if(int rc = hc.finish(stats)) return rc;
	if(truncated) *truncated += got;
	return 0;
}

} // namespace
