// materials_tree_host.inc -- the C-ABI of include/snail_materials_tree.h: the transparency continuation together with the mirrored bounce, the
// tile renderer, 4x antialiasing, depth shading and the tint; included by snail_hip.hip after materials_transparency_host.inc.  matShadeTree is
// matShadeTransp generalised: the way down of chain A, then for k = D .. 0 the B chain of A_k (mirror, walk, sample, generator / walk / sample
// down to level D, truncation count, way back up), the reflection blend into A_k, its transparency blend, lights and colour.  matTreeStore runs
// it over a packet list in slices that keep the levels within the set's budget, and hands the float colours to k_inst_store.
#include "../../include/snail_materials_tree.h"

namespace {

// the levels of n packets: L[0]'s opacity / selector / order + D A-levels, and with the bounce D + 1 B-levels
size_t treeBytes(size_t n, int nLights, int depth, bool refl) { return transpBytes(n, nLights, depth) + (refl ? (size_t)(depth + 1) * TranspLevel::bytes(n, nLights) : 0); }

// The stages of one frame over the np packets of dXY (the scene's mu held) into `frame`, packet-major `bgrPackets` or, when colPackets is given,
// float colours for k_inst_store.  W: level 0; the levels are carved at `arena` (treeBytes).  Without refl the sequence is matShadeTransp's.
// pstats (a heat-map launch, include/snail_materials_heatmap.h; cleared by the caller): every stage that books into dStats -- the walks, the lights,
// the generators and the mirrors -- also books per packet there, through its PSTATS / _heat instantiation, at the packet's index in dXY; the stages
// that only make colours (both blends, the colour stages, k_mat_final) are left out, and frame / bgrPackets / colPackets are not written: no
// selector, normal or position a counter depends on reads a colour.
#define SNAIL_TREE_LAUNCH(ARGS_T, GRID, REC, K)                                                                                              \
	do {                                                                                                                                   \
		if(pstats) SNAIL_LAUNCH(sse, ARGS_T, GRID, wave, 0, st, REC, K##_heat);                                                            \
		else SNAIL_LAUNCH(sse, ARGS_T, GRID, wave, 0, st, REC, K);                                                                         \
	} while(0)
int matShadeTree(SnailMaterials *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights,
				 const float ambient[3], uint8_t *frame, int pitch, uint8_t *bgrPackets, float *colPackets, const SnailMaterials::Bufs &W, char *arena, int maxDepth,
				 bool refl, uint64_t *dTrunc, uint64_t *dStats, hipStream_t st, uint32_t *pstats = nullptr) {
	SnailScene *s = m->scene;
	SceneUse use(s, st);
	if(use.rc) return use.rc;
	const int D = maxDepth;
	TranspLevel L[SNAIL_MAT_TRANSP_MAX_DEPTH + 1], M[SNAIL_MAT_TRANSP_MAX_DEPTH + 1];   // chain A; chain B: ONE set of levels, reused by every k (the stream orders them)
	char *p = L[0].carveExtra(arena, (size_t)np);
	for(int k = 1; k <= D; k++) p = L[k].carve(p, (size_t)np, nLights);
	if(refl) for(int j = 0; j <= D; j++) p = M[j].carve(p, (size_t)np, nLights);
	if(int rc = launchPrimary(s, cam, resx, resy, 0, 0, 0, 0, dXY, np, W.hitT, W.hitU, W.hitV, W.hitId, dStats, st, nullptr, false, nullptr, nullptr, nullptr, nullptr, 0, pstats))
		return rc;
	dev::TreeArgs G;
	memset(&G, 0, sizeof(G));
	dev::TranspArgs &T = G.t;
	dev::MatArgs &A = T.m;
	matFillArgs(m, A, cam, resx, resy, dXY, np);
	A.s.nLights = nLights;
	for(int n = 0; n < nLights; n++) for(int k = 0; k < 7; k++) A.s.lights[n][k] = lights7[n * 7 + k];
	for(int c = 0; c < 3; c++) { A.s.ambient[c] = ambient[c]; A.s.color[c] = 1.0f; }
	A.s.hitT = W.hitT; A.s.hitId = W.hitId; A.hitU = W.hitU; A.hitV = W.hitV;
	A.samples = W.samples; A.s.sDist = W.sDist;
	A.s.frame = frame; A.s.pitch = pitch; A.s.bgrPackets = bgrPackets;
	A.s.colPackets = colPackets;
	A.s.stats = (dev::u64 *)dStats;
	A.s.pstats = pstats;
	A.rUVStride = 8;
	T.trunc = (unsigned long long *)dTrunc;
	const bool sse = s->arith == SNAIL_ARITH_HOST_SSE;
	const dim3 grid(np), wave(64);
	// a level's generic packets as the stages' source, under its own order list (null: every packet)
	auto level = [&](const TranspLevel &X, const int32_t *order) {
		const SnailMaterials::BounceBufs &R = X.R;
		A.s.rOrg = R.rOrg; A.s.rDir = R.rDir; A.s.rIDir = R.rIDir; A.s.rMask = R.rMask; A.s.rDist = R.rDist; A.s.rObj = R.rObj; A.s.rCol = R.rCol;
		A.rU = R.bary; A.rV = R.bary + 4;
		A.nSamples = R.nSamples; A.nSDist = R.nSDist;
		T.inOrder = order;
	};
	int lrc = 0;   // the first error of the way back up, kept while the origin-relative copies are booked
	auto launched = [&](const char *what) {
		const hipError_t e = hipGetLastError();
		if(e != hipSuccess && !lrc) { snail_set_error("%s: %s: %s", fn, what, hipGetErrorString(e)); lrc = 100 + (int)e; }
	};
	// the ordered walk of a level's packets (order null: all of them, as the bounce walks its mirrored packets) and its sample stage
	auto walkSample = [&](const TranspLevel &X, const int32_t *order) {
		if(lrc) return;
		// the walk reads the barycentrics it was given and writes them back for lanes without a hit: zeros, not what the buffer last held
		const hipError_t e = hipMemsetAsync(X.R.bary, 0, (size_t)np * 256 * 8, st);
		if(e != hipSuccess) { snail_set_error("%s: hipMemsetAsync: %s", fn, hipGetErrorString(e)); lrc = 100 + (int)e; return; }
		if(order) lrc = launchRays(s, false, np, 64, 0, X.R.rOrg, X.R.rDir, X.R.rIDir, X.R.rMask, X.R.rDist, X.R.rObj, X.R.bary, dStats, st, order, nullptr, np, nullptr, 0, pstats);
		else lrc = launchRays(s, false, np, 64, 0, X.R.rOrg, X.R.rDir, X.R.rIDir, X.R.rMask, X.R.rDist, X.R.rObj, X.R.bary, dStats, st, nullptr, nullptr, 0, nullptr, 0, pstats);
		if(lrc) return;
		level(X, order);
		T.opacity = X.opacity; T.sel = X.sel;
		SNAIL_LAUNCH(sse, TranspArgs, grid, wave, 0, st, T, k_mat_sample_transp_rays);
		launched("k_mat_sample_transp_rays");
	};
	// the generator: from level `from` (its rays, hits, selector and own order list) into level `to`'s packets and order list
	auto generate = [&](const TranspLevel &from, const int32_t *fromOrder, const TranspLevel &to) {
		if(lrc) return;
		level(to, fromOrder);
		T.order = to.order;
		T.cT = from.R.rDist; T.cSel = from.sel;
		T.cOrg = from.R.rOrg; T.cDir = from.R.rDir; T.cIDir = from.R.rIDir;
		SNAIL_TREE_LAUNCH(TranspArgs, grid, T, k_mat_continue_rays);
		launched("k_mat_continue_rays");
	};
	auto truncated = [&](const TranspLevel &X, const int32_t *order) {
		if(lrc) return;
		level(X, order);
		T.bSel = X.sel;
		SNAIL_LAUNCH(sse, TranspArgs, grid, wave, 0, st, T, k_mat_truncated);
		launched("k_mat_truncated");
	};
	const dim3 lgrid(np, nLights > 0 ? nLights : 1);
	// a nested level's way back up: (the blend from the deeper level's colour,) its lights, its colour
	auto lightColour = [&](const TranspLevel &X, const int32_t *order, const TranspLevel *deeper) {
		if(lrc) return;
		level(X, order);
		if(deeper && !pstats) {
			T.bSamples = X.R.nSamples; T.bOpacity = X.opacity; T.bSel = X.sel; T.bCol = deeper->R.rCol;
			SNAIL_LAUNCH(sse, TranspArgs, grid, wave, 0, st, T, k_mat_blend_transp);
			launched("k_mat_blend_transp");
		}
		if(nLights && !lrc) {
			if(pstats) {
				if(useDeep(s)) SNAIL_LAUNCH(sse, TranspArgs, lgrid, wave, 0, st, T, k_mat_light_transp_heat<true>);
				else SNAIL_LAUNCH(sse, TranspArgs, lgrid, wave, 0, st, T, k_mat_light_transp_heat<false>);
			} else if(useDeep(s)) SNAIL_LAUNCH(sse, TranspArgs, lgrid, wave, 0, st, T, k_mat_light_transp<true>);
			else SNAIL_LAUNCH(sse, TranspArgs, lgrid, wave, 0, st, T, k_mat_light_transp<false>);
			launched("k_mat_light_transp");
		}
		if(!lrc && !pstats) { SNAIL_LAUNCH(sse, TranspArgs, grid, wave, 0, st, T, k_mat_colour_transp); launched("k_mat_colour_transp"); }
	};

	// ---- the way down of chain A: sample, then per level generator -> ordered walk -> nested sample ----
	T.opacity = L[0].opacity; T.sel = L[0].sel; T.inOrder = nullptr;
	SNAIL_LAUNCH(sse, TranspArgs, grid, wave, 0, st, T, k_mat_sample_transp);
	HIP_TRY(hipGetLastError());
	for(int k = 1; k <= D; k++) {
		if(k == 1) {
			level(L[1], nullptr);
			T.order = L[1].order;
			T.cT = W.hitT; T.cSel = L[0].sel;
			T.cOrg = T.cDir = T.cIDir = nullptr;
			SNAIL_TREE_LAUNCH(TranspArgs, grid, T, k_mat_continue);
			launched("k_mat_continue");
		} else generate(L[k - 1], L[k - 1].order, L[k]);
		walkSample(L[k], L[k].order);
		if(lrc) return lrc;
	}
	// the lanes the deepest level would still select: counted, then treated as not selected
	truncated(L[D], L[D].order);
	if(lrc) return lrc;

	// ---- the way back up ----
	int relWhich[SNAIL_MAX_LIGHTS];
	for(int n = 0; n < SNAIL_MAX_LIGHTS; n++) { relWhich[n] = -1; A.s.relLight[n] = nullptr; }
	// (every origin-relative copy taken here is booked as used on st on EVERY way out, first error kept: matShade's rule; the lights of every
	// level of both chains walk from the same origins: the same copies)
	if(nLights && A.s.pack && !useDeep(s))
		for(int n = 0; n < nLights && !lrc; n++) lrc = relFor(s, A.s.lights[n], st, &A.s.relLight[n], &relWhich[n]);
	for(int k = D; k >= 0 && !lrc; k--) {
		const int32_t *aOrder = k ? L[k].order : nullptr;
		if(refl) {
			// the B chain of A_k: the mirrored call B_{k,k} (every packet of A_k, hit or not) and its continuations down to level D
			const int32_t *bOrder = k ? M[k].order : nullptr;   // (k = 0: every packet, the bounce's walk)
			if(k) {
				level(L[k], aOrder);
				G.oOrg = M[k].R.rOrg; G.oDir = M[k].R.rDir; G.oIDir = M[k].R.rIDir; G.oDist = M[k].R.rDist; G.oObj = M[k].R.rObj; G.oMask = M[k].R.rMask;
				G.oOrder = M[k].order;
				SNAIL_TREE_LAUNCH(TreeArgs, grid, G, k_mat_mirror_rays);
				launched("k_mat_mirror_rays");
			} else {
				level(M[0], nullptr);
				SNAIL_TREE_LAUNCH(MatArgs, grid, A, k_mat_mirror);
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
					level(L[k], aOrder);
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
	if(!lrc && !pstats) {
		level(L[1], nullptr);   // (the primary stages read none of a level's packets; rCol must not be left on a B level's)
		T.bSamples = W.samples; T.bOpacity = L[0].opacity; T.bSel = L[0].sel; T.bCol = L[1].R.rCol;
		SNAIL_LAUNCH(sse, TranspArgs, grid, wave, 0, st, T, k_mat_blend_transp);
		launched("k_mat_blend_transp");
	}
	if(nLights && !lrc && pstats) {
		if(useDeep(s)) SNAIL_LAUNCH(sse, MatArgs, lgrid, wave, 0, st, A, k_mat_light_heat<true>);
		else SNAIL_LAUNCH(sse, MatArgs, lgrid, wave, 0, st, A, k_mat_light_heat<false>);
		launched("k_mat_light");
	} else if(nLights && !lrc) {
		if(useDeep(s)) SNAIL_LAUNCH(sse, MatArgs, lgrid, wave, 0, st, A, k_mat_light<true>);
		else SNAIL_LAUNCH(sse, MatArgs, lgrid, wave, 0, st, A, k_mat_light<false>);
		launched("k_mat_light");
	}
	for(int n = 0; n < nLights; n++)
		if(relWhich[n] >= 0) { const int urc = relUsed(s, relWhich[n], st); if(!lrc) lrc = urc; }
	if(lrc || pstats) return lrc;
	// both blends are in the sample buffer: the colour stage without one of its own, bytes or the floats k_inst_store goes on from
	if(colPackets) SNAIL_LAUNCH(sse, MatArgs, grid, wave, 0, st, A, k_mat_colour);
	else SNAIL_LAUNCH(sse, MatArgs, grid, wave, 0, st, A, k_mat_final);
	HIP_TRY(hipGetLastError());
	return 0;
}
#undef SNAIL_TREE_LAUNCH

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

int64_t matTreeLevelBytes(int nLights, int flags, int maxDepth) {
	if(flags & SNAIL_RENDER_DEPTH) return 0;
	return (int64_t)treeBytes((flags & SNAIL_RENDER_AA4) ? 4 : 1, nLights, maxDepth, (flags & SNAIL_RENDER_REFLECTIONS) != 0);
}

#define SNAIL_TREE_STORE(AA, PL) SNAIL_LAUNCH(sse, InstStoreArgs, dim3(np), dim3(64), 0, st, S, k_inst_store<false, AA, PL>)

// One run of the pipeline over the np packets of dXY with any flags and tint, into packet-major bytes (bgrPackets) or the planes of J's tiles;
// the scene's mu held.  The packet list runs in slices of whole output packets, back to back on st over the same intermediates, so that the
// levels stay within the set's budget (rounding makes the levels of n packets at most n times those of one); the float colours of ALL packets
// and the sub-packet list are kept, and ONE k_inst_store follows the last slice.
// heat (include/snail_materials_heatmap.h; never with SNAIL_RENDER_DEPTH): the per-packet TreeStats instead of the colours -- cleared on st in
// dPacketStats or, when the caller keeps none, in the set's own array; every slice books at its packets' offset in the whole list's array; after
// the last slice the counters' colours: dev_heat::k_heat_store straight into bgrPackets, or with a tint or tile planes dev_heat::k_heat_colours
// into the set's float colours and the same ONE k_inst_store.  No output at all: the counters alone.
int matTreeStore(SnailMaterials *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights,
				 const float ambient[3], int flags, const float *tint, uint8_t *bgrPackets, const InstTileJob *J, int maxDepth, uint64_t *dTrunc, uint64_t *dStats,
				 hipStream_t st, bool heat = false, uint32_t *dPacketStats = nullptr) {
	if(flags & SNAIL_RENDER_DEPTH)   // gVals[1] returns before the full-shading branch: no level runs
		return matShadeStore(m, fn, cam, resx, resy, dXY, np, lights7, nLights, ambient, flags, tint, bgrPackets, J, dStats, st);
	SnailScene *s = m->scene;
	const bool aa = (flags & SNAIL_RENDER_AA4) != 0, refl = (flags & SNAIL_RENDER_REFLECTIONS) != 0;
	const bool floats = heat ? (tint || J) : (aa || tint || J);   // otherwise the lit packets as they are: bytes from k_mat_final (k_heat_store)
	const int q = aa ? 4 : 1;
	const int rx = aa ? resx * 2 : resx, ry = aa ? resy * 2 : resy;
	const uint64_t one = (uint64_t)matTreeLevelBytes(nLights, flags, maxDepth);
	const uint64_t budget = std::max(m->levelBudget ? m->levelBudget : (uint64_t)SNAIL_MAT_LEVEL_BUDGET, one);
	const int slice = (int)std::min<uint64_t>(budget / one, (uint64_t)np);   // output packets per slice
	const size_t ns = (size_t)slice * q, n = (size_t)np * q;
	SnailMaterials::Set *Wp = nullptr;
	if(int rc = matNextSet(m, (int)ns, nLights, false, false, st, &Wp)) return rc;
	SnailMaterials::Set &W = *Wp;
	if(floats && (!W.tiles || W.tilesPackets < n)) {   // the tile renderer's part for the WHOLE list; grown under matNextSet's rule
		HIP_TRY(hipDeviceSynchronize());
		if(W.tiles) (void)hipFree(W.tiles);
		const size_t packets = std::max(W.tilesPackets, n);
		W.tiles = nullptr; W.tilesPackets = 0; W.used = false;
		HIP_TRY(hipMalloc((void **)&W.tiles, SnailMaterials::TileBufs::bytes(packets)));
		W.tilesPackets = packets;
	}
	const size_t want = treeBytes(ns, nLights, maxDepth, refl);
	if(!W.transp || W.transpBytes < want) {   // grown: its previous user may still be running
		HIP_TRY(hipDeviceSynchronize());
		if(W.transp) (void)hipFree(W.transp);
		W.transp = nullptr; W.transpBytes = 0; W.used = false;
		HIP_TRY(hipMalloc((void **)&W.transp, want));
		W.transpBytes = want;
	}
	uint32_t *pst = nullptr;
	if(heat) {
		if(!dPacketStats && (!W.pstats || W.pstatsPackets < n)) {   // grown under matNextSet's rule
			HIP_TRY(hipDeviceSynchronize());
			if(W.pstats) (void)hipFree(W.pstats);
			const size_t packets = std::max(W.pstatsPackets, n);
			W.pstats = nullptr; W.pstatsPackets = 0; W.used = false;
			HIP_TRY(hipMalloc((void **)&W.pstats, packets * 16));
			W.pstatsPackets = packets;
		}
		pst = dPacketStats ? dPacketStats : W.pstats;
	}
	SnailMaterials::Bufs B;
	B.carve(W.base, ns);
	SnailMaterials::TileBufs T;
	if(floats) T.carve(W.tiles, n);
	int rc = 0;
	const int32_t *list = dXY;
	if(aa && !floats) {   // (a heat launch without colours to reduce: the sub-packet list needs the tile part's list alone)
		if(!W.tiles || W.tilesPackets < n) {
			HIP_TRY(hipDeviceSynchronize());
			if(W.tiles) (void)hipFree(W.tiles);
			const size_t packets = std::max(W.tilesPackets, n);
			W.tiles = nullptr; W.tilesPackets = 0; W.used = false;
			HIP_TRY(hipMalloc((void **)&W.tiles, SnailMaterials::TileBufs::bytes(packets)));
			W.tilesPackets = packets;
		}
		T.carve(W.tiles, n);
	}
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
		if(heat) rc = matShadeTree(m, fn, cam, rx, ry, list + at * 2, cnt * q, lights7, nLights, ambient, nullptr, 0, nullptr, nullptr, B, W.transp, maxDepth, refl, dTrunc, dStats, st, pst + at * 4);
		else rc = matShadeTree(m, fn, cam, rx, ry, list + at * 2, cnt * q, lights7, nLights, ambient, nullptr, 0, floats ? nullptr : bgrPackets + at * 768,
							   floats ? T.col + at * 768 : nullptr, B, W.transp, maxDepth, refl, dTrunc, dStats, st);
	}
	if(!rc && heat && (floats || bgrPackets)) {   // no new colour arithmetic: the stores of heatmap.inc
		if(floats) hipLaunchKernelGGL(dev_heat::k_heat_colours, dim3((unsigned)n), dim3(64), 0, st, (const unsigned *)pst, (int)n, T.col);
		else if(aa) hipLaunchKernelGGL(dev_heat::k_heat_store<true>, dim3((unsigned)np), dim3(64), 0, st, (const unsigned *)pst, np, bgrPackets);
		else hipLaunchKernelGGL(dev_heat::k_heat_store<false>, dim3((unsigned)np), dim3(64), 0, st, (const unsigned *)pst, np, bgrPackets);
		const hipError_t e = hipGetLastError();
		if(e != hipSuccess) { snail_set_error("%s: the heat store: %s", fn, hipGetErrorString(e)); rc = 100 + (int)e; }
	}
	if(!rc && floats) {
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
		case 0: SNAIL_TREE_STORE(false, false); break;
		case 1: SNAIL_TREE_STORE(false, true); break;
		case 2: SNAIL_TREE_STORE(true, false); break;
		default: SNAIL_TREE_STORE(true, true); break;
		}
		const hipError_t e = hipGetLastError();
		if(e != hipSuccess) { snail_set_error("%s: k_inst_store: %s", fn, hipGetErrorString(e)); rc = 100 + (int)e; }
	}
	return matSetDone(W, fn, rc, st);
}
#undef SNAIL_TREE_STORE

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
	return matTreeStore(m, fn, cam, resx, resy, dPacketXY, nPackets, lights7, nLights, ambient, flags, tint, bgrPackets, nullptr, maxDepth, dTruncated, dStats, (hipStream_t)stream);
}

int snail_materials_tree_render_tiles(SnailMaterials *m, const float cam[13], int resx, int resy, const int32_t *coords, const int64_t *offsets, int nTiles,
									  const float *lights7, int nLights, const float ambient[3], int flags, const float *tint, uint8_t *data, int maxDepth,
									  uint64_t *truncated, uint64_t stats[4]) {
	const char *fn = "snail_materials_tree_render_tiles";
	if(int rc = matTreeArgsOk(fn, cam, resx, resy, lights7, nLights, ambient, flags, tint, maxDepth, truncated)) return rc;
	if(nTiles > 0 && (!coords || !offsets || !data)) { snail_set_error("%s: null buffer", fn); return 1; }
	for(int k = 0; k < nTiles; k++) {
		const long long x = coords[(size_t)k * 4 + 0], y = coords[(size_t)k * 4 + 1], w = coords[(size_t)k * 4 + 2], hh = coords[(size_t)k * 4 + 3];
		if(w <= 0 || hh <= 0 || x < 0 || y < 0 || x + w > (1 << 24) || y + hh > (1 << 24)) {
			snail_set_error("%s: tile %d: bad rect %lld,%lld %lldx%lld", fn, k, x, y, w, hh);
			return 1;
		}
	}
	if(int rc = checkMaterialsAny(m, fn)) return rc;
	if(nTiles <= 0) return 0;
	std::lock_guard<std::mutex> renderLock(m->renderMu);   // one cached tile job per set: its calls take turns
	DeviceGuard guard(m->device);
	HostCallScope hc(m->scene, fn);
	if(hc.rc) return hc.rc;
	if(!m->tileJob) m->tileJob = new InstTileJob();
	InstTileJob &J = *m->tileJob;
	if(int rc = buildInstTileJob(J, resx, resy, coords, nTiles)) return rc;
	if(stats) { if(int rc = hc.zeroStats()) return rc; }
	if(int rc = hc.reserve(HostCallScope::pad(8))) return rc;
	uint64_t *dTrunc = (uint64_t *)hc.carve(8);
	HIP_TRY(hipMemsetAsync(dTrunc, 0, 8, hc.stream()));
	{
		SNAIL_LOCK(m->scene);
		if(int rc = matTreeStore(m, fn, cam, resx, resy, J.dXY, J.nPackets, lights7, nLights, ambient, flags, tint, nullptr, &J, maxDepth, dTrunc, stats ? hc.stats() : nullptr,
								 hc.stream()))
			return rc;
	}
	HIP_TRY(hipMemcpyAsync(J.hPinned, J.dOut, J.planarBytes, hipMemcpyDeviceToHost, hc.stream()));
	uint64_t got = 0;
	if(int rc = hc.get(&got, dTrunc, 8)) return rc;
	if(int rc = hc.finish(stats)) return rc;
	*truncated += got;
	for(int k = 0; k < nTiles; k++)
		memcpy(data + offsets[k], J.hPinned + J.compactOff[(size_t)k], (size_t)3 * coords[(size_t)k * 4 + 2] * coords[(size_t)k * 4 + 3]);
	return 0;
}

int snail_materials_tree_render_frame(SnailMaterials *m, const float cam[13], int resx, int resy, const float *lights7, int nLights, const float ambient[3], int flags,
									  uint8_t *image, int pitch, int maxDepth, uint64_t *truncated, uint64_t stats[4]) {
	const char *fn = "snail_materials_tree_render_frame";
	if(int rc = matTreeArgsOk(fn, cam, resx, resy, lights7, nLights, ambient, flags, nullptr, maxDepth, truncated)) return rc;
	if(!image || pitch < resx * 3) { snail_set_error("%s: null image or a pitch below 3 * resx", fn); return 1; }
	if(int rc = checkMaterialsAny(m, fn)) return rc;
	DeviceGuard guard(m->device);
	HostCallScope hc(m->scene, fn);
	if(hc.rc) return hc.rc;
	if(stats) { if(int rc = hc.zeroStats()) return rc; }
	const int np = ((resx + 15) / 16) * ((resy + 15) / 16);
	const size_t row = (size_t)resx * 3;
	typedef HostCallScope H;
	if(int rc = hc.reserve(H::pad((size_t)np * 768) + H::pad(row * resy + 4) + H::pad(8))) return rc;
	uint8_t *bgr = (uint8_t *)hc.carve((size_t)np * 768), *dImg = (uint8_t *)hc.carve(row * resy + 4);
	uint64_t *dTrunc = (uint64_t *)hc.carve(8);
	HIP_TRY(hipMemsetAsync(dTrunc, 0, 8, hc.stream()));
	{
		SNAIL_LOCK(m->scene);
		const int32_t *dXY = nullptr;
		int n = 0;
		if(int rc = matFrameList(m, resx, resy, &dXY, &n)) return rc;
		if(int rc = matTreeStore(m, fn, cam, resx, resy, dXY, np, lights7, nLights, ambient, flags, nullptr, bgr, nullptr, maxDepth, dTrunc, stats ? hc.stats() : nullptr, hc.stream()))
			return rc;
		// (under mu: the cached frame list may be dropped by a later call, which first waits for everything enqueued)
		if(int rc = snail_packets_bgr_to_frame_dev(dXY, np, resx, resy, bgr, dImg, (int)row, hc.stream())) return rc;
	}
	HIP_TRY(hipMemcpy2DAsync(image, (size_t)pitch, dImg, row, row, (size_t)resy, hipMemcpyDeviceToHost, hc.stream()));
	uint64_t got = 0;
	if(int rc = hc.get(&got, dTrunc, 8)) return rc;
	if(int rc = hc.finish(stats)) return rc;
	*truncated += got;
	return 0;
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
	return matTreeLevelBytes(nLights, flags, maxDepth);
}

} // extern "C"
