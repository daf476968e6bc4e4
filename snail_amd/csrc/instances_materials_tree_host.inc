// instances_materials_tree_host.inc -- the C-ABI of include/snail_instances_materials_tree.h: the transparency continuation of an instanced scene
// together with the mirrored bounce, the tile renderer, 4x antialiasing, depth shading and the tint; included by snail_hip.hip after
// instances_materials_transparency_host.inc.  The instanced twin of materials_tree_host.inc, function for function: imatShadeTree is
// imatShadeTransp generalised by imatNested as matShadeTree is matShadeTransp generalised by the bounce -- the way down of chain A, then for
// k = D .. 0 the B chain of A_k (mirror, walk, sample, generator / walk / sample down to level D, truncation count, way back up), the reflection
// blend into A_k, its transparency blend, lights and colour.  imatTreeStore runs it over a packet list in slices that keep the levels within the
// set's budget, and hands the float colours to k_inst_store.  No stage is new: the kernels are those of instances*.inc, materials*.inc and
// instances_shade.inc, unchanged (instances_materials_tree.inc).
#include "../../include/snail_instances_materials_tree.h"

namespace {

// the levels of n packets: L[0]'s opacity / selector / order + D A-levels, and with the bounce D + 1 B-levels
size_t imatTreeBytes(size_t n, int nLights, int depth, bool refl) {
	return imatTranspBytes(n, nLights, depth) + (refl ? (size_t)(depth + 1) * ITranspLevel::bytes(n, nLights) : 0);
}

// The stages of one frame over the np packets of dXY (the handle's mu held) into packet-major `bgrPackets` or, when colPackets is given, float
// colours for k_inst_store.  W: level 0; the levels are carved at `arena` (imatTreeBytes).  Without refl the sequence is imatShadeTransp's.
// Every launch is booked through instancesBegin / instancesEnd, so the frame is ordered against snail_instances_update and
// snail_instances_rebuild_dev as a walk is.
// pstats (a heat-map launch, include/snail_instances_materials_heatmap.h; cleared by the caller): every stage that books into dStats -- the walks, the
// lights, the generators and the mirrors -- also books per packet there, through its PSTATS / _heat instantiation (k_inst_frame: through
// InstArgs::pstats), at the packet's index in dXY; the stages that only make colours (both blends, the colour stages, k_mat_final) are left out, and
// bgrPackets / colPackets are not written: no selector, normal or position a counter depends on reads a colour.
#define SNAIL_ITREE_LAUNCH_PSTATS(ARGS_T, GRID, REC, K)                                                                                       \
	do {                                                                                                                                   \
		if(pstats) SNAIL_LAUNCH(sse, ARGS_T, GRID, wave, 0, st, REC, K##_heat);                                                            \
		else SNAIL_LAUNCH(sse, ARGS_T, GRID, wave, 0, st, REC, K);                                                                         \
	} while(0)
// (... of a kernel with a <DEEP> argument)
#define SNAIL_ITREE_LAUNCH_PSTATS_DEEP(ARGS_T, GRID, REC, K)                                                                                  \
	do {                                                                                                                                   \
		if(pstats) {                                                                                                                       \
			if(deep) SNAIL_LAUNCH(sse, ARGS_T, GRID, wave, 0, st, REC, K##_heat<true>);                                                    \
			else SNAIL_LAUNCH(sse, ARGS_T, GRID, wave, 0, st, REC, K##_heat<false>);                                                       \
		} else if(deep) SNAIL_LAUNCH(sse, ARGS_T, GRID, wave, 0, st, REC, K<true>);                                                        \
		else SNAIL_LAUNCH(sse, ARGS_T, GRID, wave, 0, st, REC, K<false>);                                                                  \
	} while(0)
int imatShadeTree(SnailInstancesMaterials *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights,
				  const float ambient[3], uint8_t *bgrPackets, float *colPackets, const SnailInstancesMaterials::Bufs &W, char *arena, int maxDepth, bool refl,
				  uint64_t *dTrunc, uint64_t *dStats, hipStream_t st, uint32_t *pstats = nullptr) {
	SnailInstances *h = m->inst;
	dev::InstArgs I;
	bool sse, deep;
	if(int rc = instancesBegin(h, fn, I, &sse, &deep, st)) return rc;
	const int D = maxDepth;
	ITranspLevel L[SNAIL_MAT_TRANSP_MAX_DEPTH + 1], M[SNAIL_MAT_TRANSP_MAX_DEPTH + 1];   // chain A; chain B: ONE set of levels, reused by every k (the stream orders them)
	char *p = L[0].carveExtra(arena, (size_t)np);
	for(int k = 1; k <= D; k++) p = L[k].carve(p, (size_t)np, nLights);
	if(refl) for(int j = 0; j <= D; j++) p = M[j].carve(p, (size_t)np, nLights);
	const dim3 grid(np), wave(64), lgrid(np, nLights > 0 ? nLights : 1);
	// primary hits, with their barycentrics
	dev::InstArgs P = I;
	P.g = makeGen(cam, resx, resy);
	P.resx = resx; P.resy = resy;
	P.packetXY = (const int2 *)dXY; P.nPackets = np;
	P.t = W.hitT; P.u = W.hitU; P.v = W.hitV; P.instOut = W.hitInst; P.triOut = W.hitTri;
	P.stats = (dev::u64 *)dStats;
	P.pstats = pstats;   // (k_inst_frame books per packet whenever it is given the array)
	if(deep) SNAIL_INST_LAUNCH(sse, grid, st, P, k_inst_frame<true>);
	else SNAIL_INST_LAUNCH(sse, grid, st, P, k_inst_frame<false>);

	dev::ITranspArgs S;
	memset(&S, 0, sizeof(S));
	dev::IMatArgs &A = S.a;
	imatFillArgs(m, A, I, cam, resx, resy, dXY, np);
	A.m.s.nLights = nLights;
	for(int n = 0; n < nLights; n++) for(int k = 0; k < 7; k++) A.m.s.lights[n][k] = lights7[n * 7 + k];
	for(int c = 0; c < 3; c++) { A.m.s.ambient[c] = ambient[c]; A.m.s.color[c] = 1.0f; }
	A.m.s.hitT = W.hitT; A.m.s.hitId = W.hitTri; A.m.hitU = W.hitU; A.m.hitV = W.hitV; A.hitInst = W.hitInst;
	A.m.samples = W.samples; A.m.s.sDist = W.sDist;
	A.m.s.bgrPackets = bgrPackets; A.m.s.colPackets = colPackets;
	A.m.s.stats = (dev::u64 *)dStats;
	A.m.s.pstats = pstats;   // (T.m and G.t.m are copies of A.m: level() enters it again with everything else)
	A.m.rUVStride = 8;
	// the scene-free stages take a TranspArgs (materials_transparency.inc) or a TreeArgs (materials_tree.inc): its MatArgs is the frame's, entered
	// again whenever a level changes it
	dev::TreeArgs G;
	memset(&G, 0, sizeof(G));
	dev::TranspArgs &T = G.t;
	T.m = A.m;
	T.trunc = (unsigned long long *)dTrunc;
	// a level's generic packets as the stages' source, under its own order list (null: every packet); the object of the walk, of the generator and
	// of the mirror stage is the instance slot, the sample stages' rObj the triIds
	auto level = [&](const ITranspLevel &X, const int32_t *order, bool slotAsObject) {
		const SnailInstancesMaterials::BounceBufs &R = X.R;
		A.m.s.rOrg = R.rOrg; A.m.s.rDir = R.rDir; A.m.s.rIDir = R.rIDir; A.m.s.rMask = R.rMask; A.m.s.rDist = R.rDist; A.m.s.rCol = R.rCol;
		A.m.s.rObj = slotAsObject ? R.rInst : R.rTri;
		A.m.rU = R.bary; A.m.rV = R.bary + 4;
		A.m.nSamples = R.nSamples; A.m.nSDist = R.nSDist;
		S.rInst = R.rInst;
		S.inOrder = order;
		T.m = A.m;
		T.inOrder = order;
	};
	// (the stages enqueued so far are booked as every launch of the handle is, whatever failed)
	auto failed = [&](const char *what, hipError_t e) {
		(void)instancesEnd(h, st);
		snail_set_error("%s: %s: %s", fn, what, hipGetErrorString(e));
		return 100 + (int)e;
	};
	hipError_t me = hipSuccess;   // the first failed clear of the way back up
	// the ordered walk of a level's packets (order null: all of them, as the bounce walks its mirrored packets) and its sample stage
	auto walkSample = [&](const ITranspLevel &X, const int32_t *order) {
		if(me != hipSuccess) return;
		// the walk leaves element and barycentrics of a lane without a hit as it found them: zeros, not what the buffers last held (rTri and bary
		// are neighbours: ONE memset, as imatNested's)
		me = hipMemsetAsync(X.R.rTri, 0, (size_t)np * 256 * 12, st);
		if(me != hipSuccess) return;
		dev::ILevelArgs V;
		memset(&V, 0, sizeof(V));
		V.i = I;
		V.i.nPackets = np; V.i.size = 64;
		V.i.origin = X.R.rOrg; V.i.dir = X.R.rDir; V.i.idir = X.R.rIDir; V.i.mask = X.R.rMask;
		V.i.distance = X.R.rDist; V.i.object = X.R.rInst; V.i.element = X.R.rTri; V.i.bary = X.R.bary;
		V.i.stats = (dev::u64 *)dStats;
		V.i.pstats = pstats;
		V.order = order;
		SNAIL_ITREE_LAUNCH_PSTATS_DEEP(ILevelArgs, grid, V, k_imat_trace_level);
		level(X, order, false);
		S.opacity = X.opacity; S.sel = X.sel;
		SNAIL_ITRANSP_LAUNCH(sse, grid, st, S, k_imat_sample_transp_rays);
	};
	// the generator: from level `from` (its rays, hits, selector and own order list) into level `to`'s packets and order list; it zeroes the object
	// (here: the instance slot)
	auto generate = [&](const ITranspLevel &from, const int32_t *fromOrder, const ITranspLevel &to) {
		if(me != hipSuccess) return;
		level(to, fromOrder, true);
		T.order = to.order;
		T.cT = from.R.rDist; T.cSel = from.sel;
		T.cOrg = from.R.rOrg; T.cDir = from.R.rDir; T.cIDir = from.R.rIDir;
		SNAIL_ITREE_LAUNCH_PSTATS(TranspArgs, grid, T, k_mat_continue_rays);
	};
	// the lanes a level D would still select: counted, then treated as not selected
	auto truncated = [&](const ITranspLevel &X, const int32_t *order) {
		if(me != hipSuccess) return;
		level(X, order, false);
		T.bSel = X.sel;
		SNAIL_LAUNCH(sse, TranspArgs, grid, wave, 0, st, T, k_mat_truncated);
	};
	// a nested level's way back up: (the blend from the deeper level's colour,) its lights, its colour
	auto lightColour = [&](const ITranspLevel &X, const int32_t *order, const ITranspLevel *deeper) {
		if(me != hipSuccess) return;
		level(X, order, false);
		if(deeper && !pstats) {
			T.bSamples = X.R.nSamples; T.bOpacity = X.opacity; T.bSel = X.sel; T.bCol = deeper->R.rCol;
			SNAIL_LAUNCH(sse, TranspArgs, grid, wave, 0, st, T, k_mat_blend_transp);
		}
		if(nLights) SNAIL_ITREE_LAUNCH_PSTATS_DEEP(ITranspArgs, lgrid, S, k_imat_light_transp);
		if(!pstats) SNAIL_LAUNCH(sse, TranspArgs, grid, wave, 0, st, T, k_mat_colour_transp);
	};

	// ---- the way down of chain A: sample, then per level generator -> ordered walk -> nested sample ----
	S.opacity = L[0].opacity; S.sel = L[0].sel; S.inOrder = nullptr;
	SNAIL_ITRANSP_LAUNCH(sse, grid, st, S, k_imat_sample_transp);
	for(int k = 1; k <= D; k++) {
		if(k == 1) {
			level(L[1], nullptr, true);
			T.order = L[1].order;
			T.cT = W.hitT; T.cSel = L[0].sel;
			T.cOrg = T.cDir = T.cIDir = nullptr;
			SNAIL_ITREE_LAUNCH_PSTATS(TranspArgs, grid, T, k_mat_continue);
		} else generate(L[k - 1], L[k - 1].order, L[k]);
		walkSample(L[k], L[k].order);
	}
	truncated(L[D], L[D].order);

	// ---- the way back up ----
	for(int k = D; k >= 0 && me == hipSuccess; k--) {
		const int32_t *aOrder = k ? L[k].order : nullptr;
		if(refl) {
			// the B chain of A_k: the mirrored call B_{k,k} (every packet of A_k, hit or not) and its continuations down to level D
			const int32_t *bOrder = k ? M[k].order : nullptr;   // (k = 0: every packet, the bounce's walk)
			if(k) {
				level(L[k], aOrder, false);
				G.oOrg = M[k].R.rOrg; G.oDir = M[k].R.rDir; G.oIDir = M[k].R.rIDir; G.oDist = M[k].R.rDist; G.oObj = M[k].R.rInst; G.oMask = M[k].R.rMask;
				G.oOrder = M[k].order;
				SNAIL_ITREE_LAUNCH_PSTATS(TreeArgs, grid, G, k_mat_mirror_rays);
			} else {
				level(M[0], nullptr, true);
				SNAIL_ITREE_LAUNCH_PSTATS(MatArgs, grid, A.m, k_mat_mirror);
			}
			walkSample(M[k], bOrder);
			for(int j = k + 1; j <= D; j++) {
				generate(M[j - 1], j - 1 == k ? bOrder : M[j - 1].order, M[j]);
				walkSample(M[j], M[j].order);
			}
			truncated(M[D], D == k ? bOrder : M[D].order);
			for(int j = D; j >= k; j--) lightColour(M[j], j == k ? bOrder : M[j].order, j < D ? &M[j + 1] : nullptr);
			if(me != hipSuccess) break;
			// diffuse += (refl - diffuse) * 0.3 on A_k's hit lanes, before its transparency blend
			if(!pstats) {
				if(k) {
					level(L[k], aOrder, false);
					T.bSamples = L[k].R.nSamples; T.bCol = M[k].R.rCol;
					SNAIL_LAUNCH(sse, TranspArgs, grid, wave, 0, st, T, k_mat_blend_refl_rays);
				} else {
					T.m = A.m;
					T.inOrder = nullptr;
					T.bSamples = W.samples; T.bCol = M[0].R.rCol;
					SNAIL_LAUNCH(sse, TranspArgs, grid, wave, 0, st, T, k_mat_blend_refl);
				}
			}
		}
		if(k) lightColour(L[k], aOrder, k < D ? &L[k + 1] : nullptr);
	}
	if(me != hipSuccess) return failed("clearing a level's hit records failed", me);
	level(L[1], nullptr, false);   // (the primary stages read none of a level's packets; rCol must not be left on a B level's)
	T.bSamples = W.samples; T.bOpacity = L[0].opacity; T.bSel = L[0].sel; T.bCol = L[1].R.rCol;
	if(!pstats) SNAIL_LAUNCH(sse, TranspArgs, grid, wave, 0, st, T, k_mat_blend_transp);
	if(nLights) SNAIL_ITREE_LAUNCH_PSTATS_DEEP(IMatArgs, lgrid, A, k_imat_light);
	// both blends are in the sample buffer: the colour stage without one of its own, bytes or the floats k_inst_store goes on from
	if(!pstats) {   // (a heat launch: the counters alone)
		if(colPackets) SNAIL_LAUNCH(sse, MatArgs, grid, wave, 0, st, A.m, k_mat_colour);
		else SNAIL_LAUNCH(sse, MatArgs, grid, wave, 0, st, A.m, k_mat_final);
	}
	const hipError_t le = hipGetLastError();
	const int rc = instancesEnd(h, st);
	if(le != hipSuccess) { snail_set_error("%s: a stage's launch failed: %s", fn, hipGetErrorString(le)); return 100 + (int)le; }
	return rc;
}
#undef SNAIL_ITREE_LAUNCH_PSTATS
#undef SNAIL_ITREE_LAUNCH_PSTATS_DEEP

int64_t imatTreeLevelBytes(int nLights, int flags, int maxDepth) {
	if(flags & SNAIL_RENDER_DEPTH) return 0;
	return (int64_t)imatTreeBytes((flags & SNAIL_RENDER_AA4) ? 4 : 1, nLights, maxDepth, (flags & SNAIL_RENDER_REFLECTIONS) != 0);
}

// a part of a group of intermediates grown under imatNextSet's rule: its previous user may still be running
int imatGrow(SnailInstancesMaterials::Set &W, char *&part, size_t &have, size_t want, size_t bytes) {
	if(part && have >= want) return 0;
	HIP_TRY(hipDeviceSynchronize());
	if(part) (void)hipFree(part);
	part = nullptr; have = 0; W.used = false;
	HIP_TRY(hipMalloc((void **)&part, bytes));
	have = want;
	return 0;
}

#define SNAIL_ITREE_STORE(AA, PL) SNAIL_LAUNCH(sse, InstStoreArgs, dim3(np), dim3(64), 0, st, S, k_inst_store<false, AA, PL>)

// One run of the pipeline over the np packets of dXY with any flags and tint, into packet-major bytes (bgrPackets) or the planes of J's tiles;
// the handle's mu held.  The packet list runs in slices of whole output packets, back to back on st over the same intermediates, so that the
// levels stay within the set's budget (rounding makes the levels of n packets at most n times those of one); the float colours of ALL packets
// and the sub-packet list are kept, and ONE k_inst_store follows the last slice.
// heat (include/snail_instances_materials_heatmap.h; never with SNAIL_RENDER_DEPTH): the per-packet TreeStats instead of the colours -- cleared on st
// in dPacketStats or, when the caller keeps none, in the set's own array; every slice books at its packets' offset in the whole list's array; after
// the last slice the counters' colours: dev_heat::k_heat_store straight into bgrPackets, or with a tint or tile planes dev_heat::k_heat_colours
// into the set's float colours and the same ONE k_inst_store.  No output at all: the counters alone.
int imatTreeStore(SnailInstancesMaterials *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights,
				  const float ambient[3], int flags, const float *tint, uint8_t *bgrPackets, const InstTileJob *J, int maxDepth, uint64_t *dTrunc, uint64_t *dStats,
				  hipStream_t st, bool heat = false, uint32_t *dPacketStats = nullptr) {
	SnailInstances *h = m->inst;
	if(flags & SNAIL_RENDER_DEPTH) {   // gVals[1] returns before the full-shading branch: the hit distances of k_inst_frame alone, no level runs
		const float white[3] = {1.0f, 1.0f, 1.0f};
		return instancesShadeStore(h, fn, cam, resx, resy, dXY, np, nullptr, 0, ambient, white, flags & (SNAIL_RENDER_DEPTH | SNAIL_RENDER_AA4), tint, bgrPackets, J, dStats, st);
	}
	const bool aa = (flags & SNAIL_RENDER_AA4) != 0, refl = (flags & SNAIL_RENDER_REFLECTIONS) != 0;
	const bool floats = heat ? (tint || J) : (aa || tint || J);   // otherwise the lit packets as they are: bytes from k_mat_final (k_heat_store)
	const int q = aa ? 4 : 1;
	const int rx = aa ? resx * 2 : resx, ry = aa ? resy * 2 : resy;
	const uint64_t one = (uint64_t)imatTreeLevelBytes(nLights, flags, maxDepth);
	const uint64_t budget = std::max(m->levelBudget ? m->levelBudget : (uint64_t)SNAIL_MAT_LEVEL_BUDGET, one);
	const int slice = (int)std::min<uint64_t>(budget / one, (uint64_t)np);   // output packets per slice
	const size_t ns = (size_t)slice * q, n = (size_t)np * q;
	SnailInstancesMaterials::Set *Wp = nullptr;
	if(int rc = imatNextSet(m, (int)ns, nLights, false, st, &Wp)) return rc;
	SnailInstancesMaterials::Set &W = *Wp;
	if(floats || (heat && aa)) {   // the tile renderer's part for the WHOLE list (a heat launch without colours to reduce: for its sub-packet list alone)
		const size_t packets = std::max(W.tilesPackets, n);
		if(int rc = imatGrow(W, W.tiles, W.tilesPackets, packets, SnailMaterials::TileBufs::bytes(packets))) return rc;
	}
	{
		const size_t want = std::max(W.transpBytes, imatTreeBytes(ns, nLights, maxDepth, refl));
		if(int rc = imatGrow(W, W.transp, W.transpBytes, want, want)) return rc;
	}
	SnailInstancesMaterials::Bufs B;
	B.carve(W.base, ns);
	uint32_t *pst = nullptr;
	if(heat) {
		if(!dPacketStats) {
			const size_t packets = std::max(W.pstatsPackets, n);
			char *part = (char *)W.pstats;
			const int grc = imatGrow(W, part, W.pstatsPackets, packets, packets * 16);
			W.pstats = (uint32_t *)part;
			if(grc) return grc;
		}
		pst = dPacketStats ? dPacketStats : W.pstats;
	}
	SnailMaterials::TileBufs T;
	if(floats || (heat && aa)) T.carve(W.tiles, n);
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
		if(heat) rc = imatShadeTree(m, fn, cam, rx, ry, list + at * 2, cnt * q, lights7, nLights, ambient, nullptr, nullptr, B, W.transp, maxDepth, refl, dTrunc, dStats, st, pst + at * 4);
		else rc = imatShadeTree(m, fn, cam, rx, ry, list + at * 2, cnt * q, lights7, nLights, ambient, floats ? nullptr : bgrPackets + at * 768, floats ? T.col + at * 768 : nullptr, B,
								W.transp, maxDepth, refl, dTrunc, dStats, st);
	}
	if(!rc && heat && (floats || bgrPackets)) {   // no new colour arithmetic: the stores of heatmap.inc
		if(floats) hipLaunchKernelGGL(dev_heat::k_heat_colours, dim3((unsigned)n), dim3(64), 0, st, (const unsigned *)pst, (int)n, T.col);
		else if(aa) hipLaunchKernelGGL(dev_heat::k_heat_store<true>, dim3((unsigned)np), dim3(64), 0, st, (const unsigned *)pst, np, bgrPackets);
		else hipLaunchKernelGGL(dev_heat::k_heat_store<false>, dim3((unsigned)np), dim3(64), 0, st, (const unsigned *)pst, np, bgrPackets);
		const hipError_t e = hipGetLastError();
		if(e != hipSuccess) { snail_set_error("%s: the heat store: %s", fn, hipGetErrorString(e)); rc = 100 + (int)e; }
	}
	if(!rc && floats) {
		const bool sse = h->blas[0]->arith == SNAIL_ARITH_HOST_SSE;
		dev::InstStoreArgs S;
		memset(&S, 0, sizeof(S));
		S.hostTab = sse ? h->blas[0]->dTab : nullptr;
		S.in = T.col;
		S.nPackets = np;
		if(tint) { S.tinted = 1; for(int c = 0; c < 3; c++) S.tint[c] = tint[c]; }
		S.bgrPackets = bgrPackets;
		if(J) {
			S.tiles = (const int4 *)J->dTiles; S.packetTile = J->dPacketTile; S.firstPacket = J->dFirst; S.outOff = (const long long *)J->dOff;
			S.out = J->dOut; S.resx = resx; S.resy = resy;
		}
		switch((aa ? 2 : 0) | (J ? 1 : 0)) {
		case 0: SNAIL_ITREE_STORE(false, false); break;
		case 1: SNAIL_ITREE_STORE(false, true); break;
		case 2: SNAIL_ITREE_STORE(true, false); break;
		default: SNAIL_ITREE_STORE(true, true); break;
		}
		const hipError_t e = hipGetLastError();
		if(e != hipSuccess) { snail_set_error("%s: k_inst_store: %s", fn, hipGetErrorString(e)); rc = 100 + (int)e; }
	}
	return imatSetDone(W, fn, rc, st);
}
#undef SNAIL_ITREE_STORE

} // namespace

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
	return imatTreeStore(m, fn, cam, resx, resy, dPacketXY, nPackets, lights7, nLights, ambient, flags, tint, bgrPackets, nullptr, maxDepth, dTruncated, dStats, (hipStream_t)stream);
}

int snail_instances_materials_tree_render_tiles(SnailInstancesMaterials *m, const float cam[13], int resx, int resy, const int32_t *coords, const int64_t *offsets,
												int nTiles, const float *lights7, int nLights, const float ambient[3], int flags, const float *tint, uint8_t *data,
												int maxDepth, uint64_t *truncated, uint64_t stats[4]) {
	const char *fn = "snail_instances_materials_tree_render_tiles";
	if(int rc = matTreeArgsOk(fn, cam, resx, resy, lights7, nLights, ambient, flags, tint, maxDepth, truncated)) return rc;
	if(nTiles > 0 && (!coords || !offsets || !data)) { snail_set_error("%s: null buffer", fn); return 1; }
	for(int k = 0; k < nTiles; k++) {
		const long long x = coords[(size_t)k * 4 + 0], y = coords[(size_t)k * 4 + 1], w = coords[(size_t)k * 4 + 2], hh = coords[(size_t)k * 4 + 3];
		if(w <= 0 || hh <= 0 || x < 0 || y < 0 || x + w > (1 << 24) || y + hh > (1 << 24)) {
			snail_set_error("%s: tile %d: bad rect %lld,%lld %lldx%lld", fn, k, x, y, w, hh);
			return 1;
		}
	}
	if(int rc = checkIMatAny(m, fn)) return rc;
	if(nTiles <= 0) return 0;
	SnailInstances *h = m->inst;
	std::lock_guard<std::mutex> renderLock(m->renderMu);   // one cached tile job per set: its calls take turns
	DeviceGuard guard(m->device);
	HostCallScope hc(h->blas[0], fn);   // (a stream, counters and staging arena of the call's own; the BLAS handle only lends its free list)
	if(hc.rc) return hc.rc;
	if(!m->tileJob) m->tileJob = new InstTileJob();
	InstTileJob &J = *m->tileJob;
	if(int rc = buildInstTileJob(J, resx, resy, coords, nTiles)) return rc;
	if(stats) { if(int rc = hc.zeroStats()) return rc; }
	if(int rc = hc.reserve(HostCallScope::pad(8))) return rc;
	uint64_t *dTrunc = (uint64_t *)hc.carve(8);
	HIP_TRY(hipMemsetAsync(dTrunc, 0, 8, hc.stream()));
	{
		std::lock_guard<std::mutex> lock(h->mu);
		if(int rc = imatTreeStore(m, fn, cam, resx, resy, J.dXY, J.nPackets, lights7, nLights, ambient, flags, tint, nullptr, &J, maxDepth, dTrunc, stats ? hc.stats() : nullptr,
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

int snail_instances_materials_tree_render_frame(SnailInstancesMaterials *m, const float cam[13], int resx, int resy, const float *lights7, int nLights,
												const float ambient[3], int flags, uint8_t *image, int pitch, int maxDepth, uint64_t *truncated, uint64_t stats[4]) {
	const char *fn = "snail_instances_materials_tree_render_frame";
	if(int rc = matTreeArgsOk(fn, cam, resx, resy, lights7, nLights, ambient, flags, nullptr, maxDepth, truncated)) return rc;
	if(!image || pitch < resx * 3) { snail_set_error("%s: null image or a pitch below 3 * resx", fn); return 1; }
	if(int rc = checkIMatAny(m, fn)) return rc;
	SnailInstances *h = m->inst;
	DeviceGuard guard(m->device);
	HostCallScope hc(h->blas[0], fn);
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
		std::lock_guard<std::mutex> lock(h->mu);
		const int32_t *dXY = nullptr;
		int n = 0;
		if(int rc = imatFrameList(m, resx, resy, &dXY, &n)) return rc;
		if(int rc = imatTreeStore(m, fn, cam, resx, resy, dXY, np, lights7, nLights, ambient, flags, nullptr, bgr, nullptr, maxDepth, dTrunc, stats ? hc.stats() : nullptr, hc.stream()))
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
	return imatTreeLevelBytes(nLights, flags, maxDepth);
}

} // extern "C"
