// instances_materials_dynamic_host.inc -- the C-ABI of include/snail_instances_materials_dynamic.h: the material set of an instanced scene in
// which the records of every BLAS of snail_scene_create_fast_dev are packed on the device and packed again behind every rebuild of that BLAS,
// all listed BLASes in ONE launch (instances_materials_dynamic.inc).  Per BLAS it is materials_dynamic_host.inc's scheme: the rebuild is
// snail_scenes_rebuild_fast_dev's own (fastRebuildBatchLocked: the listed BLASes' builds in one batched pass), the pack's stream has waited for every user of the BLAS scene (fastWaitUsers;
// instanced launches book their use in instancesEnd) and the scene's `ready` is recorded again behind the pack, so every later instanced launch
// waits for it in instancesBegin.  Lock order: the set's renderMu, the instances handle's mu, the BLAS scenes' mu in ascending BLAS index.
#include "../../include/snail_instances_materials_dynamic.h"

struct SnailInstancesMaterialsDyn {
	char *base = nullptr;                  // ONE allocation: every dynamic BLAS's input-order copies and perm, then the words below
	struct Blas {
		bool dynamic = false;              // (false: built from host triangles, the records are the creator's)
		const float *dUV = nullptr;        // [n][3][2]
		const int *dMatIdx = nullptr;      // [n]
		const unsigned char *dFlat = nullptr;   // [n], or null: none flat
		int *dPerm = nullptr;              // the perm of the tree the records match: k_fast_commit writes it on status 0 only, the pack reads it
		int *dBuild = nullptr;             // k_fast_commit's {status, nNodes, depth, n}
		int *dZeroed = nullptr;            // 0 between calls: k_ishd_info reads it and sets it back
		unsigned long long builtFor = 0;   // SnailSceneFast::rebuilds when the records were last packed (under that scene's mu)
	};
	std::vector<Blas> blas;                // one per BLAS of the handle
	int *dCheck = nullptr;                 // k_shd_check's {code, first offender}, creation only
};

namespace {

void imatDynFree(SnailInstancesMaterialsDyn *d) {
	if(!d) return;
	if(d->base) (void)hipFree(d->base);
	delete d;
}

int imatDynCheckFresh(const SnailInstancesMaterials *m, const char *fn) {
	const SnailInstancesMaterialsDyn *d = m->dyn;
	for(size_t b = 0; b < d->blas.size(); b++) {
		if(!d->blas[b].dynamic) continue;
		SnailScene *s = m->inst->blas[b];
		std::lock_guard<std::mutex> lock(s->mu);
		if(s->fast && d->blas[b].builtFor == s->fast->rebuilds) continue;
		snail_set_error("%s: the set's records of BLAS %d are those of an earlier tree: that BLAS scene was rebuilt since (snail_scene_rebuild_fast_dev, "
						"snail_materials_rebuild_dev, or snail_instances_materials_rebuild_dev of another set); snail_instances_materials_update_dev with "
						"the current perm brings the set up to date", fn, (int)b);
		return 1;
	}
	return 0;
}

// a set of snail_instances_materials_create_dev, stale or not
int checkIMatDyn(const SnailInstancesMaterials *m, const char *fn) {
	if(!m || !m->inst || !m->dBase) { snail_set_error("%s: invalid instanced material set handle", fn); return 1; }
	if(!m->dyn) { snail_set_error("%s: the set was not made by snail_instances_materials_create_dev", fn); return 1; }
	return checkInstances(m->inst, fn);
}

// the BLAS scenes' mu in ascending BLAS index (idx sorted), a scene that stands under two indices once
void imatDynLock(SnailInstances *h, const std::vector<int> &idx, std::vector<std::unique_lock<std::mutex>> &locks) {
	std::vector<SnailScene *> held;
	for(int b : idx) {
		SnailScene *s = h->blas[b];
		if(std::find(held.begin(), held.end(), s) != held.end()) continue;
		held.push_back(s);
		locks.emplace_back(s->mu);
	}
}

// the part of an entry that the set knows; perm, build, permOut, info and the normals are the call's
devshd::PackArgs imatDynEntry(const SnailInstancesMaterials *m, int b) {
	const SnailInstancesMaterialsDyn::Blas &D = m->dyn->blas[b];
	devshd::PackArgs A;
	memset((void *)&A, 0, sizeof(A));
	A.uv6 = D.dUV; A.matIdx = D.dMatIdx; A.flat = D.dFlat;
	A.shtris = const_cast<uint4 *>(m->hTab[b].shtris);
	A.zeroed = D.dZeroed; A.check = m->dyn->dCheck;
	A.n = m->hTab[b].nTris; A.nMap = m->hTab[b].nMap;
	return A;
}

// the batched pack of E (entry k belongs to BLAS idx[k]) and the info words on st, and what makes every later launch wait for it; the handle's and
// the listed scenes' mu held, st has waited for the scenes' users
int imatDynPack(SnailInstancesMaterials *m, const std::vector<int> &idx, const std::vector<devshd::PackArgs> &E, hipStream_t st) {
	for(size_t at = 0; at < E.size(); at += devshd::kIshdMax) {
		devshd::IPackArgs T;
		memset((void *)&T, 0, sizeof(T));
		T.count = (int)std::min(E.size() - at, (size_t)devshd::kIshdMax);
		for(int k = 0; k < T.count; k++) {
			T.e[k] = E[at + k];
			T.first[k + 1] = T.first[k] + (T.e[k].n + 255) / 256;
		}
		for(int k = T.count + 1; k <= devshd::kIshdMax; k++) T.first[k] = T.first[T.count];
		hipLaunchKernelGGL(devshd::k_ishd_pack, dim3((unsigned)T.first[T.count]), dim3(256), 0, st, T);
		hipLaunchKernelGGL(devshd::k_ishd_info, dim3((unsigned)T.count), dim3(64), 0, st, T);   // (always: it sets the counters back to 0)
	}
	HIP_TRY(hipGetLastError());
	for(int b : idx) {
		SnailSceneFast *f = m->inst->blas[b]->fast;
		if(!f->ready) HIP_TRY(hipEventCreateWithFlags(&f->ready, hipEventDisableTiming));
		HIP_TRY(hipEventRecord(f->ready, st));
		f->hasReady = true;
		m->dyn->blas[b].builtFor = f->rebuilds;
	}
	return 0;
}

// what both calls refuse about their list; the part that needs no set comes first (set == null: that part alone)
int imatDynCheckList(const char *fn, const SnailInstancesMaterials *m, const SnailBlasRebuild *list, int nList, bool rebuild) {
	if(!m) {
		if(!list || nList <= 0) { snail_set_error("%s: no BLAS listed (a null list or nList <= 0)", fn); return 1; }
		for(int k = 0; k < nList; k++) {
			if(list[k].blas < 0) { snail_set_error("%s: entry %d: BLAS index %d is out of range", fn, k, list[k].blas); return 1; }
			for(int j = 0; j < k; j++)
				if(list[j].blas == list[k].blas) { snail_set_error("%s: entry %d: BLAS %d is listed twice (entry %d)", fn, k, list[k].blas, j); return 1; }
			if(rebuild && !list[k].d_verts9) { snail_set_error("%s: entry %d (BLAS %d): null vertices", fn, k, list[k].blas); return 1; }
			if(!rebuild && (!list[k].d_perm || (!list[k].d_nrm9 && !list[k].d_verts9))) {
				snail_set_error("%s: entry %d (BLAS %d): null perm, or neither normals nor vertices", fn, k, list[k].blas);
				return 1;
			}
		}
		return 0;
	}
	for(int k = 0; k < nList; k++) {
		const int b = list[k].blas;
		if(b >= m->nBlas) { snail_set_error("%s: entry %d: BLAS index %d is out of range (the handle has %d)", fn, k, b, m->nBlas); return 1; }
		if(!m->dyn->blas[b].dynamic) {
			snail_set_error("%s: entry %d: BLAS %d is never rebuilt (it was built from host triangles): its records are the creator's", fn, k, b);
			return 1;
		}
		for(int j = 0; j < k; j++)
			if(m->inst->blas[list[j].blas] == m->inst->blas[b]) { snail_set_error("%s: entries %d and %d name one BLAS scene (BLAS %d and %d)", fn, j, k, list[j].blas, b); return 1; }
	}
	return 0;
}

// everything snail_instances_materials_rebuild_dev refuses, before anything is enqueued (fn: the caller's name in the texts)
int imatDynCheckRebuild(const char *fn, const SnailInstancesMaterials *m, const SnailBlasRebuild *list, int nList) {
	if(int rc = imatDynCheckList(fn, nullptr, list, nList, true)) return rc;
	if(int rc = checkIMatDyn(m, fn)) return rc;
	if(int rc = imatDynCheckList(fn, m, list, nList, true)) return rc;
	// (a stale set is refused: should a build then fail, nothing would bring that BLAS's records back to the tree it keeps)
	return imatDynCheckFresh(m, fn);
}

// snail_instances_materials_rebuild_dev after its arguments were judged; the set's renderMu, the handle's mu and the listed scenes' mu held.
// The builds of all listed BLASes are ONE batched pass (bvh_fast_batch.inc), the pack of all of them one launch behind it
int imatDynRebuildLocked(SnailInstancesMaterials *m, const SnailBlasRebuild *list, int nList, hipStream_t st) {
	SnailInstances *h = m->inst;
	std::vector<int> idx;
	std::vector<devshd::PackArgs> E;
	std::vector<FastBatchItem> builds;
	for(int k = 0; k < nList; k++) {
		const int b = list[k].blas;
		SnailInstancesMaterialsDyn::Blas &D = m->dyn->blas[b];
		// the build commits perm and tree together, into the SET's perm and status words of this BLAS: the pack behind it reads both on the stream
		builds.push_back(FastBatchItem{h->blas[b], list[k].d_verts9, D.dPerm, D.dBuild});
		devshd::PackArgs A = imatDynEntry(m, b);
		A.perm = D.dPerm; A.build = D.dBuild; A.permOut = list[k].d_perm; A.info = list[k].d_info;
		A.nrm9 = list[k].d_nrm9; A.verts9 = list[k].d_verts9;
		idx.push_back(b);
		E.push_back(A);
	}
	if(int rc = fastRebuildBatchLocked(builds.data(), nList, st)) return rc;
	return imatDynPack(m, idx, E, st);
}

std::vector<int> imatDynSorted(const SnailBlasRebuild *list, int nList) {
	std::vector<int> idx((size_t)nList);
	for(int k = 0; k < nList; k++) idx[k] = list[k].blas;
	std::sort(idx.begin(), idx.end());
	return idx;
}

} // namespace

extern "C" {

SnailInstancesMaterials *snail_instances_materials_create_dev(SnailInstances *h, const SnailBlasShadingDev *perBlas, int nBlas, const SnailMaterial *mats, int nMats,
															  const int32_t *opacityTexture, const SnailTexture *textures, int nTex, void *stream) {
	const char *fn = "snail_instances_materials_create_dev";
	const bool transp = opacityTexture != nullptr;
	// the caller's HOST data first (imatCreate's order), a dynamic BLAS by the dynamic creator's rules
	if(!perBlas || nBlas <= 0) { snail_set_error("%s: no per-BLAS shading data", fn); return nullptr; }
	bool canSelectAny = false;
	std::vector<char> isDev((size_t)nBlas);
	for(int b = 0; b < nBlas; b++) {
		const SnailBlasShadingDev &P = perBlas[b];
		isDev[b] = P.shtris64 == nullptr;
		if(isDev[b] && (!P.d_uv6 || !P.d_matIdx || !P.d_perm || (!P.d_nrm9 && !P.d_verts9))) {
			snail_set_error("%s: BLAS %d: no host records, and a null uv, material index or perm array, or neither normals nor vertices", fn, b);
			return nullptr;
		}
		if(!isDev[b] && (P.d_uv6 || P.d_matIdx || P.d_flat || P.d_perm || P.d_nrm9 || P.d_verts9)) {
			snail_set_error("%s: BLAS %d: host records AND device data (a BLAS has one or the other)", fn, b);
			return nullptr;
		}
		bool canSelect = false;
		if(!matCheckHost(fn, transp, isDev[b] != 0, P.shtris64, P.nTris, P.matMap, P.nMap, mats, nMats, opacityTexture, textures, nTex, &canSelect)) {
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
		if(h->blas[b]->fast && !isDev[b]) {
			snail_set_error("%s: BLAS %d is rebuilt on the device, which renumbers its triangles, and was given host records: give its input-order data in device memory", fn, b);
			return nullptr;
		}
		if(!h->blas[b]->fast && isDev[b]) {
			snail_set_error("%s: BLAS %d was not made by snail_scene_create_fast_dev and was given device data: a tree that is never rebuilt takes host records", fn, b);
			return nullptr;
		}
		if(perBlas[b].nTris != h->blas[b]->nTris) { snail_set_error("%s: BLAS %d: %d records (nTris) for a scene of %d triangles", fn, b, perBlas[b].nTris, h->blas[b]->nTris); return nullptr; }
	}

	// the set's copies of the input-order data
	hipStream_t st = (hipStream_t)stream;
	DeviceGuard guard(h->device);
	SnailInstancesMaterialsDyn *d = new SnailInstancesMaterialsDyn();
	d->blas.resize((size_t)nBlas);
	typedef HostCallScope H;
	std::vector<size_t> oUV((size_t)nBlas), oMat((size_t)nBlas), oFlat((size_t)nBlas), oPerm((size_t)nBlas);
	size_t total = 0;
	for(int b = 0; b < nBlas; b++) {
		if(!isDev[b]) continue;
		const size_t n = (size_t)perBlas[b].nTris;
		oUV[b] = total; total += H::pad(n * 24);
		oMat[b] = total; total += H::pad(n * 4);
		oFlat[b] = total; total += H::pad(n);
		oPerm[b] = total; total += H::pad(n * 4);
	}
	const size_t oBuild = total, oZeroed = oBuild + H::pad((size_t)nBlas * 16), oCheck = oZeroed + H::pad((size_t)nBlas * 4);
	total = oCheck + 256;
	hipError_t e = hipMalloc((void **)&d->base, total);
	if(e == hipSuccess) e = hipMemset(d->base, 0, total);
	for(int b = 0; b < nBlas && e == hipSuccess; b++) {
		if(!isDev[b]) continue;
		const SnailBlasShadingDev &P = perBlas[b];
		const size_t n = (size_t)P.nTris;
		e = hipMemcpy(d->base + oUV[b], P.d_uv6, n * 24, hipMemcpyDeviceToDevice);
		if(e == hipSuccess) e = hipMemcpy(d->base + oMat[b], P.d_matIdx, n * 4, hipMemcpyDeviceToDevice);
		if(e == hipSuccess && P.d_flat) e = hipMemcpy(d->base + oFlat[b], P.d_flat, n, hipMemcpyDeviceToDevice);
		SnailInstancesMaterialsDyn::Blas &D = d->blas[b];
		D.dynamic = true;
		D.dUV = (const float *)(d->base + oUV[b]); D.dMatIdx = (const int *)(d->base + oMat[b]);
		D.dFlat = P.d_flat ? (const unsigned char *)(d->base + oFlat[b]) : nullptr;
		D.dPerm = (int *)(d->base + oPerm[b]);
		D.dBuild = (int *)(d->base + oBuild + (size_t)b * 16); D.dZeroed = (int *)(d->base + oZeroed + (size_t)b * 4);
	}
	d->dCheck = (int *)(d->base + oCheck);
	if(e == hipSuccess) e = hipDeviceSynchronize();   // (device-to-device copies need not have run when hipMemcpy returns; st may not wait for the null stream)
	if(e != hipSuccess) { snail_set_error("%s: device copy failed: %s", fn, hipGetErrorString(e)); imatDynFree(d); return nullptr; }

	// what snail_shtris_pack and the creators judge on the host, here on the device, BLAS by BLAS; before any record is written
	for(int b = 0; b < nBlas; b++) {
		if(!isDev[b]) continue;
		const int checkInit[2] = {0, 0x7fffffff};
		int check[2] = {0, 0};
		devshd::PackArgs C;
		memset((void *)&C, 0, sizeof(C));
		C.uv6 = d->blas[b].dUV; C.matIdx = d->blas[b].dMatIdx; C.perm = perBlas[b].d_perm; C.check = d->dCheck; C.n = perBlas[b].nTris; C.nMap = perBlas[b].nMap;
		if((e = hipMemcpy(d->dCheck, checkInit, sizeof(checkInit), hipMemcpyHostToDevice)) == hipSuccess && (e = hipDeviceSynchronize()) == hipSuccess) {
			hipLaunchKernelGGL(devshd::k_shd_check, dim3((unsigned)((C.n + 255) / 256)), dim3(256), 0, st, C);
			if((e = hipGetLastError()) == hipSuccess && (e = hipStreamSynchronize(st)) == hipSuccess) e = hipMemcpy(check, d->dCheck, sizeof(check), hipMemcpyDeviceToHost);
		}
		if(e != hipSuccess) { snail_set_error("%s: %s", fn, hipGetErrorString(e)); imatDynFree(d); return nullptr; }
		if(check[0]) {
			if(check[0] == 1) snail_set_error("%s: BLAS %d: triangle %d: texture coordinate not finite or not below 2^20", fn, b, check[1]);
			else if(check[0] == 2) snail_set_error("%s: BLAS %d: triangle %d: material index outside the map of %d entries", fn, b, check[1], perBlas[b].nMap);
			else snail_set_error("%s: BLAS %d: perm[%d] is outside 0..%d", fn, b, check[1], perBlas[b].nTris - 1);
			imatDynFree(d);
			return nullptr;
		}
	}

	std::vector<SnailBlasShading> per((size_t)nBlas);
	for(int b = 0; b < nBlas; b++) { per[b].shtris64 = perBlas[b].shtris64; per[b].nTris = perBlas[b].nTris; per[b].matMap = perBlas[b].matMap; per[b].nMap = perBlas[b].nMap; }
	SnailInstancesMaterials *m = imatUpload(fn, canSelectAny, h, per.data(), nBlas, mats, nMats, opacityTexture, textures, nTex);
	if(!m) { imatDynFree(d); return nullptr; }
	m->dyn = d;
	int rc = 0;
	if((e = hipDeviceSynchronize()) != hipSuccess) { snail_set_error("%s: %s", fn, hipGetErrorString(e)); rc = 1; }   // (the set's zeroed records, as above)
	std::vector<int> idx;
	std::vector<devshd::PackArgs> E;
	for(int b = 0; b < nBlas; b++) {
		if(!isDev[b]) continue;
		devshd::PackArgs A = imatDynEntry(m, b);
		A.perm = perBlas[b].d_perm; A.permOut = d->blas[b].dPerm;
		A.nrm9 = perBlas[b].d_nrm9; A.verts9 = perBlas[b].d_verts9;
		idx.push_back(b);
		E.push_back(A);
	}
	if(!rc && !E.empty()) {
		std::lock_guard<std::mutex> lock(h->mu);
		std::vector<std::unique_lock<std::mutex>> locks;
		imatDynLock(h, idx, locks);
		for(size_t k = 0; k < idx.size() && !rc; k++) rc = fastWaitUsers(h->blas[idx[k]], st);
		if(!rc) rc = imatDynPack(m, idx, E, st);
	}
	if(!rc && (e = hipStreamSynchronize(st)) != hipSuccess) { snail_set_error("%s: %s", fn, hipGetErrorString(e)); rc = 1; }
	if(rc) { snail_instances_materials_destroy(m); return nullptr; }
	return m;
}

int snail_instances_materials_rebuild_dev(SnailInstancesMaterials *m, const SnailBlasRebuild *list, int nList, void *stream) {
	const char *fn = "snail_instances_materials_rebuild_dev";
	if(int rc = imatDynCheckRebuild(fn, m, list, nList)) return rc;
	SnailInstances *h = m->inst;
	DeviceGuard guard(m->device);
	std::lock_guard<std::mutex> renderLock(m->renderMu);   // the set's tile job takes turns with this call
	std::lock_guard<std::mutex> lock(h->mu);               // no launch of the handle comes between a BLAS's build and its pack
	const std::vector<int> sorted = imatDynSorted(list, nList);
	std::vector<std::unique_lock<std::mutex>> locks;
	imatDynLock(h, sorted, locks);
	return imatDynRebuildLocked(m, list, nList, (hipStream_t)stream);
}

int snail_instances_materials_update_dev(SnailInstancesMaterials *m, const SnailBlasRebuild *list, int nList, void *stream) {
	const char *fn = "snail_instances_materials_update_dev";
	if(int rc = imatDynCheckList(fn, nullptr, list, nList, false)) return rc;
	if(int rc = checkIMatDyn(m, fn)) return rc;
	if(int rc = imatDynCheckList(fn, m, list, nList, false)) return rc;
	SnailInstances *h = m->inst;
	hipStream_t st = (hipStream_t)stream;
	DeviceGuard guard(m->device);
	std::lock_guard<std::mutex> renderLock(m->renderMu);
	std::lock_guard<std::mutex> lock(h->mu);
	const std::vector<int> sorted = imatDynSorted(list, nList);
	std::vector<std::unique_lock<std::mutex>> locks;
	imatDynLock(h, sorted, locks);
	std::vector<int> idx;
	std::vector<devshd::PackArgs> E;
	for(int k = 0; k < nList; k++) {
		const int b = list[k].blas;
		if(int rc = fastWaitUsers(h->blas[b], st)) return rc;
		devshd::PackArgs A = imatDynEntry(m, b);
		A.perm = list[k].d_perm; A.permOut = m->dyn->blas[b].dPerm; A.info = list[k].d_info;
		A.nrm9 = list[k].d_nrm9; A.verts9 = list[k].d_verts9;
		idx.push_back(b);
		E.push_back(A);
	}
	return imatDynPack(m, idx, E, st);
}

#ifdef SNAIL_DEBUG_API
// The workbench build only, for the tests: the records the set holds now for one BLAS, nTris x 64 bytes into host memory (waits for the device).
int snail_instances_materials_debug_records(SnailInstancesMaterials *m, int blas, void *out64, int nTris) {
	const char *fn = "snail_instances_materials_debug_records";
	if(!m || !m->dBase || !out64 || blas < 0 || blas >= m->nBlas || nTris != m->hTab[blas].nTris) {
		snail_set_error("%s: invalid set, BLAS index out of range, null buffer or another triangle count", fn);
		return 1;
	}
	DeviceGuard guard(m->device);
	HIP_TRY(hipDeviceSynchronize());
	HIP_TRY(hipMemcpy(out64, m->hTab[blas].shtris, (size_t)nTris * 64, hipMemcpyDeviceToHost));
	return 0;
}
#endif

} // extern "C"
