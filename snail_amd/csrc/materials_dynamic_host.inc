// materials_dynamic_host.inc -- the C-ABI of include/snail_materials_dynamic.h: a material set over a handle of snail_scene_create_fast_dev
// whose ShTriangle records are packed on the device (materials_dynamic.inc) and packed again behind every rebuild, on the rebuild's stream.
// The host data goes through the creators' shared check and upload (matCheckHost / matUpload, materials_host.inc); the rebuild is
// snail_scene_rebuild_fast_dev's own (fastRebuildLocked, bvh_fast.inc) and so is the ordering: the pack's stream has waited for every launch
// enqueued on the handle (fastWaitUsers) and `ready` is recorded again behind the pack, so every later launch (SceneUse) waits for it.
#include "../../include/snail_materials_dynamic.h"

struct SnailMaterialsDyn {
	char *base = nullptr;              // ONE allocation: the input-order copies, the perm and the words below
	const float *dUV = nullptr;        // [n][3][2]
	const int *dMatIdx = nullptr;      // [n]
	const unsigned char *dFlat = nullptr;   // [n], or null: none flat
	int *dPerm = nullptr;              // the perm of the tree the records match: k_fast_commit writes it on status 0 only, k_shd_pack reads it
	int *dBuild = nullptr;             // k_fast_commit's {status, nNodes, depth, n}
	int *dZeroed = nullptr, *dCheck = nullptr;
	unsigned long long builtFor = 0;   // SnailSceneFast::rebuilds when the records were last packed (under the scene's mu)
};

namespace {

void dynFree(SnailMaterialsDyn *d) {
	if(!d) return;
	if(d->base) (void)hipFree(d->base);
	delete d;
}

int dynCheckFresh(const SnailMaterials *m, const char *fn) {
	SnailScene *s = m->scene;
	std::lock_guard<std::mutex> lock(s->mu);
	if(s->fast && m->dyn->builtFor == s->fast->rebuilds) return 0;
	snail_set_error("%s: the set's records are those of an earlier tree: the scene was rebuilt since (snail_scene_rebuild_fast_dev, or snail_materials_rebuild_dev "
					"of another set); snail_materials_update_dev with the current perm brings the set up to date", fn);
	return 1;
}

// a set of snail_materials_create_dev, stale or not
int checkMaterialsDyn(const SnailMaterials *m, const char *fn) {
	if(!m || !m->scene || !m->dBase) { snail_set_error("%s: invalid material set handle", fn); return 1; }
	if(!m->dyn || !m->scene->fast) { snail_set_error("%s: the set was not made by snail_materials_create_dev", fn); return 1; }
	return checkScene(m->scene, fn);
}

// the pack (+ the caller's info words) on st, and what makes every later launch wait for it; the scene's mu held, st has waited for the handle's users
int dynPack(SnailMaterials *m, const int *dPerm, const float *dNrm, const float *dVerts, const int *dBuild, int *dPermOut, int *dInfo, hipStream_t st) {
	SnailMaterialsDyn *d = m->dyn;
	SnailSceneFast *f = m->scene->fast;
	devshd::PackArgs A;
	memset((void *)&A, 0, sizeof(A));
	A.uv6 = d->dUV; A.matIdx = d->dMatIdx; A.flat = d->dFlat;
	A.nrm9 = dNrm; A.verts9 = dVerts;
	A.perm = dPerm; A.build = dBuild;
	A.shtris = const_cast<uint4 *>(m->dShTris);
	A.permOut = dPermOut; A.zeroed = d->dZeroed; A.check = d->dCheck; A.info = dInfo;
	A.n = m->nTris; A.nMap = m->nMap;
	HIP_TRY(hipMemsetAsync(d->dZeroed, 0, sizeof(int), st));
	hipLaunchKernelGGL(devshd::k_shd_pack, dim3((unsigned)((m->nTris + 255) / 256)), dim3(256), 0, st, A);
	if(dInfo) hipLaunchKernelGGL(devshd::k_shd_info, dim3(1), dim3(64), 0, st, A);
	HIP_TRY(hipGetLastError());
	if(!f->ready) HIP_TRY(hipEventCreateWithFlags(&f->ready, hipEventDisableTiming));
	HIP_TRY(hipEventRecord(f->ready, st));
	f->hasReady = true;
	d->builtFor = f->rebuilds;
	return 0;
}

} // namespace

extern "C" {

SnailMaterials *snail_materials_create_dev(SnailScene *scene, const float *d_uv6, const int32_t *d_matIdx, const uint8_t *d_flat, int nTris, const int32_t *d_perm,
										   const float *d_nrm9, const float *d_verts9, const int32_t *matMap, int nMap, const SnailMaterial *mats, int nMats,
										   const int32_t *opacityTexture, const SnailTexture *textures, int nTex, void *stream) {
	const char *fn = "snail_materials_create_dev";
	if(!d_uv6 || !d_matIdx || !d_perm || (!d_nrm9 && !d_verts9)) {
		snail_set_error("%s: null uv, material index or perm array, or neither normals nor vertices", fn);
		return nullptr;
	}
	bool canSelect = false;
	if(!matCheckHost(fn, opacityTexture != nullptr, true, nullptr, nTris, matMap, nMap, mats, nMats, opacityTexture, textures, nTex, &canSelect)) return nullptr;
	if(checkScene(scene, fn)) return nullptr;
	if(!scene->fast) { snail_set_error("%s: the scene was not made by snail_scene_create_fast_dev (snail_materials_create serves a tree that is never rebuilt)", fn); return nullptr; }
	if(nTris != scene->nTris) { snail_set_error("%s: %d triangles for a scene of %d triangles", fn, nTris, scene->nTris); return nullptr; }

	hipStream_t st = (hipStream_t)stream;
	DeviceGuard guard(scene->device);
	SnailMaterialsDyn *d = new SnailMaterialsDyn();
	typedef HostCallScope H;
	const size_t n = (size_t)nTris, oUV = 0, oMat = oUV + H::pad(n * 24), oFlat = oMat + H::pad(n * 4), oPerm = oFlat + H::pad(n), oWords = oPerm + H::pad(n * 4),
				 total = oWords + 256;
	hipError_t e = hipMalloc((void **)&d->base, total);
	if(e == hipSuccess) e = hipMemset(d->base, 0, total);
	if(e == hipSuccess) e = hipMemcpy(d->base + oUV, d_uv6, n * 24, hipMemcpyDeviceToDevice);
	if(e == hipSuccess) e = hipMemcpy(d->base + oMat, d_matIdx, n * 4, hipMemcpyDeviceToDevice);
	if(e == hipSuccess && d_flat) e = hipMemcpy(d->base + oFlat, d_flat, n, hipMemcpyDeviceToDevice);
	const int checkInit[2] = {0, 0x7fffffff};
	if(e == hipSuccess) e = hipMemcpy(d->base + oWords + 32, checkInit, sizeof(checkInit), hipMemcpyHostToDevice);
	if(e == hipSuccess) e = hipDeviceSynchronize();   // (device-to-device copies need not have run when hipMemcpy returns; st may not wait for the null stream)
	if(e != hipSuccess) { snail_set_error("%s: device copy failed: %s", fn, hipGetErrorString(e)); dynFree(d); return nullptr; }
	d->dUV = (const float *)(d->base + oUV); d->dMatIdx = (const int *)(d->base + oMat); d->dFlat = d_flat ? (const unsigned char *)(d->base + oFlat) : nullptr;
	d->dPerm = (int *)(d->base + oPerm);
	d->dBuild = (int *)(d->base + oWords); d->dZeroed = (int *)(d->base + oWords + 16); d->dCheck = (int *)(d->base + oWords + 32);

	// what snail_shtris_pack and the creators judge on the host, here on the device; before any record is written
	devshd::PackArgs C;
	memset((void *)&C, 0, sizeof(C));
	C.uv6 = d->dUV; C.matIdx = d->dMatIdx; C.perm = d_perm; C.check = d->dCheck; C.n = nTris; C.nMap = nMap;
	hipLaunchKernelGGL(devshd::k_shd_check, dim3((unsigned)((nTris + 255) / 256)), dim3(256), 0, st, C);
	int check[2] = {0, 0};
	if((e = hipGetLastError()) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess ||
	   (e = hipMemcpy(check, d->dCheck, sizeof(check), hipMemcpyDeviceToHost)) != hipSuccess) {
		snail_set_error("%s: %s", fn, hipGetErrorString(e));
		dynFree(d);
		return nullptr;
	}
	if(check[0]) {
		if(check[0] == 1) snail_set_error("%s: triangle %d: texture coordinate not finite or not below 2^20", fn, check[1]);
		else if(check[0] == 2) snail_set_error("%s: triangle %d: material index outside the map of %d entries", fn, check[1], nMap);
		else snail_set_error("%s: perm[%d] is outside 0..%d", fn, check[1], nTris - 1);
		dynFree(d);
		return nullptr;
	}
	SnailMaterials *m = matUpload(fn, canSelect, scene, nullptr, nTris, matMap, nMap, mats, nMats, opacityTexture, textures, nTex);
	if(!m) { dynFree(d); return nullptr; }
	m->dyn = d;
	int rc;
	{
		SNAIL_LOCK(scene);
		rc = fastWaitUsers(scene, st);
		if(!rc) rc = dynPack(m, d_perm, d_nrm9, d_verts9, nullptr, d->dPerm, nullptr, st);
	}
	if(!rc && (e = hipStreamSynchronize(st)) != hipSuccess) { snail_set_error("%s: %s", fn, hipGetErrorString(e)); rc = 1; }
	if(rc) { snail_materials_destroy(m); return nullptr; }
	return m;
}

int snail_materials_rebuild_dev(SnailMaterials *m, const float *d_verts9, const float *d_nrm9, int32_t *d_perm, int32_t *d_info, void *stream) {
	const char *fn = "snail_materials_rebuild_dev";
	if(int rc = checkMaterialsDyn(m, fn)) return rc;
	if(!d_verts9) { snail_set_error("%s: null vertices", fn); return 1; }
	// (a stale set is refused: should the build then fail, nothing would bring its records back to the tree the handle keeps)
	if(int rc = dynCheckFresh(m, fn)) return rc;
	hipStream_t st = (hipStream_t)stream;
	DeviceGuard guard(m->device);
	std::lock_guard<std::mutex> renderLock(m->renderMu);   // the set's tile job takes turns with this call
	SNAIL_LOCK(m->scene);
	SnailMaterialsDyn *d = m->dyn;
	// the build commits perm and tree together, into the SET's perm and status words: the pack behind it reads both on the stream
	if(int rc = fastRebuildLocked(m->scene, d_verts9, d->dPerm, d->dBuild, st)) return rc;
	return dynPack(m, d->dPerm, d_nrm9, d_verts9, d->dBuild, d_perm, d_info, st);
}

int snail_materials_update_dev(SnailMaterials *m, const int32_t *d_perm, const float *d_nrm9, const float *d_verts9, int32_t *d_info2, void *stream) {
	const char *fn = "snail_materials_update_dev";
	if(int rc = checkMaterialsDyn(m, fn)) return rc;
	if(!d_perm || (!d_nrm9 && !d_verts9)) { snail_set_error("%s: null perm, or neither normals nor vertices", fn); return 1; }
	hipStream_t st = (hipStream_t)stream;
	DeviceGuard guard(m->device);
	std::lock_guard<std::mutex> renderLock(m->renderMu);
	SNAIL_LOCK(m->scene);
	if(int rc = fastWaitUsers(m->scene, st)) return rc;
	return dynPack(m, d_perm, d_nrm9, d_verts9, nullptr, m->dyn->dPerm, d_info2, st);
}

#ifdef SNAIL_DEBUG_API
// The workbench build only, for the tests: the records any set holds now, nTris x 64 bytes into host memory (waits for the device).
int snail_materials_debug_records(SnailMaterials *m, void *out64, int nTris) {
	const char *fn = "snail_materials_debug_records";
	if(!m || !m->dBase || !out64 || nTris != m->nTris) { snail_set_error("%s: invalid set, null buffer or another triangle count", fn); return 1; }
	DeviceGuard guard(m->device);
	HIP_TRY(hipDeviceSynchronize());
	HIP_TRY(hipMemcpy(out64, m->dShTris, (size_t)nTris * 64, hipMemcpyDeviceToHost));
	return 0;
}
#endif

} // extern "C"
