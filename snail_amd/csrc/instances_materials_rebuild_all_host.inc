// instances_materials_rebuild_all_host.inc -- the C-ABI of include/snail_instances_materials_rebuild_all.h: the per-frame step of an animated
// instanced scene in ONE call under ONE set of locks -- snail_instances_materials_rebuild_dev (the listed BLASes' builds in one batched pass,
// bvh_fast_batch.inc, and their records' pack) followed by snail_instances_rebuild_dev (the top-level tree over the new root boxes).  Both
// halves are the two functions' own locked inner functions (imatDynRebuildLocked, instancesRebuildLocked); nothing is implemented again here.
// Lock order: the set's renderMu, the instances handle's mu, then the mu of EVERY BLAS scene of the handle that can be rebuilt on the device,
// in ascending BLAS index (the top-level build reads each one's root box, the listed ones' behind their commits).
#include "../../include/snail_instances_materials_rebuild_all.h"

extern "C" {

int snail_instances_materials_rebuild_all_dev(SnailInstancesMaterials *m, const SnailBlasRebuild *list, int nList, const float *d_xf12, const int32_t *d_blasIdx, int n,
											  int32_t *d_topPerm, int32_t *d_topInfo, void *stream) {
	const char *fn = "snail_instances_materials_rebuild_all_dev";
	// the union of both functions' refusals, all before anything is enqueued
	if(int rc = imatDynCheckRebuild(fn, m, list, nList)) return rc;
	SnailInstances *h = m->inst;
	if(int rc = instancesRebuildCheck(fn, h, d_xf12, n)) return rc;
	hipStream_t st = (hipStream_t)stream;
	DeviceGuard guard(m->device);
	std::lock_guard<std::mutex> renderLock(m->renderMu);
	std::lock_guard<std::mutex> lock(h->mu);               // no launch of the handle comes between the BLAS rebuilds and the top-level rebuild
	std::vector<int> fastBlas;
	for(size_t b = 0; b < h->blas.size(); b++)
		if(h->blas[b]->fast) fastBlas.push_back((int)b);
	std::vector<std::unique_lock<std::mutex>> locks;
	imatDynLock(h, fastBlas, locks);
	std::vector<SnailScene *> held;
	for(int b : fastBlas) held.push_back(h->blas[b]);
	// room for the top-level tree first: growing it waits for the device and may fail, and then no BLAS has been touched
	if(int rc = buildReserve(h, n)) return rc;
	if(int rc = imatDynRebuildLocked(m, list, nList, st)) return rc;
	// (the root boxes are read on st behind the commits: a BLAS whose build was refused contributes the box of the tree it keeps)
	return instancesRebuildLocked(h, d_xf12, d_blasIdx, n, d_topPerm, d_topInfo, st, &held);
}

} // extern "C"
