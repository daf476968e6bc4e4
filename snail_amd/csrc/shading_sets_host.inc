// shading_sets_host.inc -- what the handles that shade frames keep between launches, once for all of them; included by snail_hip.hip ahead of
// instances_host.inc.
//   frameGrid    the row-major packet list of a whole frame, on the host
//   FrameLists   ... cached on the device by packet-grid size (SnailInstances, SnailMaterials, SnailInstancesMaterials)
//   ShadeSets    the pool of intermediates of the two material handles: eight event-guarded sets handed out round-robin, one per launch in
//                flight, each of parts that are allocated once asked for and only grow (levelsGrow); with setsNext / setDone the place where the
//                handles' concurrency contract lives.  Booked under the handle's lock (the scene's mu, the instances handle's mu).

namespace {

struct InstTileJob; void freeInstTileJob(InstTileJob *);   // instances_tiles_host.inc: the cached lists of a tile renderer

// the packets of a pw x ph packet grid (16 x 16 pixels each), row-major: x, y of every packet's first pixel
std::vector<int32_t> frameGrid(int pw, int ph) {
	std::vector<int32_t> xy((size_t)pw * ph * 2);
	for(int y = 0; y < ph; y++)
		for(int x = 0; x < pw; x++) { xy[((size_t)y * pw + x) * 2] = x * 16; xy[((size_t)y * pw + x) * 2 + 1] = y * 16; }
	return xy;
}

// packet lists of whole frames on the device, by packet-grid size; built once each (the owner's lock held)
struct FrameLists {
	struct Entry { int pw, ph; int32_t *d; };
	std::vector<Entry> lists;
	int get(int resx, int resy, const int32_t **dXY, int *np) {
		const int pw = (resx + 15) / 16, ph = (resy + 15) / 16;
		*np = pw * ph;
		for(auto &f : lists)
			if(f.pw == pw && f.ph == ph) { *dXY = f.d; return 0; }
		if(lists.size() >= 16) {   // (a host that keeps changing its resolution: start over once nothing reads the old lists)
			HIP_TRY(hipDeviceSynchronize());
			release();
		}
		const std::vector<int32_t> xy = frameGrid(pw, ph);
		Entry f = {pw, ph, nullptr};
		HIP_TRY(hipMalloc((void **)&f.d, xy.size() * 4));
		if(hipMemcpy(f.d, xy.data(), xy.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(f.d); snail_set_error("frame packet list: upload failed"); return 1; }
		lists.push_back(f);
		*dXY = f.d;
		return 0;
	}
	void release() {
		for(auto &f : lists) (void)hipFree(f.d);
		lists.clear();
	}
};

// the base of SnailMaterials and SnailInstancesMaterials: the intermediates of the lit frames, one set per launch in flight
struct ShadeSets {
	struct Set {
		char *base = nullptr;         // the handle's Bufs: primary hits, samples, shadow distances
		size_t packets = 0;
		int lights = 0;
		char *bounce = nullptr;       // the handle's BounceBufs, only once a bounce has been asked for
		size_t bouncePackets = 0;
		int bounceLights = 0;
		char *tiles = nullptr;        // the tile renderer's part (TileBufs): the float colours of a whole packet list and, under 4x antialiasing, its sub-packet list
		size_t tilesPackets = 0;
		char *transp = nullptr;       // the levels of the transparency continuation (materials_levels_host.inc), sized by packets, lights and the depth asked for
		size_t transpBytes = 0;
		uint32_t *pstats = nullptr;   // a heat-map launch's per-packet TreeStats [packets][4] when the caller keeps none of its own
		size_t pstatsPackets = 0;
		hipEvent_t done = nullptr;
		bool used = false;
	};
	enum { kSets = 8 };
	Set set[kSets];
	unsigned setCount = 0;
	FrameLists frameLists;
	// the tile renderers: ONE cached tile job per handle (the structure of instances_tiles_host.inc); its calls take turns under renderMu, which is
	// taken before the handle's lock
	std::mutex renderMu;
	InstTileJob *tileJob = nullptr;
	// snail_materials_set_level_budget / snail_instances_materials_set_level_budget: the bytes the levels of one set may take; 0 = SNAIL_MAT_LEVEL_BUDGET
	uint64_t levelBudget = 0;
	// the destroyers, after the device has been waited for
	void release() {
		for(auto &W : set) {
			for(void *part : {(void *)W.base, (void *)W.bounce, (void *)W.tiles, (void *)W.transp, (void *)W.pstats})
				if(part) (void)hipFree(part);
			if(W.done) (void)hipEventDestroy(W.done);
		}
		freeInstTileJob(tileJob);
		frameLists.release();
	}
};

// A part of a set grown to `want` (and wantLights, for a part that is sized by both): nothing if it holds as much.  Its previous user may still be
// running, so the device is waited for before the free, and the set is as good as new: no event to wait for.  A failure leaves the part empty.
template <class Part>
int levelsGrow(ShadeSets::Set &W, Part *&part, size_t &have, size_t want, size_t bytes, int *haveLights = nullptr, int wantLights = 0) {
	if(part && have >= want && (!haveLights || *haveLights >= wantLights)) return 0;
	HIP_TRY(hipDeviceSynchronize());
	if(part) (void)hipFree(part);
	part = nullptr; have = 0; W.used = false;
	if(haveLights) *haveLights = 0;
	HIP_TRY(hipMalloc((void **)&part, bytes));
	have = want;
	if(haveLights) *haveLights = wantLights;
	return 0;
}

// The next set of the rotation for np packets and nLights lights (the handle's lock held), sized by the byte formulas of the handle H: base, with
// refl the bounce's part, with tiles the tile renderer's -- packets and lights each grown to max(have, want) -- and its previous user waited for on st.
template <class H>
int setsNext(H *m, int np, int nLights, bool refl, bool tiles, hipStream_t st, ShadeSets::Set **out) {
	ShadeSets::Set &W = m->set[m->setCount++ % ShadeSets::kSets];
	{
		const size_t packets = std::max(W.packets, (size_t)np);
		const int lights = std::max(W.lights, nLights);
		if(int rc = levelsGrow(W, W.base, W.packets, packets, H::Bufs::bytes(packets, lights), &W.lights, lights)) return rc;
	}
	if(refl) {
		const size_t packets = std::max(W.bouncePackets, (size_t)np);
		const int lights = std::max(W.bounceLights, nLights);
		if(int rc = levelsGrow(W, W.bounce, W.bouncePackets, packets, H::BounceBufs::bytes(packets, lights), &W.bounceLights, lights)) return rc;
	}
	if(tiles) {
		const size_t packets = std::max(W.tilesPackets, (size_t)np);
		if(int rc = levelsGrow(W, W.tiles, W.tilesPackets, packets, H::TileBufs::bytes(packets))) return rc;
	}
	if(!W.done) HIP_TRY(hipEventCreateWithFlags(&W.done, hipEventDisableTiming));
	if(W.used) HIP_TRY(hipStreamWaitEvent(st, W.done, 0));
	*out = &W;
	return 0;
}

// After the set's user has enqueued its stages on st (rc: how that went).  The event is recorded also when a stage failed after earlier ones were
// enqueued: they may still be running on these buffers, and the set's next user (on any stream) must come after them.  Should the record itself
// fail, every part counts as empty: the set's next user grows them all, which waits for the device.
int setDone(ShadeSets::Set &W, const char *fn, int rc, hipStream_t st) {
	if(hipEventRecord(W.done, st) == hipSuccess) W.used = true;
	else {
		W.packets = 0; W.bouncePackets = 0; W.tilesPackets = 0; W.transpBytes = 0; W.pstatsPackets = 0; W.used = false;
		if(!rc) { snail_set_error("%s: hipEventRecord failed", fn); return 1; }
	}
	return rc;
}

} // namespace
