// instances_materials_bounce_host.inc -- the C-ABI of include/snail_instances_materials_bounce.h: the frames of instances_materials_host.inc with
// the one mirrored bounce of gVals[7] (k_inst_frame with barycentrics -> k_imat_sample -> k_mat_mirror -> k_inst_trace<false, true, DEEP, true> ->
// k_imat_sample_rays -> k_imat_light_rays -> k_mat_colour_rays -> k_imat_light -> k_mat_final_blend), and its two stages on their own.  Included
// after instances_materials_host.inc, whose set, argument record and frame driver (imatShade, which calls imatNested below) it uses.
#include "../../include/snail_instances_materials_bounce.h"

namespace {

#define SNAIL_IMAT_RAYS_LAUNCH(SSE, GRID, STREAM, A, ...) SNAIL_LAUNCH(SSE, IMatRaysArgs, GRID, dim3(64), 0, STREAM, A, __VA_ARGS__)

// include/snail_instances_materials_bounce.h: flags = 0 or SNAIL_RENDER_REFLECTIONS, judged before anything else
int checkIMatBounceFrameArgs(const char *fn, const float cam[13], int resx, int resy, const float *lights7, int nLights, const float ambient[3], int flags) {
	if(flags & ~SNAIL_RENDER_REFLECTIONS) {
		snail_set_error("%s: flags must be 0 or SNAIL_RENDER_REFLECTIONS (got 0x%x): no depth shading, transparency or antialiasing under full shading of instanced scenes", fn, flags);
		return 1;
	}
	return checkMatFrameArgs(fn, cam, resx, resy, lights7, nLights, ambient, 0);
}

// the nested RayTrace of the mirrored packets, between imatShade's sample stage and its primary lights (the handle's mu held; A: the frame's argument
// record, the primary samples written; I from instancesBegin).  Enters R into A for the stages that follow: k_mat_final_blend reads rCol.
int imatNested(SnailInstances *h, const char *fn, dev::IMatArgs &A, const dev::InstArgs &I, bool sse, bool deep, const SnailInstancesMaterials::BounceBufs &R,
			   hipStream_t st) {
	const int np = A.m.s.nPackets, nLights = A.m.s.nLights;
	const dim3 grid(np);
	A.m.s.rOrg = R.rOrg; A.m.s.rDir = R.rDir; A.m.s.rIDir = R.rIDir; A.m.s.rMask = R.rMask; A.m.s.rDist = R.rDist; A.m.s.rCol = R.rCol;
	A.m.rU = R.bary; A.m.rV = R.bary + 4; A.m.rUVStride = 8;
	A.m.nSamples = R.nSamples; A.m.nSDist = R.nSDist;
	A.m.s.blend = 1;
	// the mirrored packets: k_mat_mirror zeroes the object (here: the instance slot); the walk leaves element and barycentrics of a lane without a
	// hit as it found them: zeros, not what the buffers last held
	A.m.s.rObj = R.rInst;
	SNAIL_LAUNCH(sse, MatArgs, grid, dim3(64), 0, st, A.m, k_mat_mirror);
	A.m.s.rObj = R.rTri;   // from here on the triIds, as k_imat_sample_rays reads them
	const hipError_t e = hipMemsetAsync(R.rTri, 0, (size_t)np * 256 * 12, st);
	if(e != hipSuccess) {   // (the stages enqueued so far are booked as every launch of the handle is)
		(void)instancesEnd(h, st);
		snail_set_error("%s: clearing the mirrored packets' hit records failed: %s", fn, hipGetErrorString(e));
		return 100 + (int)e;
	}
	dev::InstArgs T = I;
	T.nPackets = np; T.size = 64;
	T.origin = R.rOrg; T.dir = R.rDir; T.idir = R.rIDir; T.mask = R.rMask;
	T.distance = R.rDist; T.object = R.rInst; T.element = R.rTri; T.bary = R.bary;
	T.stats = A.m.s.stats;
	if(deep) SNAIL_INST_LAUNCH(sse, grid, st, T, k_inst_trace<false, true, true, true>);
	else SNAIL_INST_LAUNCH(sse, grid, st, T, k_inst_trace<false, true, false, true>);
	dev::IMatRaysArgs B;
	B.a = A; B.rInst = R.rInst;
	SNAIL_IMAT_RAYS_LAUNCH(sse, grid, st, B, k_imat_sample_rays);
	if(nLights) {
		const dim3 lgrid(np, nLights);
		if(deep) SNAIL_IMAT_LAUNCH(sse, lgrid, st, A, k_imat_light_rays<true>);
		else SNAIL_IMAT_LAUNCH(sse, lgrid, st, A, k_imat_light_rays<false>);
	}
	SNAIL_LAUNCH(sse, MatArgs, grid, dim3(64), 0, st, A.m, k_mat_colour_rays);   // (nested samples, hits and surviving distances: the plain scenes' stage as it is)
	return 0;
}

} // namespace

extern "C" {

int snail_instances_materials_mirror_packets_dev(SnailInstancesMaterials *m, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets,
												 const float *dT, const float *dSamples, float *dOrigin, float *dDir, float *dIDir, uint8_t *dMask, float *dDistance,
												 int32_t *dObject, int32_t *dElement, float *dBary, uint64_t *dStats, void *stream) {
	const char *fn = "snail_instances_materials_mirror_packets_dev";
	// the arguments first, the handle last (as snail_instances_materials_create judges its host data): what is refused here needs no device
	if(nPackets <= 0) return 0;
	if(!cam || resx <= 0 || resy <= 0 || !dPacketXY || !dT || !dSamples || !dOrigin || !dDir || !dIDir || !dMask || !dDistance || !dObject || !dElement || !dBary ||
	   (((unsigned long long)dT | (unsigned long long)dSamples | (unsigned long long)dOrigin | (unsigned long long)dDir | (unsigned long long)dIDir | (unsigned long long)dDistance |
		 (unsigned long long)dObject | (unsigned long long)dElement | (unsigned long long)dBary) & 15)) {
		snail_set_error("%s: bad camera or resolution, a null buffer, or a buffer not 16-byte aligned", fn);
		return 1;
	}
	if(int rc = checkIMat(m, fn)) return rc;
	SnailInstances *h = m->inst;
	hipStream_t st = (hipStream_t)stream;
	DeviceGuard guard(m->device);
	std::lock_guard<std::mutex> lock(h->mu);
	dev::InstArgs I;
	bool sse, deep;
	if(int rc = instancesBegin(h, fn, I, &sse, &deep, st)) return rc;   // (the arithmetic and its tables are the BLAS scenes'; ordered as every launch of the handle)
	dev::IMatArgs A;
	imatFillArgs(m, A, I, cam, resx, resy, dPacketXY, nPackets);
	A.m.s.hitT = dT; A.m.samples = const_cast<float *>(dSamples);
	A.m.s.rOrg = dOrigin; A.m.s.rDir = dDir; A.m.s.rIDir = dIDir; A.m.s.rMask = dMask; A.m.s.rDist = dDistance; A.m.s.rObj = dObject;
	A.m.s.stats = (dev::u64 *)dStats;
	SNAIL_LAUNCH(sse, MatArgs, dim3(nPackets), dim3(64), 0, st, A.m, k_mat_mirror);
	hipError_t e = hipMemsetAsync(dElement, 0, (size_t)nPackets * 256 * 4, st);
	if(e == hipSuccess) e = hipMemsetAsync(dBary, 0, (size_t)nPackets * 256 * 8, st);
	const int rc = instancesEnd(h, st);   // (the kernel is enqueued: booked as every launch of the handle is, whatever the clears did)
	if(e != hipSuccess) { snail_set_error("%s: clearing the element and bary buffers failed: %s", fn, hipGetErrorString(e)); return 100 + (int)e; }
	return rc;
}

int snail_instances_materials_shade_rays_dev(SnailInstancesMaterials *m, int nPackets, const float *dDir, const uint8_t *dMask, const float *dT, const float *dBary,
											 const int32_t *dInst, const int32_t *dTriId, float *dSamples, void *stream) {
	const char *fn = "snail_instances_materials_shade_rays_dev";
	// the arguments first, the handle last (as snail_instances_materials_create judges its host data): what is refused here needs no device
	if(nPackets <= 0) return 0;
	if(!dDir || !dT || !dBary || !dInst || !dTriId || !dSamples ||
	   (((unsigned long long)dDir | (unsigned long long)dT | (unsigned long long)dBary | (unsigned long long)dInst | (unsigned long long)dTriId | (unsigned long long)dSamples) & 15)) {
		snail_set_error("%s: a null buffer, or a buffer not 16-byte aligned", fn);
		return 1;
	}
	if(int rc = checkIMat(m, fn)) return rc;
	SnailInstances *h = m->inst;
	hipStream_t st = (hipStream_t)stream;
	DeviceGuard guard(m->device);
	std::lock_guard<std::mutex> lock(h->mu);
	dev::InstArgs I;
	bool sse, deep;
	if(int rc = instancesBegin(h, fn, I, &sse, &deep, st)) return rc;   // (the stage reads the instance records: ordered against updates as a walk is)
	dev::IMatRaysArgs B;
	memset(&B, 0, sizeof(B));
	const float noCam[13] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 1};   // (generic packets carry their rays: no stage of this call generates any)
	imatFillArgs(m, B.a, I, noCam, 16, 16, nullptr, nPackets);
	B.a.m.s.rDir = const_cast<float *>(dDir); B.a.m.s.rMask = const_cast<uint8_t *>(dMask); B.a.m.s.rDist = const_cast<float *>(dT);
	B.a.m.s.rObj = const_cast<int32_t *>(dTriId);
	B.a.m.rU = dBary; B.a.m.rV = dBary + 4; B.a.m.rUVStride = 8;
	B.a.m.nSamples = dSamples;
	B.rInst = dInst;
	SNAIL_IMAT_RAYS_LAUNCH(sse, dim3(nPackets), st, B, k_imat_sample_rays);
	return instancesEnd(h, st);
}

int snail_instances_materials_bounce_dev(SnailInstancesMaterials *m, const float cam[13], int resx, int resy, const float *lights7, int nLights,
										 const float ambient[3], int flags, uint8_t *frame, int pitch, uint64_t *dStats, void *stream) {
	const char *fn = "snail_instances_materials_bounce_dev";
	if(int rc = checkIMatBounceFrameArgs(fn, cam, resx, resy, lights7, nLights, ambient, flags)) return rc;
	if(int rc = checkIMat(m, fn)) return rc;
	if(!frame || pitch < resx * 3) { snail_set_error("%s: null frame or a pitch below 3 * resx", fn); return 1; }
	return frameDev<IMatLevels>(m, fn, cam, resx, resy, lights7, nLights, ambient, (flags & SNAIL_RENDER_REFLECTIONS) != 0, 0, frame, pitch, nullptr, dStats, stream);
}

int snail_instances_materials_bounce_packets_dev(SnailInstancesMaterials *m, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets,
												 const float *lights7, int nLights, const float ambient[3], int flags, uint8_t *bgrPackets, uint64_t *dStats,
												 void *stream) {
	const char *fn = "snail_instances_materials_bounce_packets_dev";
	if(int rc = checkIMatBounceFrameArgs(fn, cam, resx, resy, lights7, nLights, ambient, flags)) return rc;
	if(int rc = checkIMat(m, fn)) return rc;
	if(!dPacketXY && nPackets > 0) { snail_set_error("%s: null packet list", fn); return 1; }
	if(nPackets <= 0) return 0;
	if(!bgrPackets || ((unsigned long long)bgrPackets & 3)) { snail_set_error("%s: null or unaligned output", fn); return 1; }
	return framePacketsDev<IMatLevels>(m, fn, cam, resx, resy, dPacketXY, nPackets, lights7, nLights, ambient, (flags & SNAIL_RENDER_REFLECTIONS) != 0, 0, bgrPackets, nullptr, dStats, stream);
}

int snail_instances_materials_bounce_image(SnailInstancesMaterials *m, const float cam[13], int resx, int resy, const float *lights7, int nLights,
										   const float ambient[3], int flags, uint8_t *image, int pitch, uint64_t stats[4]) {
	const char *fn = "snail_instances_materials_bounce_image";
	if(int rc = checkIMatBounceFrameArgs(fn, cam, resx, resy, lights7, nLights, ambient, flags)) return rc;
	if(int rc = checkIMat(m, fn)) return rc;
	if(!image || pitch < resx * 3) { snail_set_error("%s: null image or a pitch below 3 * resx", fn); return 1; }
	return frameImage<IMatLevels>(m, fn, cam, resx, resy, lights7, nLights, ambient, (flags & SNAIL_RENDER_REFLECTIONS) != 0, 0, image, pitch, nullptr, stats);
}

} // extern "C"
