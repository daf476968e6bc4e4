// materials_tiles_host.inc -- host side of the tile renderer of full-shaded plain scenes (include/snail_materials_tiles.h); included by
// snail_hip.hip after materials_host.inc.  The host calls are renderTilesHost / renderFrameHost of materials_levels_host.inc with matShadeStore as
// their store step (matStoreStep).  RenderTask::Work (src/render.cpp:47-211) around the staged pipeline of materials_host.inc:
//   [k_inst_aa_packets: the four double-resolution packets of every packet]  ->  the scene's primary walk into hit distances (depth shading) or
//   matShade with float colours (k_mat_colour / k_mat_colour_blend)  ->  k_inst_store: reduction, tint, ConvColor, packet-major bytes or the
//   tiles' planes.
// Nothing here has a store rule of its own: k_inst_aa_packets, k_inst_store (instances_shade.inc) and the tile job (InstTileJob,
// instances_tiles_host.inc) are the instanced scenes', which read no instance data.
namespace {

const int kMatTileFlags = SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_DEPTH | SNAIL_RENDER_AA4;

// everything that can be judged without the handle; the flags first
int matTilesArgsOk(const char *fn, const float *cam, int resx, int resy, const float *lights7, int nLights, const float *ambient, int flags, const float *tint) {
	if(flags & ~kMatTileFlags) {
		snail_set_error("%s: unknown bits in flags (got 0x%x): SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_DEPTH | SNAIL_RENDER_AA4", fn, flags);
		return 1;
	}
	if(!cam || resx <= 0 || resy <= 0 || resx > (1 << 20) || resy > (1 << 20)) { snail_set_error("%s: bad camera or resolution", fn); return 1; }
	if(nLights < 0 || nLights > SNAIL_MAX_LIGHTS || (nLights && !lights7) || !ambient) {
		snail_set_error("%s: bad arguments (at most %d lights, ambient)", fn, SNAIL_MAX_LIGHTS);
		return 1;
	}
	if(tint && !(std::isfinite(tint[0]) && std::isfinite(tint[1]) && std::isfinite(tint[2]))) { snail_set_error("%s: the tint is not finite", fn); return 1; }
	return 0;
}

#define SNAIL_MAT_STORE(D, AA, PL) SNAIL_LAUNCH(sse, InstStoreArgs, dim3(np), dim3(64), 0, st, S, k_inst_store<D, AA, PL>)

// One run of the pipeline over the np packets of dXY with any flags and tint, into packet-major bytes (bgrPackets) or the planes of J's tiles
// (J->dOut); intermediates from the set's next group; the scene's mu held.
int matShadeStore(SnailMaterials *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights,
				  const float ambient[3], int flags, const float *tint, uint8_t *bgrPackets, const InstTileJob *J, uint64_t *dStats, hipStream_t st) {
	SnailScene *s = m->scene;
	const bool aa = (flags & SNAIL_RENDER_AA4) != 0, depth = (flags & SNAIL_RENDER_DEPTH) != 0;
	const bool refl = !depth && (flags & SNAIL_RENDER_REFLECTIONS) != 0;
	const size_t n = aa ? (size_t)np * 4 : (size_t)np;
	const int rx = aa ? resx * 2 : resx, ry = aa ? resy * 2 : resy;
	const int nl = depth ? 0 : nLights;
	ShadeSets::Set *Wp = nullptr;
	if(int rc = setsNext(m, (int)n, nl, refl, true, st, &Wp)) return rc;
	ShadeSets::Set &W = *Wp;
	SnailMaterials::Bufs B;
	B.carve(W.base, n);
	SnailMaterials::BounceBufs RB;
	if(refl) RB.carve(W.bounce, n, nl);
	SnailMaterials::TileBufs T;
	T.carve(W.tiles, n);
	int rc = 0;
	const int32_t *list = dXY;
	if(aa) {
		hipLaunchKernelGGL(dev::k_inst_aa_packets, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const int2 *)dXY, np, (int2 *)T.xy2);
		list = T.xy2;
	}
	const float *in = nullptr;
	if(depth) {   // gVals[1] returns before the full-shading branch: the hit distances of the scene's primary walk alone
		SceneUse use(s, st);
		rc = use.rc;
		if(!rc) rc = launchPrimary(s, cam, rx, ry, 0, 0, 0, 0, list, (int)n, B.hitT, nullptr, nullptr, nullptr, dStats, st);
		in = B.hitT;
	} else {
		rc = matShade(m, fn, cam, rx, ry, list, (int)n, lights7, nl, ambient, nullptr, 0, nullptr, B, refl ? &RB : nullptr, dStats, st, T.col);
		in = T.col;
	}
	if(!rc) {
		const bool sse = s->arith == SNAIL_ARITH_HOST_SSE;
		dev::InstStoreArgs S;
		memset(&S, 0, sizeof(S));
		S.hostTab = sse ? s->dTab : nullptr;
		S.in = in;
		S.nPackets = np;
		if(tint) { S.tinted = 1; for(int c = 0; c < 3; c++) S.tint[c] = tint[c]; }
		S.bgrPackets = bgrPackets;
		if(J) {
			S.tiles = (const int4 *)J->dTiles; S.packetTile = J->dPacketTile; S.firstPacket = J->dFirst; S.outOff = (const long long *)J->dOff;
			S.out = J->dOut; S.resx = resx; S.resy = resy;
		}
		switch((depth ? 4 : 0) | (aa ? 2 : 0) | (J ? 1 : 0)) {
		case 0: SNAIL_MAT_STORE(false, false, false); break;
		case 1: SNAIL_MAT_STORE(false, false, true); break;
		case 2: SNAIL_MAT_STORE(false, true, false); break;
		case 3: SNAIL_MAT_STORE(false, true, true); break;
		case 4: SNAIL_MAT_STORE(true, false, false); break;
		case 5: SNAIL_MAT_STORE(true, false, true); break;
		case 6: SNAIL_MAT_STORE(true, true, false); break;
		default: SNAIL_MAT_STORE(true, true, true); break;
		}
		const hipError_t e = hipGetLastError();
		if(e != hipSuccess) { snail_set_error("%s: k_inst_store: %s", fn, hipGetErrorString(e)); rc = 100 + (int)e; }
	}
	return setDone(W, fn, rc, st);
}
#undef SNAIL_MAT_STORE

// ... as the store step of renderTilesHost / renderFrameHost (materials_levels_host.inc), which hand it levelsStore's arguments: the opaque stages
// have no levels, truncation counter, heat mode or per-packet counters
const auto matStoreStep = [](SnailMaterials *m, const char *fn, const float cam[13], int resx, int resy, const int32_t *dXY, int np, const float *lights7, int nLights,
							 const float ambient[3], int flags, const float *tint, uint8_t *bgrPackets, const InstTileJob *J, int, uint64_t *, uint64_t *dStats, hipStream_t st,
							 bool, uint32_t *) { return matShadeStore(m, fn, cam, resx, resy, dXY, np, lights7, nLights, ambient, flags, tint, bgrPackets, J, dStats, st); };

} // namespace

extern "C" {

int snail_materials_frame_packets_dev(SnailMaterials *m, const float cam[13], int resx, int resy, const int32_t *dPacketXY, int nPackets, const float *lights7,
									  int nLights, const float ambient[3], int flags, const float *tint, uint8_t *bgrPackets, uint64_t *dStats, void *stream) {
	const char *fn = "snail_materials_frame_packets_dev";
	if(int rc = matTilesArgsOk(fn, cam, resx, resy, lights7, nLights, ambient, flags, tint)) return rc;
	if(nPackets > 0 && !dPacketXY) { snail_set_error("%s: null packet list", fn); return 1; }
	if(nPackets > (1 << 24)) { snail_set_error("%s: more than 2^24 packets", fn); return 1; }
	if(nPackets > 0 && (!bgrPackets || ((unsigned long long)bgrPackets & 3))) { snail_set_error("%s: null or unaligned output", fn); return 1; }
	if(int rc = checkMaterials(m, fn)) return rc;
	if(nPackets <= 0) return 0;
	if(!tint && !(flags & (SNAIL_RENDER_DEPTH | SNAIL_RENDER_AA4)))   // the lit packets as they are: the merged path, bytes from k_mat_final / k_mat_final_blend
		return framePacketsDev<MatLevels>(m, fn, cam, resx, resy, dPacketXY, nPackets, lights7, nLights, ambient, (flags & SNAIL_RENDER_REFLECTIONS) != 0, 0, bgrPackets, nullptr, dStats, stream);
	DeviceGuard guard(m->device);
	SNAIL_LOCK(m->scene);
	return matShadeStore(m, fn, cam, resx, resy, dPacketXY, nPackets, lights7, nLights, ambient, flags, tint, bgrPackets, nullptr, dStats, (hipStream_t)stream);
}

int snail_materials_render_tiles(SnailMaterials *m, const float cam[13], int resx, int resy, const int32_t *coords, const int64_t *offsets, int nTiles,
								 const float *lights7, int nLights, const float ambient[3], int flags, const float *tint, uint8_t *data, uint64_t stats[4]) {
	const char *fn = "snail_materials_render_tiles";
	if(int rc = matTilesArgsOk(fn, cam, resx, resy, lights7, nLights, ambient, flags, tint)) return rc;
	if(nTiles > 0 && (!coords || !offsets || !data)) { snail_set_error("%s: null buffer", fn); return 1; }
	if(int rc = tileRectsOk(fn, coords, nTiles)) return rc;
	if(int rc = checkMaterials(m, fn)) return rc;
	if(nTiles <= 0) return 0;
	return renderTilesHost<MatLevels>(m, fn, cam, resx, resy, coords, offsets, nTiles, lights7, nLights, ambient, flags, tint, data, 0, nullptr, stats, false, matStoreStep);
}

int snail_materials_render_frame(SnailMaterials *m, const float cam[13], int resx, int resy, const float *lights7, int nLights, const float ambient[3], int flags,
								 uint8_t *image, int pitch, uint64_t stats[4]) {
	const char *fn = "snail_materials_render_frame";
	if(int rc = matTilesArgsOk(fn, cam, resx, resy, lights7, nLights, ambient, flags, nullptr)) return rc;
	if(!image || pitch < resx * 3) { snail_set_error("%s: null image or a pitch below 3 * resx", fn); return 1; }
	if(int rc = checkMaterials(m, fn)) return rc;
	if(!(flags & (SNAIL_RENDER_AA4 | SNAIL_RENDER_DEPTH)))   // exactly snail_materials_bounce_image
		return frameImage<MatLevels>(m, fn, cam, resx, resy, lights7, nLights, ambient, (flags & SNAIL_RENDER_REFLECTIONS) != 0, 0, image, pitch, nullptr, stats);
	return renderFrameHost<MatLevels>(m, fn, cam, resx, resy, lights7, nLights, ambient, flags, image, pitch, 0, nullptr, stats, false, matStoreStep);
}

} // extern "C"
