// materials.inc -- full shading of the primary packets of a plain scene (include/snail_materials.h): the gVals[6] && HasShadingData() branch of
// Scene::RayTrace (src/scene_trace.cpp:145-358) and, on its samples, the lights of the simple-shading pipeline.  Included once per arithmetic
// after instances_shade.inc, into the same namespace (dev / dev_sse).  Always over an explicit packet list, one wave per packet or per
// (packet, light), lane q = quad q, the reference's block of 4 quads = lanes 4b .. 4b + 3:
//   k_mat_sample           hit records (t, u, v, triId) + ShTriangle records + materials + textures -> 9 floats per ray (normal, diffuse,
//                          specular), component-major [packet][component][quad][lane]: every store instruction writes one contiguous KB
//   k_mat_light<DEEP>      one wave per (packet, light): position + the sample's normal -> light cull -> shadow packet -> TraverseShadow ->
//                          the surviving distances [light][packet][256]                         Scene::TraceLight, src/scene_trace.cpp:523-566
//   k_mat_final            the tail of TraceLight per light, outColor = diffuse * lDiffuse + specular * lSpecular, ConvColor, store  :567-601, :484-512
// hitBounds / lightCulled / shadowLane and the shadow walks are the plain pipeline's device functions, called on these samples; what differs is
// that N.L takes the interpolated normal and that diffuse and specular are two buffers.  Table look-ups in their fully checked form.
// With the one mirrored bounce of gVals[7] (include/snail_materials_bounce.h; src/scene_trace.cpp:454-466, :603-618), between k_mat_sample and
// k_mat_light:
//   k_mat_mirror           primary samples -> mirrored packets (Reflect about the INTERPOLATED normal) + lane masks, in the layout and masked-lane
//                          convention of k_final<SRC_PRIMARY, DST_MIRROR>; books the nested call's TracingRays           Scene::TraceReflection
//   k_rays<false, true>    TraversePrimary<0, 1> of the mirrored packets, with barycentrics (launchRays, unchanged)
//   k_mat_sample_rays      the sample stage on generic packets: RayGroup<0, hasMask>, hasMask = not all 256 lanes selected (:615-617)
//   k_mat_light_rays<DEEP> / k_mat_colour_rays   the nested lights and outColor as FLOATS [packet][256][3] (no ConvColor)
// and k_mat_final_blend instead of k_mat_final: diffuse += (colour - diffuse) * 0.3 on the hit lanes, before the lights (:462-465).
// For the tile renderer (include/snail_materials_tiles.h) the primary colour stage has a float exit: k_mat_colour / k_mat_colour_blend leave outColor
// as floats [packet][256][3] in ShadeArgs::colPackets, and k_inst_store (instances_shade.inc) goes on from there.
// The sample, light and colour stages are ONE body each, templated by their source (SRC_PRIMARY: rays from the camera, a hit = t < inf;
// SRC_MIRROR: rays, masks and hits from the mirrored-packet buffers, a hit = t < inf AND the lane's mask bit: a masked lane carries -inf, not
// inf); the primary kernels keep their names.  The sample body, matSample, also serves instanced scenes and the transparent kinds.
namespace SNAIL_DEV_NS {

enum { MAT_SIMPLE = 0, MAT_TEX = 1, MAT_UBER = 2, MAT_TRANSPARENT = 3 };   // (MAT_TRANSPARENT: only in a set made for materials_transparency.inc)
struct MatRec {            // 48 bytes, read as three dwordx4
	int kind, ndotr;
	float col[3], spec[3];
	int tex, pad[3];
};
struct TexRec {            // 96 bytes
	unsigned long long base;   // first byte of level 0 in MatArgs::texels
	int w, h, mips, pad;
	unsigned lvl[16];          // byte offset of level m from base
	unsigned pad2[2];
};
struct MatArgs {
	ShadeArgs s;               // FIRST: its hostTab opens the kernel-argument segment.  hitT / hitId = the primary hits; nodes / tris / pf / relLight: the shadow walks
	const float *hitU, *hitV;  // barycentric.x / .y of the primary hits, packet-major
	const uint4 *shtris;       // ShTriangle records, 4 x uint4 each, triId order
	int nTris;
	const int *matMap;
	int nMap;
	const MatRec *mats;
	int nMats;
	const TexRec *tex;
	const unsigned char *texels;
	float *samples;            // [packet][9][64][4]
	// SRC_MIRROR (generic packets: s.rDir / s.rOrg / s.rMask (null = all lanes selected) / s.rDist / s.rObj are rays and hits, indexed by list position)
	const float *rU, *rV;      // barycentric.x / .y of those hits: quad q's four lanes at rU + q * rUVStride (8: launchRays' bary buffer, 4: planes)
	int rUVStride;
	float *nSamples;           // the samples of the generic packets, [packet][9][64][4]
	float *nSDist;             // their shadow distances, [light][packet][256]
};

// RayGenerator::Generate for the lane's quad, exactly as in loadSamples (checked look-ups)
__device__ __forceinline__ void matRays(const ShadeArgs &A, const PacketPos &P, int lane, float (&d)[3][4]) {
	const int ty = lane >> 2, k4 = lane & 3;
#pragma unroll
	for(int l = 0; l < 4; l++) {
		const float xoff = (float)(P.px + (l >= 2 ? 2 : 0)), yoff = (float)(P.py - (l >= 2 ? 1 : 0));
		const float tposx = (float)(4 * k4) + xoff, tposy = (float)ty + yoff;
		const float p0 = A.g.tright[0] * tposx + (A.g.tup[0] * tposy + A.g.txyz[0][l]);
		const float p1 = A.g.tright[1] * tposx + (A.g.tup[1] * tposy + A.g.txyz[1][l]);
		const float p2 = A.g.tright[2] * tposx + (A.g.tup[2] * tposy + A.g.txyz[2][l]);
		const float rs = RSqrt(p0 * p0 + p1 * p1 + p2 * p2);
		d[0][l] = p0 * rs; d[1][l] = p1 * rs; d[2][l] = p2 * rs;
	}
}

struct ShTri {
	float uv[3][2], nrm[3][3];
	int matId;
};
__device__ __forceinline__ ShTri loadShTri(const MatArgs &A, int idx) {
	const uint4 *r = A.shtris + (size_t)idx * 4;
	const uint4 a = r[0], b = r[1], c = r[2], e = r[3];
	ShTri T;
	T.uv[0][0] = asf(a.x); T.uv[0][1] = asf(a.y); T.uv[1][0] = asf(a.z); T.uv[1][1] = asf(a.w);
	T.uv[2][0] = asf(b.x); T.uv[2][1] = asf(b.y);
	T.nrm[0][0] = asf(b.z); T.nrm[0][1] = asf(b.w); T.nrm[0][2] = asf(c.x);
	T.nrm[1][0] = asf(c.y); T.nrm[1][1] = asf(c.z); T.nrm[1][2] = asf(c.w);
	T.nrm[2][0] = asf(e.x); T.nrm[2][1] = asf(e.y); T.nrm[2][2] = asf(e.z);
	T.matId = (int)e.w;
	return T;
}
// BVH::GetMaterialId(shTri.MatId()) = materials[idx].id (src/bvh/tree.h:82-84); -1 = defaultMat.  (The set's creation has checked every record and
// entry; the tests here only keep a corrupted table from turning into an address.)
__device__ __forceinline__ int matIdOf(const MatArgs &A, int shMatId) {
	const int idx = shMatId & 0x7fffffff;
	if(idx >= A.nMap) return -1;
	const int m = A.matMap[idx];
	return (unsigned)m < (unsigned)A.nMats ? m : -1;
}

// PointSampler::Sample for one ray (src/sampling/point_sampler.cpp:126-210): every operation rounded separately, in the order written
__device__ __forceinline__ void matSampleTex(const MatArgs &A, int texIdx, float cu, float cv, float tdx, float tdy, float (&out)[3]) {
	const TexRec *T = A.tex + texIdx;
	const int w = T->w, h = T->h, mips = T->mips;
	const float wMul = (float)(w - 1), hMul = (float)(h - 1);
	// ClampTexCoord: coord - float(int(coord)), + 1 if negative
	float ux = cu - (float)(int)cu, uy = cv - (float)(int)cv;
	ux = ux < 0.0f ? ux + 1.0f : ux;
	uy = uy < 0.0f ? uy + 1.0f : uy;
	const float px = ux * wMul, py = uy * hMul;
	// the mip: texDiff is the quad's (broadcast), so Minimize over the quad is the value itself
	const float ax = tdx * wMul, ay = tdy * hMul;
	const float mn = ax < ay ? ax : ay;
	unsigned pixels = (unsigned)(long long)(mn * 0.6f);   // uint(float) of the x86-64 build: cvttss2si to 64 bits, low word
	int mip = pixels ? 32 - __builtin_clz(pixels) : 0;           // while(pixels) { mip++; pixels >>= 1; }
	mip = mip < mips - 1 ? mip : mips - 1;
	const unsigned char *data = A.texels + T->base + T->lvl[mip & 15];
	const int wm = w >> mip, pitch = 3 * (wm > 1 ? wm : 1);
	int x1 = (int)px, y1 = (int)py;
	int x2 = x1 + 1, y2 = y1 + 1;
	const float dx = px - (float)x1, dy = py - (float)y1;
	y1 = h - y1; y2 = h - y2;
	x1 >>= mip; y1 >>= mip; x2 >>= mip; y2 >>= mip;
	const int xm = (w - 1) >> mip, ym = (h - 1) >> mip;
	x1 &= xm; y1 &= ym; x2 &= xm; y2 &= ym;
	x1 = x1 + x1 + x1; x2 = x2 + x2 + x2;
	y1 *= pitch; y2 *= pitch;
	const int o[4] = {x1 + y1, x2 + y1, x1 + y2, x2 + y2};
	float ch[4][3];
#pragma unroll
	for(int k = 0; k < 4; k++) {
		// a tap = ONE 4-byte load at byte alignment (offsets are multiples of 3), three bytes of it used, as the reference's DATA(a, b); the device
		// copy of every texture is padded by 4 bytes for the last texel's.  Chosen by the resource report over three byte loads: the same VGPRs,
		// SGPRs and occupancy, 32 instructions fewer per kernel (profiles/materials.txt)
		unsigned v;
		__builtin_memcpy(&v, data + o[k], 4);
		ch[k][0] = (float)(int)(v & 255u); ch[k][1] = (float)(int)((v >> 8) & 255u); ch[k][2] = (float)(int)((v >> 16) & 255u);
	}
#pragma unroll
	for(int c = 0; c < 3; c++) {   // Lerp(a, b, x) = a + (b - a) * x (veclib/vecbase.h:80)
		const float top = ch[0][c] + (ch[1][c] - ch[0][c]) * dx;
		const float bot = ch[2][c] + (ch[3][c] - ch[2][c]) * dx;
		out[c] = (top + (bot - top) * dy) * (1.0f / 255.0f);
	}
}

// broadcast of the block's first lane (lanes 4b .. 4b + 3 -> lane 4b): quad_perm [0, 0, 0, 0]
__device__ __forceinline__ int blockFirst(int v) { return __builtin_amdgcn_mov_dpp(v, 0x00, 0xf, 0xf, true); }
// broadcast of lane I of the block (quad_perm [I, I, I, I])
template <int I>
__device__ __forceinline__ int blockLane(int v) { return __builtin_amdgcn_mov_dpp(v, I * 0x55, 0xf, 0xf, true); }
// a predicate over all four lanes of the block
__device__ __forceinline__ bool blockAll(bool p, int lane) {
	const unsigned long long b = __builtin_amdgcn_ballot_w64(p);
	return ((b >> (lane & ~3)) & 15ull) == 15ull;
}

// (a + b * x) + c * y and a + (b * x + c * y): the two associations of src/scene_trace.cpp:204 / :218-220,:245-249,:272-279
__device__ __forceinline__ float lerpL(float a, float b, float c, float x, float y) { return (a + b * x) + c * y; }
__device__ __forceinline__ float lerpR(float a, float b, float c, float x, float y) { return a + (b * x + c * y); }

// the packet of a stage's block: the list entry (SRC_PRIMARY), or the list position alone (SRC_MIRROR: generic packets have no place in a frame)
template <int SRC>
__device__ __forceinline__ PacketPos matPacket(const MatArgs &A, int li) {
	if(SRC != SRC_MIRROR) return packetOf(A.s, li);
	PacketPos P;
	P.px = P.py = 0; P.pidx = (size_t)li; P.valid = true;
	return P;
}

// a level's order list (TranspArgs::inOrder and its kin): a packet whose word is negative is not part of the level; null: every packet
__device__ __forceinline__ bool orderSkipped(const int *order, int li) { return order && __builtin_amdgcn_readfirstlane(order[li]) < 0; }

// The key of a plain scene's hit: the triId alone, clamped to nTris; the record through loadShTri, its material through matIdOf.  No slot: the
// constant 0 folds every slot comparison of matSample away.
struct MatKey {
	typedef MatArgs Args;
	enum { SLOTS = 0 };
	static __device__ __forceinline__ const MatArgs &mat(const MatArgs &A) { return A; }
	static __device__ __forceinline__ void slots(const MatArgs &, const int *, size_t, int (&s)[4]) { s[0] = s[1] = s[2] = s[3] = 0; }
	static __device__ __forceinline__ int tri(const MatArgs &A, int id) {
		const int i = id < 0 ? 0 : id;
		return i < A.nTris ? i : A.nTris - 1;
	}
	static __device__ __forceinline__ ShTri load(const MatArgs &A, int, int tri, int &mat) {
		const ShTri T = loadShTri(A, tri);
		mat = matIdOf(A, T.matId);
		return T;
	}
};

// ---- one packet: the sample stage, hit records -> the nine planes of the sample buffer (+ [T] Sample::opacity and the transSel selector) ----
// ONE body for the eight sample kernels, instantiated over three compile-time axes:
//   SRC     SRC_PRIMARY: the camera's rays and the primary hits (every lane selected, RayGroup<0, 0>)            k_*_sample, k_*_sample_transp
//           SRC_MIRROR: GENERIC packets, RayGroup<0, hasMask> (the nested calls of the bounce and of a transparency level): the directions read
//           from the packet, a hit = t < inf AND the lane's mask bit, the bary stride, the packet's own hasMask   k_*_sample_rays, k_*_sample_transp_rays
//   KEY     MatKey (above): a plain scene, the key is triId                                                       k_mat_sample*
//           IMatKey (instances_materials.inc): an instanced scene, the key is the pair (slot, triId) -- every equality of :171-356 is on the
//           pair (object, element), as the reference compares wherever isctFlags & fElement is set (:162, :179-182, :252-253, :263) --, the
//           record through imatLoadTri                                                                            k_imat_sample*
//   TRANSP  the lines marked [T]: the kinds that can select a transparent lane (TransparentMaterial<NDotR>, UberMaterial's dissFactor),
//           Sample::opacity per ray, the transSel selector after the opacity < 1 filter (:190, :306, :347-349, :472) and the level's order
//           list (inOrder, opacity, selOut: null without)                                                         k_*_sample_transp*
// X is the kernel's argument record (KEY::Args, MatArgs inside it), inst the slots of the hits (null for MatKey).
// The planes of a set without the [T] kinds are the same byte for byte with TRANSP on or off; with it off the code holds no load of
// MatRec::pad, no second texture sample, no opac / flagged / winner scan and no store of opacity or selector.
template <int SRC, bool TRANSP, class KEY>
__device__ __forceinline__ void matSample(const typename KEY::Args &X, const int *inst, const int *inOrder, float *opacity, unsigned char *selOut) {
	const MatArgs &A = KEY::mat(X);
	const int lane = threadIdx.x & 63;
	const int li = (int)blockIdx.x;
	if(li >= A.s.nPackets || (TRANSP && orderSkipped(inOrder, li))) return;   // [T] a packet outside its level's call is skipped
	const PacketPos P = matPacket<SRC>(A, li);
	const size_t quad = P.pidx * 64 + lane;
	const float inf = __builtin_inff();
	float d[3][4];
	unsigned mask4 = 15u;
	if(SRC == SRC_MIRROR) {
		loadQuad3(A.s.rDir, quad, d);
		if(A.s.rMask) mask4 = A.s.rMask[quad] & 15u;
	} else matRays(A.s, P, lane, d);
	// hasMask is the PACKET's: RayGroup<0, 0> when all 256 lanes are selected, RayGroup<0, 1> otherwise (src/scene_trace.cpp:615-617, :631-633)
	const bool pktMasked = SRC == SRC_MIRROR && __builtin_amdgcn_ballot_w64(mask4 != 15u) != 0;
	float bx[4], by[4];
	bool hit[4];
	int obj[4], slt[4];
	{
		const size_t uvq = SRC == SRC_MIRROR ? quad * (size_t)A.rUVStride : quad * 4;
		const float4 tv = *(const float4 *)((SRC == SRC_MIRROR ? A.s.rDist : A.s.hitT) + quad * 4);
		const float4 uv = *(const float4 *)((SRC == SRC_MIRROR ? A.rU : A.hitU) + uvq), vv = *(const float4 *)((SRC == SRC_MIRROR ? A.rV : A.hitV) + uvq);
		const int4 iv = *(const int4 *)((SRC == SRC_MIRROR ? (const int *)A.s.rObj : A.s.hitId) + quad * 4);
		const float t[4] = {tv.x, tv.y, tv.z, tv.w};
		const int id[4] = {iv.x, iv.y, iv.z, iv.w};
		int sl[4];
		KEY::slots(X, inst, quad, sl);
		bx[0] = uv.x; bx[1] = uv.y; bx[2] = uv.z; bx[3] = uv.w;
		by[0] = vv.x; by[1] = vv.y; by[2] = vv.z; by[3] = vv.w;
#pragma unroll
		for(int l = 0; l < 4; l++) {
			hit[l] = t[l] < inf && ((mask4 >> l) & 1u) != 0;   // mask = tDistance < maxDist && selector, :157
			const int i = KEY::tri(X, id[l]), s = sl[l];   // (scalars, so that both lines below are selects: the hit records stay one dwordx4 load each)
			slt[l] = hit[l] ? s : 0;       // object = Condition(mask, tObject, 0), :161
			obj[l] = hit[l] ? i : 0;       // element = Condition(mask, tElement, 0), :162 (a plain scene's object, :161)
		}
	}
	// mask4 == 0x0f0f0f0f, and the 16 objects -- (object, element) pairs -- equal to the block's first (:178-182)
	const bool full = blockAll(hit[0] && hit[1] && hit[2] && hit[3], lane);
	const int obj0b = blockFirst(obj[0]), slt0b = KEY::SLOTS ? blockFirst(slt[0]) : 0;
	const bool single = blockAll(obj[0] == obj0b && obj[1] == obj0b && obj[2] == obj0b && obj[3] == obj0b &&
								 slt[0] == slt0b && slt[1] == slt0b && slt[2] == slt0b && slt[3] == slt0b, lane) && full;

	float nrm[3][4], tc[2][4], tdx = 0.0f, tdy = 0.0f;
	int mid[4];
#pragma unroll
	for(int l = 0; l < 4; l++) { nrm[0][l] = nrm[1][l] = nrm[2][l] = 0.0f; tc[0][l] = tc[1][l] = 0.0f; mid[l] = -1; }
	if(single) {
		// (a): one triangle (of one instance) for the block
		int m;
		const ShTri T = KEY::load(X, slt0b, obj0b, m);
		const bool flat = T.matId < 0;
		const bool texd = m >= 0 && (A.mats[m].kind == MAT_TEX || (TRANSP && A.mats[m].kind == MAT_TRANSPARENT));   // Material::fTexCoords  [T]: TransparentMaterial carries it too
#pragma unroll
		for(int l = 0; l < 4; l++) {
			mid[l] = m;
			if(texd) {
#pragma unroll
				for(int c = 0; c < 2; c++) tc[c][l] = lerpL(T.uv[0][c], T.uv[1][c], T.uv[2][c], bx[l], by[l]);
#pragma unroll
				for(int c = 0; c < 3; c++) nrm[c][l] = lerpL(T.nrm[0][c], T.nrm[1][c], T.nrm[2][c], bx[l], by[l]);
			} else {
#pragma unroll
				for(int c = 0; c < 3; c++) nrm[c][l] = flat ? T.nrm[0][c] : lerpR(T.nrm[0][c], T.nrm[1][c], T.nrm[2][c], bx[l], by[l]);
			}
		}
		if(texd) {   // texDiff = Maximize(texCoord) - Minimize(texCoord) of the quad (:219; finite values: the fold's order is immaterial)
			tdx = vmax(vmax(tc[0][0], tc[0][1]), vmax(tc[0][2], tc[0][3])) - vmin(vmin(tc[0][0], tc[0][1]), vmin(tc[0][2], tc[0][3]));
			tdy = vmax(vmax(tc[1][0], tc[1][1]), vmax(tc[1][2], tc[1][3])) - vmin(vmin(tc[1][0], tc[1][1]), vmin(tc[1][2], tc[1][3]));
		}
	} else {
		// (b): per quad; lane 0's triangle for all four lanes if lane 0 hit, then lanes 1..3 whose key differs from lane 0's -- triId 0, or
		// (slot 0, triId 0), when lane 0 missed or is masked: a lane that hit (slot 0's) triangle 0 beside it keeps the default material and zero
		// normal / texCoord.  A record is loaded (and transformed) only on lanes that hit.
		if(hit[0]) {
			int m;
			const ShTri T = KEY::load(X, slt[0], obj[0], m);
#pragma unroll
			for(int l = 0; l < 4; l++) {
				mid[l] = hit[l] ? m : -1;
#pragma unroll
				for(int c = 0; c < 2; c++) tc[c][l] = lerpL(T.uv[0][c], T.uv[1][c], T.uv[2][c], bx[l], by[l]);
#pragma unroll
				for(int c = 0; c < 3; c++) nrm[c][l] = lerpL(T.nrm[0][c], T.nrm[1][c], T.nrm[2][c], bx[l], by[l]);
			}
		}
#pragma unroll
		for(int l = 1; l < 4; l++)
			if(hit[l] && (obj[l] != obj[0] || slt[l] != slt[0])) {
				const ShTri T = KEY::load(X, slt[l], obj[l], mid[l]);
#pragma unroll
				for(int c = 0; c < 2; c++) tc[c][l] = lerpL(T.uv[0][c], T.uv[1][c], T.uv[2][c], bx[l], by[l]);
#pragma unroll
				for(int c = 0; c < 3; c++) nrm[c][l] = lerpL(T.nrm[0][c], T.nrm[1][c], T.nrm[2][c], bx[l], by[l]);
			}
	}
	// One material for 16 hit rays: Shade unmasked (:224, :301-308) -- an instanced scene's ids index ONE scene-wide list, so two BLASes'
	// triangles of one material meet here --; otherwise (c) every selected lane by its own material on the masked path (:310-355).  The
	// per-material masks of (c) are disjoint -- a lane has one matId -- and a masked Shade writes only its own lanes, so the order in which the
	// reference walks its material list cannot show: shading each lane once by its own material is the same.
	// Branch (a) calls Shade with the packet's own hasMask (:224), (b)'s single-material call is RayGroup<.., 0> whatever the packet is (:308).
	const int mid0b = blockFirst(mid[0]);
	const bool unmasked = blockAll(mid[0] == mid0b && mid[1] == mid0b && mid[2] == mid0b && mid[3] == mid0b, lane) && full && !(single && pktMasked);

	float diff[3][4], spec[3][4], opac[4];
	int flagged[4];   // [T] the lane's material when it carries Material::fTransparency and the lane is selected, else -1
#pragma unroll
	for(int l = 0; l < 4; l++) {
		// the lane's material: loaded values of an unrolled loop (compile-time indices), never a runtime-indexed array
		int kind = MAT_SIMPLE, ndotr = 1, tex = 0, tex2 = 0;
		float col[3] = {1.0f, 1.0f, 1.0f}, sp[3] = {0.0f, 0.0f, 0.0f}, dissolve = 0.0f;   // defaultMat = SimpleMaterial<true>(1, 1, 1), src/scene.cpp:6
		if(mid[l] >= 0) {
			const uint4 *r = (const uint4 *)(A.mats + mid[l]);
			const uint4 a = r[0], b = r[1], c = r[2];
			kind = (int)a.x; ndotr = (int)a.y;
			col[0] = asf(a.z); col[1] = asf(a.w); col[2] = asf(b.x);
			sp[0] = asf(b.y); sp[1] = asf(b.z); sp[2] = asf(b.w);
			tex = (int)c.x;
			if(TRANSP) { tex2 = (int)c.y; dissolve = asf(c.z); }   // [T] MatRec::pad[0], pad[1]: the opacity map, the dissolve factor
		}
		const float dn = d[0][l] * nrm[0][l] + d[1][l] * nrm[1][l] + d[2][l] * nrm[2][l];
		const float adn = __builtin_fabsf(dn);
		float t1[3] = {0.0f, 0.0f, 0.0f}, t2[3] = {0.0f, 0.0f, 0.0f};
		// the kinds present among the wave's lanes: a branch per kind that needs code of its own, skipped when no lane has it
		if(__builtin_amdgcn_ballot_w64(kind == MAT_TEX && hit[l]) != 0) {
			if(kind == MAT_TEX && hit[l]) matSampleTex(A, tex, tc[0][l], tc[1][l], tdx, tdy, t1);
		}
		// [T] TransparentMaterial::Shade_: both samplers with mipmapping off (Sample(samples, sc, 0)) -- level 0 whatever texDiff says
		if(TRANSP && __builtin_amdgcn_ballot_w64(kind == MAT_TRANSPARENT && hit[l]) != 0) {
			if(kind == MAT_TRANSPARENT && hit[l]) {
				matSampleTex(A, tex, tc[0][l], tc[1][l], 0.0f, 0.0f, t1);
				matSampleTex(A, tex2, tc[0][l], tc[1][l], 0.0f, 0.0f, t2);
			}
		}
#pragma unroll
		for(int c = 0; c < 3; c++) {
			float df, sf;
			if(kind == MAT_TEX || (TRANSP && kind == MAT_TRANSPARENT)) { df = ndotr ? t1[c] * dn : t1[c]; sf = df; }
			else if(kind == MAT_UBER) { df = col[c] * adn; sf = unmasked ? df : sp[c]; }
			else { df = ndotr ? col[c] * adn : col[c]; sf = df; }
			diff[c][l] = hit[l] ? df : 0.0f;
			spec[c][l] = hit[l] ? sf : 0.0f;
			nrm[c][l] = hit[l] ? nrm[c][l] : 0.0f;
		}
		if(TRANSP) {
			// [T] Sample::opacity: temp1.x of the opacity sampler / dissFactor; the other kinds never write it (read before written: zero)
			const float op = kind == MAT_TRANSPARENT ? t2[0] : kind == MAT_UBER ? dissolve : 0.0f;
			opac[l] = hit[l] ? op : 0.0f;
			const bool fl = kind == MAT_TRANSPARENT || (kind == MAT_UBER && dissolve > 0.0f);   // UberMaterial: fTransparency iff dissolveFactor > 0
			flagged[l] = (hit[l] && fl) ? mid[l] : -1;
		}
	}
	unsigned sel = 0;
	if(TRANSP) {
		// [T] transSel.  (a) / (b): the block's one material's flag for the whole block (:190, :306).  (c): for each material of the block's list that
		// carries the flag, IN THE LIST'S ORDER -- first appearance over the quads, then the lanes, among the selected lanes -- transSel[b4 + q] =
		// mask[q] is ASSIGNED for all four quads (:347-349): the last flagged material of the list wins.  One rule covers the three branches: the
		// winner is the flagged material whose first appearance comes latest; a block of one material has one candidate.  A material's identity
		// in an instanced scene is its index in the ONE scene-wide list: two BLASes' triangles of one entry are one candidate.
		if(__builtin_amdgcn_ballot_w64((flagged[0] & flagged[1] & flagged[2] & flagged[3]) != -1) != 0) {
			int e[16];
#pragma unroll
			for(int l = 0; l < 4; l++) {
				e[0 + l] = blockLane<0>(flagged[l]); e[4 + l] = blockLane<1>(flagged[l]);
				e[8 + l] = blockLane<2>(flagged[l]); e[12 + l] = blockLane<3>(flagged[l]);
			}
			int win = -1;
#pragma unroll
			for(int p = 0; p < 16; p++) {
				bool first = e[p] >= 0;
#pragma unroll
				for(int k = 0; k < p; k++) first = first && e[k] != e[p];
				win = first ? e[p] : win;
			}
#pragma unroll
			for(int l = 0; l < 4; l++)
				sel |= (win >= 0 && flagged[l] == win && opac[l] < 1.0f) ? (1u << l) : 0u;   // transSel[q] &= ForWhich(opacity < 1.0f), :472
		}
	}
	float4 *o = (float4 *)((SRC == SRC_MIRROR ? A.nSamples : A.samples) + P.pidx * (9 * 256)) + lane;
#pragma unroll
	for(int c = 0; c < 3; c++) {
		o[(0 + c) * 64] = make_float4(nrm[c][0], nrm[c][1], nrm[c][2], nrm[c][3]);
		o[(3 + c) * 64] = make_float4(diff[c][0], diff[c][1], diff[c][2], diff[c][3]);
		o[(6 + c) * 64] = make_float4(spec[c][0], spec[c][1], spec[c][2], spec[c][3]);
	}
	if(TRANSP) {   // [T]
		*(float4 *)(opacity + quad * 4) = make_float4(opac[0], opac[1], opac[2], opac[3]);
		selOut[quad] = (unsigned char)sel;
	}
}
__global__ __launch_bounds__(64) void k_mat_sample(MatArgs A) { matSample<SRC_PRIMARY, false, MatKey>(A, nullptr, nullptr, nullptr, nullptr); }
__global__ __launch_bounds__(64) void k_mat_sample_rays(MatArgs A) { matSample<SRC_MIRROR, false, MatKey>(A, nullptr, nullptr, nullptr, nullptr); }

// position and hit mask as in simple shading (src/scene_trace.cpp:157-165), the normal from the sample buffer.  SRC_MIRROR: the mirrored
// packet's own rays, position = reflDir * t + reflOrig, hit = t < inf and the lane's mask bit, the normal from the nested sample buffer.
template <int SRC>
__device__ __forceinline__ void matLoadSamples(const MatArgs &A, const PacketPos &P, int lane, Samples &S) {
	const size_t quad = P.pidx * 64 + lane;
	const float inf = __builtin_inff();
	float d[3][4], org[3][4];
	unsigned mask4 = 15u;
	if(SRC == SRC_MIRROR) {
		loadQuad3(A.s.rDir, quad, d);
		loadQuad3(A.s.rOrg, quad, org);
		if(A.s.rMask) mask4 = A.s.rMask[quad] & 15u;
	} else {
		matRays(A.s, P, lane, d);
#pragma unroll
		for(int c = 0; c < 3; c++)
#pragma unroll
			for(int l = 0; l < 4; l++) org[c][l] = A.s.g.org[c];
	}
	const float4 tv = *(const float4 *)((SRC == SRC_MIRROR ? A.s.rDist : A.s.hitT) + quad * 4);
	const float t[4] = {tv.x, tv.y, tv.z, tv.w};
	const float4 *sm = (const float4 *)((SRC == SRC_MIRROR ? A.nSamples : A.samples) + P.pidx * (9 * 256)) + lane;
	const float4 n0 = sm[0], n1 = sm[64], n2 = sm[128];
	const float nn[3][4] = {{n0.x, n0.y, n0.z, n0.w}, {n1.x, n1.y, n1.z, n1.w}, {n2.x, n2.y, n2.z, n2.w}};
#pragma unroll
	for(int l = 0; l < 4; l++) {
		S.hit[l] = t[l] < inf && (SRC != SRC_MIRROR || ((mask4 >> l) & 1u) != 0);
		S.sdn[l] = 0.0f;
#pragma unroll
		for(int c = 0; c < 3; c++) { S.pos[c][l] = d[c][l] * t[l] + org[c][l]; S.nrm[c][l] = nn[c][l]; }
	}
}
// ---- one (packet, light): the shadow packet (src/scene_trace.cpp:538-558) and BVH::TraverseShadow, by the walks of lightPacket ----
// TWINS: the set-up and the walk selection below are those of lightPacket (snail_dev.inc; its main pass and its deferred M_EXACT pass folded into
// one kernel, look-ups checked), and k_inst_light (instances_shade.inc) has the same set-up around the instanced walk.  A change to the shadow
// packet, to the classify / walkSharedAsm / walk dispatch or to the stats booking belongs in all three.  imatLight (instances_materials.inc)
// is this function's sample load and set-up around k_inst_light's walk: a change to the shadow packet belongs there as well.
// SRC_MIRROR: the nested call's lights on the mirrored packets' samples -- the same shadow packet (the light's shared origin) and walks.
// PSTATS: the heat-map launches' instantiation (include/snail_materials_heatmap.h), which also books the (packet, light)'s counters per packet at
// P.pidx -- a template argument as in snail_dev.inc, so that the other launches' kernels stay the code they were.  A culled pair has returned
// before the booking: it books nothing.
template <bool DEEP, int SRC, bool PSTATS = false>
__device__ __forceinline__ void matLight(const MatArgs &A, float *lds) {
	const int lane = threadIdx.x & 63;
	const int li = (int)blockIdx.x, n = (int)blockIdx.y;
	if(li >= A.s.nPackets || n >= A.s.nLights) return;
	const PacketPos P = matPacket<SRC>(A, li);
	const float lp[3] = {A.s.lights[n][0], A.s.lights[n][1], A.s.lights[n][2]};
	const float radius = A.s.lights[n][6], radSq = radius * radius;
	Quad Q;
	{
		Samples S;
		matLoadSamples<SRC>(A, P, lane, S);
		float tMin[3], tMax[3];
		hitBounds(S, tMin, tMax);
		if(lightCulled(tMin, tMax, lp, radSq)) return;   // (wave-uniform; k_mat_final skips the light by the same test)
#pragma unroll
		for(int l = 0; l < 4; l++) {
			float sd[3], distance, dotv;
			shadowLane(S, l, lp, sd, distance, dotv, Q.dist[l]);
#pragma unroll
			for(int c = 0; c < 3; c++) { Q.d[c][l] = sd[c]; Q.id[c][l] = S.hit[l] ? InvDiv(sd[c] + 0.00000001f) : 0.0f; }
		}
	}
	unsigned rays = 0;   // stats.TracingRays(CountMaskBits(ForWhich(mask))), :557
#pragma unroll
	for(int l = 0; l < 4; l++) rays += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(Q.dist[l] > 0.0f));
	float lorg[3][4];
#pragma unroll
	for(int c = 0; c < 3; c++)
#pragma unroll
		for(int l = 0; l < 4; l++) lorg[c][l] = lp[c];
	Counters st = {0, 0, 0, 0, 0};
	int stid[4];
	float bu[4], bv[4];
	// the walk lightPacket picks for this packet (the same counters); a packet that needs M_EXACT (a non-finite value: practically never) is
	// walked here instead of in a second launch
	const bool fin = finite4(Q.id) && finite4(Q.d);
	int oct;
	const int mode = classify(A.s.fastOK != 0 && originSaneDev(lp), fin, true, Q.id, Q.dist, oct);
	if(mode == M_EXACT) walk<true, false, true, M_EXACT, false, DEEP, false>(A.s.nodes, A.s.tris, 64, lane, lorg, Q, 15u, stid, bu, bv, lds, st);
	else if(DEEP) {
		if(mode == M_COH) walk<true, false, true, M_COH, false, DEEP, false>(A.s.nodes, A.s.tris, 64, lane, lorg, Q, 15u, stid, bu, bv, lds, st, oct);
		else walk<true, false, true, M_FAST, false, DEEP, false>(A.s.nodes, A.s.tris, 64, lane, lorg, Q, 15u, stid, bu, bv, lds, st);
	} else if(A.s.pack) {
		const uint4 *pn = A.s.relLight[n];   // this light's origin-relative records
		if(mode == M_COH) walkSharedAsm<true, true, true, false, false, false>(pn, A.s.tris, 64, lane, lorg, Q, 15u, stid, bu, bv, lds, st, oct);
		else walkSharedAsm<true, false, true, false, false, false>(pn, A.s.tris, 64, lane, lorg, Q, 15u, stid, bu, bv, lds, st, 0);
	} else if(mode == M_COH) walkSharedAsm<true, true, false, false, false, false>(A.s.nodes, A.s.tris, 64, lane, lorg, Q, 15u, stid, bu, bv, lds, st, oct);
	else walkSharedAsm<true, false, false, false, false, false>(A.s.nodes, A.s.tris, 64, lane, lorg, Q, 15u, stid, bu, bv, lds, st, 0);
	flushStats(A.s.stats, st, rays, lane);
	if(PSTATS) bookPacketLate<ShadeArgs>(P.pidx, st, rays, lane);
	*(float4 *)((SRC == SRC_MIRROR ? A.nSDist : A.s.sDist) + ((size_t)n * (size_t)A.s.nPackets + P.pidx) * 256 + (size_t)lane * 4) = make_float4(Q.dist[0], Q.dist[1], Q.dist[2], Q.dist[3]);
}
template <bool DEEP>
__global__ __launch_bounds__(64) void k_mat_light(MatArgs A) {
	__shared__ float lds[LDS_FLOATS_PER_WAVE];
	matLight<DEEP, SRC_PRIMARY>(A, lds);
}
template <bool DEEP>
__global__ __launch_bounds__(64) void k_mat_light_rays(MatArgs A) {
	__shared__ float lds[LDS_FLOATS_PER_WAVE];
	matLight<DEEP, SRC_MIRROR>(A, lds);
}
template <bool DEEP>
__global__ __launch_bounds__(64) void k_mat_light_heat(MatArgs A) {
	__shared__ float lds[LDS_FLOATS_PER_WAVE];
	matLight<DEEP, SRC_PRIMARY, true>(A, lds);
}

// ---- one packet: the lights' contributions from the surviving distances, the colour and its store (shadeAndStore with two sample colours) ----
// TWINS: the per-light tail, the colour sum, ConvColor and both stores (packet-major words; the frame's three aligned dwords or the byte-wise
// tail, with the alignment rule) are shadeAndStore's (snail_dev.inc, non-fused, checked form), which k_final and k_inst_final (instances_shade.inc)
// call; this copy differs only in taking diffuse and specular from the sample buffer.  A change to the attenuation or to the store rule belongs
// in both.
// SRC_MIRROR: the nested call's outColor, stored as FLOATS r, g, b per ray in A.s.rCol [packet][256][3] (the analogue of k_final<SRC_MIRROR,
// DST_COLOR>).  BLEND (primary): diffuse = diffuse + (reflColor - diffuse) * 0.3 on the selector's lanes (= the hit lanes) before the lights,
// specular untouched (src/scene_trace.cpp:462-465).
// FLOATS (primary): outColor stays FLOATS r, g, b per ray in A.s.colPackets [packet][256][3] -- the layout k_inst_store (instances_shade.inc) reads --
// for the tile renderer's reduction, tint and stores (include/snail_materials_tiles.h); the store rule below is not repeated for them.
// TWINS: the BLEND expression and its rounding are repeated by k_mat_blend_refl / _rays (materials_tree.inc), which blends in place in the sample
// buffer so that the transparency blend can follow it; a change to the factor or the order of the three operations belongs there too.
template <int SRC, bool BLEND, bool FLOATS = false>
__device__ __forceinline__ void matFinal(const MatArgs &A) {
	const int lane = threadIdx.x & 63;
	const int li = (int)blockIdx.x;
	if(li >= A.s.nPackets) return;
	const PacketPos P = matPacket<SRC>(A, li);
	const size_t quad = P.pidx * 64 + lane;
	Samples S;
	matLoadSamples<SRC>(A, P, lane, S);
	float lDiff[3][4], lSpec[3][4];
#pragma unroll
	for(int c = 0; c < 3; c++)
#pragma unroll
		for(int l = 0; l < 4; l++) { lDiff[c][l] = A.s.ambient[c]; lSpec[c][l] = 0.0f; }
	if(A.s.nLights) {
		float tMin[3], tMax[3];
		hitBounds(S, tMin, tMax);
		const size_t packets = (size_t)A.s.nPackets;
		for(int n = 0; n < A.s.nLights; n++) {
			const float lp[3] = {A.s.lights[n][0], A.s.lights[n][1], A.s.lights[n][2]};
			const float lc[3] = {A.s.lights[n][3], A.s.lights[n][4], A.s.lights[n][5]};
			const float radius = A.s.lights[n][6], iRadius = 1.0f / radius, radSq = radius * radius;
			if(lightCulled(tMin, tMax, lp, radSq)) continue;
			const float4 sv = *(const float4 *)((SRC == SRC_MIRROR ? A.nSDist : A.s.sDist) + ((size_t)n * packets + P.pidx) * 256 + (size_t)lane * 4);
			const float sdist[4] = {sv.x, sv.y, sv.z, sv.w};
#pragma unroll
			for(int l = 0; l < 4; l++) {
				float sd[3], distance, dotv, unused;
				shadowLane(S, l, lp, sd, distance, dotv, unused);
				if(sdist[l] > 0.0f) {
					float atten = distance * iRadius;
					atten = Max<M_EXACT>(0.0f, ((1.0f - atten) * 0.2f + FastInv(16.0f * atten * atten)) - 0.0625f);
					const float diffMul = dotv * atten;
					float specMul = dotv;
					specMul *= specMul; specMul *= specMul; specMul *= specMul; specMul *= specMul;
					specMul *= atten;
#pragma unroll
					for(int c = 0; c < 3; c++) { lDiff[c][l] += lc[c] * diffMul; lSpec[c][l] += lc[c] * specMul; }
				}
			}
		}
	}
	// outColor = diffuse * lDiffuse + specular * lSpecular, or diffuse without lights (src/scene_trace.cpp:504-512)
	const float4 *sm = (const float4 *)((SRC == SRC_MIRROR ? A.nSamples : A.samples) + P.pidx * (9 * 256)) + lane;
	float col[3][4];
#pragma unroll
	for(int c = 0; c < 3; c++) {
		const float4 dv = sm[(3 + c) * 64], sv = sm[(6 + c) * 64];
		float df[4] = {dv.x, dv.y, dv.z, dv.w};
		const float sf[4] = {sv.x, sv.y, sv.z, sv.w};
		if(BLEND) {
#pragma unroll
			for(int l = 0; l < 4; l++) {
				const float refl = A.s.rCol[(quad * 4 + l) * 3 + c];
				if(S.hit[l]) df[l] = df[l] + (refl - df[l]) * 0.3f;
			}
		}
#pragma unroll
		for(int l = 0; l < 4; l++) col[c][l] = A.s.nLights ? df[l] * lDiff[c][l] + sf[l] * lSpec[c][l] : df[l];
	}
	if(SRC == SRC_MIRROR) {
#pragma unroll
		for(int l = 0; l < 4; l++) {
			float *rc = A.s.rCol + (quad * 4 + l) * 3;
			rc[0] = col[0][l]; rc[1] = col[1][l]; rc[2] = col[2][l];
		}
		return;
	}
	if(FLOATS) {
		float4 *o = (float4 *)(A.s.colPackets + quad * 12);
		o[0] = make_float4(col[0][0], col[1][0], col[2][0], col[0][1]);
		o[1] = make_float4(col[1][1], col[2][1], col[0][2], col[1][2]);
		o[2] = make_float4(col[2][2], col[0][3], col[1][3], col[2][3]);
		return;
	}
	unsigned bytes[12];
#pragma unroll
	for(int l = 0; l < 4; l++) { bytes[l * 3 + 0] = (unsigned)convChannelW(col[2][l]); bytes[l * 3 + 1] = (unsigned)convChannelW(col[1][l]); bytes[l * 3 + 2] = (unsigned)convChannelW(col[0][l]); }
	if(A.s.bgrPackets) {
		unsigned *o = (unsigned *)(A.s.bgrPackets + (quad * 4) * 3);
#pragma unroll
		for(int k = 0; k < 3; k++) o[k] = bytes[4 * k] | (bytes[4 * k + 1] << 8) | (bytes[4 * k + 2] << 16) | (bytes[4 * k + 3] << 24);
		return;
	}
	const int yy = P.py + (lane >> 2), xx = P.px + (lane & 3) * 4;
	if(yy < A.s.resy) {
		unsigned char *dd = A.s.frame + (size_t)yy * A.s.pitch + (size_t)xx * 3;
		if(xx + 3 < A.s.resx && (A.s.pitch & 3) == 0 && ((unsigned long long)A.s.frame & 3) == 0) {
			unsigned *dw = (unsigned *)dd;
#pragma unroll
			for(int k = 0; k < 3; k++) dw[k] = bytes[4 * k] | (bytes[4 * k + 1] << 8) | (bytes[4 * k + 2] << 16) | (bytes[4 * k + 3] << 24);
		} else {
#pragma unroll
			for(int l = 0; l < 4; l++)
				if(xx + l < A.s.resx) { dd[l * 3 + 0] = (unsigned char)bytes[l * 3 + 0]; dd[l * 3 + 1] = (unsigned char)bytes[l * 3 + 1]; dd[l * 3 + 2] = (unsigned char)bytes[l * 3 + 2]; }
		}
	}
}
__global__ __launch_bounds__(64) void k_mat_final(MatArgs A) { matFinal<SRC_PRIMARY, false>(A); }
__global__ __launch_bounds__(64) void k_mat_final_blend(MatArgs A) { matFinal<SRC_PRIMARY, true>(A); }
__global__ __launch_bounds__(64) void k_mat_colour_rays(MatArgs A) { matFinal<SRC_MIRROR, false>(A); }
__global__ __launch_bounds__(64) void k_mat_colour(MatArgs A) { matFinal<SRC_PRIMARY, false, true>(A); }
__global__ __launch_bounds__(64) void k_mat_colour_blend(MatArgs A) { matFinal<SRC_PRIMARY, true, true>(A); }

// ---- one packet: primary samples -> mirrored packets.  Scene::TraceReflection (src/scene_trace.cpp:603-618) on the samples of full shading:
// reflDir = Reflect(dir, samples.normal) (src/rtbase_math.h:54-58) with the INTERPOLATED normal of the sample buffer (zeros on a lane that missed),
// reflOrig = position + reflDir * 0.001, idir = SafeInv(reflDir); selector = hit lanes.
// TWINS: the output -- layout, zeros for masked lanes, distance inf / -inf (:112-115), object 0, one mask byte per quad, the nested call's
// TracingRays(CountMaskBits(mask)) (:116-117) and, in the table arithmetic, SafeInv one component at a time -- is that of k_final<SRC_PRIMARY,
// DST_MIRROR> (snail_dev.inc); only the normal's source differs.
// TWINS: k_mat_mirror_rays (materials_tree.inc) is this body with a level's generic packets (matLoadSamples<SRC_MIRROR>) as its source, under that
// level's order list; a change to Reflect, the offset, the layout or the booking belongs there too.
// PSTATS (k_mat_mirror_heat, the heat-map launches of include/snail_materials_heatmap.h): the nested call's TracingRays per packet as well, as
// matLight's.  The body is materials_mirror_body.inc, included once per kernel.
__global__ __launch_bounds__(64) void k_mat_mirror(MatArgs A) {
#define SNAIL_MIRROR_PSTATS 0
#include "materials_mirror_body.inc"
#undef SNAIL_MIRROR_PSTATS
}
__global__ __launch_bounds__(64) void k_mat_mirror_heat(MatArgs A) {
#define SNAIL_MIRROR_PSTATS 1
#include "materials_mirror_body.inc"
#undef SNAIL_MIRROR_PSTATS
}

} // namespace SNAIL_DEV_NS
