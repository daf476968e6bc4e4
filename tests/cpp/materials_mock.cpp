// Compile-and-run check of the Render(...) overloads of include/snail_adapter.hpp with and without SNAIL_ADAPTER_DEVICE_MATERIALS (given on the
// compiler's command line: -DSNAIL_ADAPTER_DEVICE_MATERIALS), against MOCK types with the reference's member names (as tests/cpp/heatmap_mock.cpp).
// With the macro, gVals[6] on a scene with shading data and an attached material set is rendered on the device (snail_materials_render_tiles /
// snail_materials_render_frame, include/snail_materials_tiles.h): the tile list with gVals[8] (rank 3) and gVals[9], the image with gVals[7].  Without
// an attached set, with gVals[5] and no gVals[1], and for an image with gVals[8], the reference's own renderer -- a stub that counts -- is reached
// instead.  Without the macro every gVals[6] call reaches the stub, attached set or not.
//   materials_mock <dir>
// reads the scene, its shading data, camera, lights, tiles and offsets from <dir> (written by tests/test_gpu_materials_tiles.py) and writes
// out_tiles.bin (the caller's whole `data` buffer, gaps included), out_img.bin and stats.txt for the caller to hold against the restatement.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <algorithm>
#include <vector>

// ---- mock reference types (names and members as in the reference) ----
using std::vector;
typedef unsigned int uint;
int gVals[16] = {0};
struct Vec3f { float x, y, z; };
struct Camera { float plane_dist; Vec3f pos, right, up, front; };
struct TreeStats {
	unsigned in = 0, it = 0, sk = 0, rays = 0;
	void Intersection(unsigned v = 1) { in += v; }
	void LoopIteration(unsigned v = 1) { it += v; }
	void Skip(unsigned v = 1) { sk += v; }
	void TracingRays(unsigned v = 1) { rays += v; }
};
struct Options { Options() { reflections = rdtscShader = 0; } bool reflections, rdtscShader; };
struct Light { Vec3f pos, color; float radius, radSq, iRadius; };
struct MipmapTexture {
	int w = 0, h = 0, pitch = 0; std::vector<unsigned char> bytes;
	int Width() const { return w; } int Height() const { return h; } int Pitch() const { return pitch; }
	void *DataPointer() { return bytes.data(); }
};
struct Vec3q { float x[4], y[4], z[4]; };
struct floatq { float v[4]; };
struct i32x4 { int v[4]; };
struct Vec2q { float x[4], y[4]; };
template <bool so, bool mask> struct RayGroup {
	enum { sharedOrigin = so, hasMask = mask };
	const Vec3q *origin, *dir, *idir; int size; char *maskp;
	const Vec3q *OriginPtr() const { return origin; }
	const Vec3q *DirPtr() const { return dir; }
	const Vec3q *IDirPtr() const { return idir; }
};
template <bool so, bool mask> struct Context {
	RayGroup<so, mask> rays; floatq *distance; i32x4 *object; i32x4 *element; Vec2q *barycentric; TreeStats *stats;
	int Size() const { return rays.size; }
	char *MaskPtr() { return rays.maskp; }
};
struct ShadowContext {
	RayGroup<1, 0> rays; floatq *distance; TreeStats *stats;
	int Size() const { return rays.size; }
};
struct Node { float b[6]; unsigned sub; int aux; };
struct Triangle { float f[16]; };
struct ShTriangle { float f[16]; };
struct BBox { Vec3f min, max; };
struct MockBVH {
	typedef Triangle CElement; typedef ShTriangle SElement;
	enum { isctFlags = 1, maxDepth = 64 };
	std::vector<Node> nodes; std::vector<Triangle> tris; std::vector<ShTriangle> shTris; int depth = 0;
	bool shading = false;   // (the mock's stand-in for a scene loaded with materials)
	bool HasShadingData() const { return shading; }
	const ShTriangle &GetSElement(int e, int) const { return shTris[e]; }
	Vec3f GetNormal(int e, int) const { return Vec3f{tris[e].f[12], tris[e].f[13], tris[e].f[14]}; }
	int GetMaterialId(int, int) const { return 0; }
	BBox GetBBox() const { return BBox{{nodes[0].b[0], nodes[0].b[1], nodes[0].b[2]}, {nodes[0].b[3], nodes[0].b[4], nodes[0].b[5]}}; }
};
template <class AccStruct> struct Scene {
	AccStruct geometry;
	Vec3f ambientLight{0.1f, 0.1f, 0.1f};
	vector<Light> lights;
};
// the reference's generic Render templates (src/render.h:16-23): the host renderer, a stub that counts its calls and writes nothing
static int hostCalls = 0;
template <class AccStruct>
TreeStats Render(const Scene<AccStruct> &, const Camera &, uint, uint, unsigned char *, const vector<int> &, const vector<int> &, const Options, uint, uint) {
	hostCalls++;
	return TreeStats();
}
template <class AccStruct> TreeStats Render(const Scene<AccStruct> &, const Camera &, MipmapTexture &, const Options, uint) {
	hostCalls++;
	return TreeStats();
}

#define SNAIL_ADAPTER_RENDER_OVERLOADS
#include "../../include/snail_adapter.hpp"

#ifdef SNAIL_ADAPTER_DEVICE_MATERIALS
static const bool kOptedIn = true;
#else
static const bool kOptedIn = false;
#endif

template <class T> static std::vector<T> slurp(const std::string &path) {
	FILE *f = std::fopen(path.c_str(), "rb");
	if(!f) { std::perror(path.c_str()); std::exit(2); }
	std::fseek(f, 0, SEEK_END); long n = std::ftell(f); std::fseek(f, 0, SEEK_SET);
	std::vector<T> v(n / sizeof(T)); if(n && std::fread(v.data(), 1, n, f) != (size_t)n) std::exit(2); std::fclose(f); return v;
}
static void dumpBytes(const std::string &path, const std::vector<unsigned char> &v) {
	FILE *f = std::fopen(path.c_str(), "wb");
	if(!f) { std::perror(path.c_str()); std::exit(2); }
	std::fwrite(v.data(), 1, v.size(), f); std::fclose(f);
}
#define FAIL(code, what) do { std::printf("FAILED: %s\n", what); return code; } while(0)

int main(int argc, char **argv) {
	// the three-argument and four-argument forms of UnsupportedSwitch keep their meaning: gVals[6] with shading data is a reason
	{
		int gv[16] = {0};
		gv[6] = 1;
		if(!snail::UnsupportedSwitch(gv, true, true) || !snail::UnsupportedSwitch(gv, true, false, true) || snail::UnsupportedSwitch(gv, false, true)) FAIL(20, "UnsupportedSwitch changed");
		if(snail::UnsupportedSwitch(gv, true, true, false, true) || !snail::UnsupportedSwitch(gv, true, true, false, false)) FAIL(21, "UnsupportedSwitch with a material set");
		gv[8] = 1;
		if(snail::UnsupportedSwitch(gv, true, true, false, true) || !snail::UnsupportedSwitch(gv, true, false, false, true)) FAIL(22, "gVals[8]: tile list only");
		gv[8] = 0; gv[5] = 1;
		if(!snail::UnsupportedSwitch(gv, true, true, true, true)) FAIL(23, "gVals[5] without gVals[1] stays on the host");
		gv[1] = 1;
		if(snail::UnsupportedSwitch(gv, true, true, true, true)) FAIL(24, "gVals[5] under gVals[1] is the depth frame");
	}
	if(argc < 2) { std::printf("compiled and linked %s SNAIL_ADAPTER_DEVICE_MATERIALS\n", kOptedIn ? "with" : "without"); return 0; }
	const std::string d = std::string(argv[1]) + "/";
	const std::vector<int> meta = slurp<int>(d + "meta.bin");   // resx, resy, hostSse, depth, image width, image height, nTex, (w, h) per texture
	const int resx = meta[0], resy = meta[1], iw = meta[4], ih = meta[5], nTex = meta[6];
	MockBVH bvh;
	bvh.nodes = slurp<Node>(d + "nodes.bin");
	bvh.tris = slurp<Triangle>(d + "tris.bin");
	bvh.depth = meta[3];
	bvh.shading = true;
	const std::vector<float> c = slurp<float>(d + "cam.bin"), ci = slurp<float>(d + "cam_img.bin");
	const Camera cam{c[12], {c[0], c[1], c[2]}, {c[3], c[4], c[5]}, {c[6], c[7], c[8]}, {c[9], c[10], c[11]}};
	const Camera camImg{ci[12], {ci[0], ci[1], ci[2]}, {ci[3], ci[4], ci[5]}, {ci[6], ci[7], ci[8]}, {ci[9], ci[10], ci[11]}};
	Scene<snail::HipBVH<MockBVH>> scene;
	const std::vector<float> l7 = slurp<float>(d + "lights7.bin");
	for(size_t i = 0; i + 6 < l7.size(); i += 7) scene.lights.push_back(Light{{l7[i], l7[i + 1], l7[i + 2]}, {l7[i + 3], l7[i + 4], l7[i + 5]}, l7[i + 6], l7[i + 6] * l7[i + 6], 1.0f / l7[i + 6]});
	scene.geometry.Upload(bvh, 0);
	if(meta[2] && !scene.geometry.SetArith(SNAIL_ARITH_HOST_SSE)) { std::fprintf(stderr, "SetArith(HOST_SSE): %s\n", snail_last_error()); return 3; }
	if(scene.geometry.Materials() != nullptr) FAIL(4, "a fresh tree has a material set");
	// the material set over the uploaded tree
	const std::vector<unsigned char> shtris = slurp<unsigned char>(d + "shtris.bin");
	const std::vector<int32_t> matMap = slurp<int32_t>(d + "matmap.bin");
	const std::vector<SnailMaterial> mats = slurp<SnailMaterial>(d + "mats.bin");
	std::vector<std::vector<unsigned char>> levels((size_t)nTex);
	std::vector<SnailTexture> tex((size_t)nTex);
	for(int k = 0; k < nTex; k++) {
		levels[(size_t)k] = slurp<unsigned char>(d + "tex" + std::to_string(k) + ".bin");
		tex[(size_t)k].levels = levels[(size_t)k].data(); tex[(size_t)k].width = meta[7 + 2 * k]; tex[(size_t)k].height = meta[8 + 2 * k];
	}
	SnailMaterials *set = snail_materials_create(scene.geometry.Handle(), shtris.data(), (int)(shtris.size() / 64), matMap.data(), (int)matMap.size(), mats.data(), (int)mats.size(),
												 tex.data(), nTex);
	if(!set) FAIL(5, snail_last_error());
	const std::vector<int> coords = slurp<int>(d + "tiles.bin"), offsets = slurp<int>(d + "offsets.bin");
	size_t total = 0;
	for(size_t k = 0; k < offsets.size(); k++) total = std::max(total, (size_t)offsets[k] + (size_t)3 * coords[k * 4 + 2] * coords[k * 4 + 3]);
	total += 3;
	const int pitch = iw * 3 + 5;
	std::vector<unsigned char> data(total, 0xA5);
	MipmapTexture img; img.w = iw; img.h = ih; img.pitch = pitch; img.bytes.assign((size_t)pitch * ih, 0xA5);
	const std::vector<unsigned char> untouchedData = data, untouchedImg = img.bytes;

	// 1. no set attached: every gVals[6] call is the host renderer's
	gVals[6] = 1; gVals[9] = 1;
	(void)Render(scene, cam, (uint)resx, (uint)resy, data.data(), coords, offsets, Options(), 3u, 4u);
	(void)Render(scene, camImg, img, Options(), 4);
	if(hostCalls != 2 || data != untouchedData || img.bytes != untouchedImg) FAIL(6, "without a set gVals[6] must reach the host renderer");
	scene.geometry.AttachMaterials(set);
	if(scene.geometry.Materials() != set) FAIL(7, "AttachMaterials");
	// 2. gVals[5] without gVals[1], and an image with gVals[8]: the host renderer, with a set attached too
	gVals[5] = 1;
	(void)Render(scene, cam, (uint)resx, (uint)resy, data.data(), coords, offsets, Options(), 3u, 4u);
	(void)Render(scene, camImg, img, Options(), 4);
	gVals[5] = 0; gVals[8] = 1;
	(void)Render(scene, camImg, img, Options(), 4);
	gVals[8] = 0; gVals[9] = 0;
	if(hostCalls != 5 || data != untouchedData || img.bytes != untouchedImg) FAIL(8, "gVals[5] without gVals[1] / an image with gVals[8] must reach the host renderer");
	if(scene.geometry.HaveFrame()) FAIL(9, "a prefetched frame was left behind");
	// 3. the tile list with gVals[8] (rank 3) and gVals[9]; the image with gVals[7]
	gVals[8] = 1; gVals[9] = 1;
	const TreeStats ts = Render(scene, cam, (uint)resx, (uint)resy, data.data(), coords, offsets, Options(), 3u, 4u);
	gVals[8] = 0; gVals[9] = 0; gVals[7] = 1;
	const TreeStats is = Render(scene, camImg, img, Options(), 4);
	gVals[7] = 0; gVals[6] = 0;
	if(kOptedIn) {
		if(hostCalls != 5) FAIL(10, "with a set attached gVals[6] must stay on the device");
		if(data == untouchedData || img.bytes == untouchedImg) FAIL(11, "nothing was rendered");
	} else {
		if(hostCalls != 7 || data != untouchedData || img.bytes != untouchedImg) FAIL(12, "without the macro gVals[6] must reach the host renderer");
	}
	dumpBytes(d + "out_tiles.bin", data);
	dumpBytes(d + "out_img.bin", img.bytes);
	FILE *f = std::fopen((d + "stats.txt").c_str(), "w");
	if(!f) return 2;
	std::fprintf(f, "tiles %u %u %u %u\nimg %u %u %u %u\n", ts.in, ts.it, ts.rays, ts.sk, is.in, is.it, is.rays, is.sk);
	std::fclose(f);
	scene.geometry.AttachMaterials(nullptr);
	snail_materials_destroy(set);
	std::printf("materials adapter ok (%s SNAIL_ADAPTER_DEVICE_MATERIALS), host renderer reached %d times\n", kOptedIn ? "with" : "without", hostCalls);
	return 0;
}
