// The routing of the Render(...) overloads of include/snail_adapter.hpp under SNAIL_ADAPTER_DEVICE_MATERIALS_HEATMAP, against MOCK reference types
// and a mock C-ABI (as tests/cpp/materials_tree_mock.cpp): nothing touches a device and the program does not link libsnailhip.so.  The macros
// come from the compiler's command line:
//   -DSNAIL_ADAPTER_DEVICE_MATERIALS [-DSNAIL_ADAPTER_DEVICE_TRANSPARENCY] [-DSNAIL_ADAPTER_DEVICE_MATERIALS_HEATMAP] [-DSNAIL_ADAPTER_NO_HOST_RENDERER]
//   materials_heat_mock routing     gVals[6] && gVals[5] && !gVals[1] goes to the _heat_ functions with maxDepth 8, gVals[7], [9] and on tile lists [8]
//                                   (with the macro) or to the host renderer (without: today's routing); under gVals[1], with gVals[8] on an image, with
//                                   a set that can select but no SNAIL_ADAPTER_DEVICE_TRANSPARENCY, or without a set, nothing changes
//   materials_heat_mock truncated   one heat call whose counter moves: the host renderer, or abort() under SNAIL_ADAPTER_NO_HOST_RENDERER
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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
	bool shading = true;
	bool HasShadingData() const { return shading; }
	const ShTriangle &GetSElement(int e, int) const { return shTris[e]; }
	Vec3f GetNormal(int e, int) const { return Vec3f{tris[e].f[12], tris[e].f[13], tris[e].f[14]}; }
	int GetMaterialId(int, int) const { return 0; }
	BBox GetBBox() const { return BBox{{0, 0, 0}, {1, 1, 1}}; }
};
template <class AccStruct> struct Scene {
	AccStruct geometry;
	Vec3f ambientLight{0.1f, 0.1f, 0.1f};
	vector<Light> lights;
};
// the reference's generic Render templates (src/render.h:16-23): the host renderer, a stub that counts its calls and returns TreeStats of its own
static int hostCalls = 0;
#ifndef SNAIL_ADAPTER_NO_HOST_RENDERER
template <class AccStruct>
TreeStats Render(const Scene<AccStruct> &, const Camera &, uint, uint, unsigned char *, const vector<int> &, const vector<int> &, const Options, uint, uint) {
	hostCalls++;
	TreeStats s; s.Intersection(77);
	return s;
}
template <class AccStruct> TreeStats Render(const Scene<AccStruct> &, const Camera &, MipmapTexture &, const Options, uint) {
	hostCalls++;
	TreeStats s; s.Intersection(78);
	return s;
}
#endif

#define SNAIL_ADAPTER_RENDER_OVERLOADS
#include "../../include/snail_adapter.hpp"

// ---- the mock C-ABI: what the overloads reach, recorded ----
static int canSelect = 1, prefetched = 0;
static uint64_t moves = 0;   // what a _tree_ or _heat_ call adds to the caller's truncated-lane counter
struct Call { int n = 0, flags = -1, depth = -1; bool tint = false; };
static Call treeTiles, treeFrame, oldTiles, oldFrame, heatTiles, heatFrame;
extern "C" {
const char *snail_last_error(void) { return "mock"; }
SnailScene *snail_scene_create(const void *, int, const void *, int, int, int) { return (SnailScene *)(uintptr_t)0x10; }
void snail_scene_destroy(SnailScene *) {}
int snail_scene_arith(const SnailScene *, int *a) { if(a) *a = SNAIL_ARITH_IEEE; return 0; }
int snail_scene_set_arith(SnailScene *, int) { return 0; }
int snail_trace_frame_packets(SnailScene *, const float *, int, int, float *, float *, float *, int32_t *, uint64_t *) { prefetched++; return 0; }
int snail_materials_can_select_transparent(const SnailMaterials *) { return canSelect; }
int snail_materials_render_tiles(SnailMaterials *, const float *, int, int, const int32_t *, const int64_t *, int, const float *, int, const float *, int flags, const float *tint,
								 uint8_t *, uint64_t st[4]) {
	oldTiles.n++; oldTiles.flags = flags; oldTiles.tint = tint != nullptr; st[0] += 1;
	return 0;
}
int snail_materials_render_frame(SnailMaterials *, const float *, int, int, const float *, int, const float *, int flags, uint8_t *, int, uint64_t st[4]) {
	oldFrame.n++; oldFrame.flags = flags; st[0] += 2;
	return 0;
}
int snail_materials_tree_render_tiles(SnailMaterials *, const float *, int, int, const int32_t *, const int64_t *, int, const float *, int, const float *, int flags,
									  const float *tint, uint8_t *, int maxDepth, uint64_t *truncated, uint64_t st[4]) {
	treeTiles.n++; treeTiles.flags = flags; treeTiles.depth = maxDepth; treeTiles.tint = tint != nullptr; st[0] += 3;
	*truncated += moves;
	return 0;
}
int snail_materials_tree_render_frame(SnailMaterials *, const float *, int, int, const float *, int, const float *, int flags, uint8_t *, int, int maxDepth,
									  uint64_t *truncated, uint64_t st[4]) {
	treeFrame.n++; treeFrame.flags = flags; treeFrame.depth = maxDepth; st[0] += 4;
	*truncated += moves;
	return 0;
}
int snail_materials_render_heat_tiles(SnailMaterials *, const float *, int, int, const int32_t *, const int64_t *, int, const float *, int, int flags, const float *tint, uint8_t *,
									  int maxDepth, uint64_t *truncated, uint64_t st[4]) {
	heatTiles.n++; heatTiles.flags = flags; heatTiles.depth = maxDepth; heatTiles.tint = tint != nullptr; st[0] += 5;
	*truncated += moves;
	return 0;
}
int snail_materials_render_heat_frame(SnailMaterials *, const float *, int, int, const float *, int, int flags, uint8_t *, int, int maxDepth, uint64_t *truncated, uint64_t st[4]) {
	heatFrame.n++; heatFrame.flags = flags; heatFrame.depth = maxDepth; st[0] += 6;
	*truncated += moves;
	return 0;
}
// reached by the branches of the overloads that this program never takes (simple shading, the heat-map)
int snail_render_tiles(SnailScene *, const float *, int, int, const int32_t *, const int64_t *, int, const float *, int, const float *, const float *, int, uint8_t *, uint64_t *) { std::abort(); }
int snail_render_tiles_multi(SnailScene *const *, int, const float *, int, int, const int32_t *, const int64_t *, int, const float *, int, const float *, const float *, int, uint8_t *,
							 uint64_t *) { std::abort(); }
int snail_render_image(SnailScene *, const float *, int, int, const float *, int, const float *, const float *, int, uint8_t *, int, uint64_t *) { std::abort(); }
int snail_render_heat_tiles(SnailScene *, const float *, int, int, const int32_t *, const int64_t *, int, const float *, int, int, uint8_t *, uint64_t *) { std::abort(); }
int snail_render_heat_image(SnailScene *, const float *, int, int, const float *, int, int, uint8_t *, int, uint64_t *) { std::abort(); }
}

#if defined(SNAIL_ADAPTER_DEVICE_MATERIALS_HEATMAP) && defined(SNAIL_ADAPTER_DEVICE_MATERIALS)
static const bool kOptedIn = true;
#else
static const bool kOptedIn = false;
#endif
#define FAIL(code, what) do { std::printf("FAILED: %s\n", what); return code; } while(0)

int main(int argc, char **argv) {
	const std::string what = argc > 1 ? argv[1] : "routing";
	if((snail::kDeviceMaterialsHeatmap != 0) != kOptedIn) FAIL(1, "kDeviceMaterialsHeatmap");
	// the five-argument form keeps its meaning; the sixth lets gVals[5] through, and only for a call the materials routing takes
	int gv[16] = {0};
	gv[6] = gv[5] = 1;
	if(!snail::UnsupportedSwitch(gv, true, true, true, true) || snail::UnsupportedSwitch(gv, true, true, true, true, true) || !snail::UnsupportedSwitch(gv, true, true, true, false, true))
		FAIL(1, "UnsupportedSwitch");
	gv[8] = 1;
	if(!snail::UnsupportedSwitch(gv, true, false, true, true, true) || snail::UnsupportedSwitch(gv, true, true, true, true, true)) FAIL(1, "UnsupportedSwitch: gVals[8] on an image");
	MockBVH bvh;
	bvh.nodes.resize(1); bvh.tris.resize(1);
	Scene<snail::HipBVH<MockBVH>> scene;
	scene.geometry.Upload(bvh, 0);
	scene.geometry.AttachMaterials((SnailMaterials *)(uintptr_t)0x20);
	const Camera cam{1.0f, {0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
	const std::vector<int> coords = {0, 0, 16, 64}, offsets = {0};
	std::vector<unsigned char> data(3 * 16 * 64);
	MipmapTexture img; img.w = 16; img.h = 16; img.pitch = 48; img.bytes.assign(48 * 16, 0);
	const bool capable = snail::kDeviceTransparency != 0;   // whether a set that can select is the device's at all
	gVals[6] = 1; gVals[5] = 1;
	if(what == "truncated") {   // one heat call whose counter moves
		moves = 5; gVals[7] = 1; canSelect = capable ? 1 : 0;
		const TreeStats ts = Render(scene, cam, 16u, 64u, data.data(), coords, offsets, Options(), 3u, 4u);
		if(!kOptedIn) { if(hostCalls != 1 || heatTiles.n) FAIL(2, "without the macro gVals[5] under full shading is the host renderer's"); }
		else if(heatTiles.n != 1 || hostCalls != 1 || prefetched != 1 || ts.in != 77) FAIL(3, "a moved counter must reach the host renderer, whose TreeStats are returned");
		std::printf("truncated heat frame rendered again by the host renderer\n");
		return 0;
	}
	const int all = SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_AA4;
	for(int sel = 0; sel < 2; sel++) {   // a set that cannot select, then one that can
		canSelect = sel;
		const bool device = kOptedIn && (sel == 0 || capable);
		const Call t0 = heatTiles, f0 = heatFrame;
		const int h0 = hostCalls, lit0 = oldTiles.n + oldFrame.n + treeTiles.n + treeFrame.n;
		// 1. the tile list with gVals[7], [8], [9]
		gVals[7] = 1; gVals[8] = 1; gVals[9] = 1;
		TreeStats ts = Render(scene, cam, 16u, 64u, data.data(), coords, offsets, Options(), 3u, 4u);
		if(device) { if(heatTiles.n != t0.n + 1 || heatTiles.depth != 8 || heatTiles.flags != all || !heatTiles.tint || hostCalls != h0 || ts.in != 5) FAIL(4, "tile list: _heat_ with depth 8"); }
		else if(hostCalls != h0 + 1 || heatTiles.n != t0.n || ts.in != 77) FAIL(5, "tile list: today's routing");
		// 2. the image: no tint; with gVals[8] the host renderer's either way
		gVals[8] = 0;
		ts = Render(scene, cam, img, Options(), 4);
		if(device) { if(heatFrame.n != f0.n + 1 || heatFrame.depth != 8 || heatFrame.flags != all || ts.in != 6) FAIL(6, "image: _heat_ with depth 8"); }
		else if(heatFrame.n != f0.n || ts.in != 78) FAIL(7, "image: today's routing");
		const int hb = hostCalls, fb = heatFrame.n;
		gVals[8] = 1;
		ts = Render(scene, cam, img, Options(), 4);
		gVals[8] = 0;
		if(hostCalls != hb + 1 || heatFrame.n != fb) FAIL(8, "an image with gVals[8] is the host renderer's");
		if(oldTiles.n + oldFrame.n + treeTiles.n + treeFrame.n != lit0) FAIL(9, "gVals[5] without gVals[1] never reaches the lit functions");
		// 3. under gVals[1] the frame is the depth frame of the lit functions, with or without the macro
		gVals[1] = 1;
		const int hb1 = hostCalls, tb1 = heatTiles.n;
		ts = Render(scene, cam, 16u, 64u, data.data(), coords, offsets, Options(), 3u, 4u);
		gVals[1] = 0;
		if(heatTiles.n != tb1) FAIL(10, "gVals[5] under gVals[1] is not a heat-map");
		if(sel == 0 || capable) { if(hostCalls != hb1 || !((sel ? treeTiles : oldTiles).flags & SNAIL_RENDER_DEPTH)) FAIL(11, "gVals[5] under gVals[1]: the depth frame"); }
		else if(hostCalls != hb1 + 1) FAIL(12, "a set that can select without SNAIL_ADAPTER_DEVICE_TRANSPARENCY is the host renderer's");
		// 4. a moved counter: the host renderer does the frame again, its TreeStats are returned, the prefetched frame is released
		moves = 9; gVals[7] = 1;
		const int hb2 = hostCalls, tb2 = heatTiles.n, fb2 = heatFrame.n;
		ts = Render(scene, cam, 16u, 64u, data.data(), coords, offsets, Options(), 3u, 4u);
		const TreeStats is = Render(scene, cam, img, Options(), 4);
		moves = 0;
		if(device && (heatTiles.n != tb2 + 1 || heatFrame.n != fb2 + 1)) FAIL(13, "the device ran first");
		if(hostCalls != hb2 + 2 || ts.in != 77 || is.in != 78 || scene.geometry.HaveFrame()) FAIL(14, "a moved counter must reach the host renderer");
	}
	// 5. gVals[5] off: the lit functions, as ever
	gVals[5] = 0; canSelect = 0;
	const int ob = oldTiles.n, hbn = heatTiles.n;
	TreeStats ts = Render(scene, cam, 16u, 64u, data.data(), coords, offsets, Options(), 3u, 4u);
	if(oldTiles.n != ob + 1 || heatTiles.n != hbn || ts.in != 1) FAIL(15, "without gVals[5] the lit functions");
	// 6. no set: the host renderer
	gVals[5] = 1;
	scene.geometry.AttachMaterials(nullptr);
	const int hb3 = hostCalls;
	ts = Render(scene, cam, 16u, 64u, data.data(), coords, offsets, Options(), 3u, 4u);
	if(hostCalls != hb3 + 1 || heatTiles.n != hbn) FAIL(16, "without a set gVals[6] is the host renderer's");
	std::printf("materials heat adapter ok (%s SNAIL_ADAPTER_DEVICE_MATERIALS_HEATMAP, %s SNAIL_ADAPTER_DEVICE_TRANSPARENCY), host renderer reached %d times, _heat_ %d + %d times\n",
				kOptedIn ? "with" : "without", capable ? "with" : "without", hostCalls, heatTiles.n, heatFrame.n);
	return 0;
}
