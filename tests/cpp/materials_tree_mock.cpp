// The routing of the Render(...) overloads of include/snail_adapter.hpp under SNAIL_ADAPTER_DEVICE_TRANSPARENCY, against MOCK reference types (as
// tests/cpp/materials_mock.cpp) AND a mock C-ABI: the snail_* functions the overloads reach are defined here and record how they were called, so
// nothing touches a device and the program does not link libsnailhip.so.  The macros come from the compiler's command line:
//   -DSNAIL_ADAPTER_DEVICE_MATERIALS [-DSNAIL_ADAPTER_DEVICE_TRANSPARENCY] [-DSNAIL_ADAPTER_NO_HOST_RENDERER]
//   materials_tree_mock routing     a set that can select goes to the _tree_ functions with maxDepth 8 (with the macro) or to the host renderer
//                                   (without: today's routing); a moved counter goes to the host renderer, whose TreeStats are returned; a set
//                                   that cannot select goes to the older functions either way
//   materials_tree_mock truncated   one tile-list call whose counter moves: the host renderer, or abort() under SNAIL_ADAPTER_NO_HOST_RENDERER
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
static uint64_t moves = 0;   // what a _tree_ call adds to the caller's truncated-lane counter
struct Call { int n = 0, flags = -1, depth = -1; bool tint = false; };
static Call treeTiles, treeFrame, oldTiles, oldFrame;
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
// reached by the branches of the overloads that this program never takes (simple shading, the heat-map)
int snail_render_tiles(SnailScene *, const float *, int, int, const int32_t *, const int64_t *, int, const float *, int, const float *, const float *, int, uint8_t *, uint64_t *) { std::abort(); }
int snail_render_tiles_multi(SnailScene *const *, int, const float *, int, int, const int32_t *, const int64_t *, int, const float *, int, const float *, const float *, int, uint8_t *,
							 uint64_t *) { std::abort(); }
int snail_render_image(SnailScene *, const float *, int, int, const float *, int, const float *, const float *, int, uint8_t *, int, uint64_t *) { std::abort(); }
int snail_render_heat_tiles(SnailScene *, const float *, int, int, const int32_t *, const int64_t *, int, const float *, int, int, uint8_t *, uint64_t *) { std::abort(); }
int snail_render_heat_image(SnailScene *, const float *, int, int, const float *, int, int, uint8_t *, int, uint64_t *) { std::abort(); }
}

#if defined(SNAIL_ADAPTER_DEVICE_TRANSPARENCY) && defined(SNAIL_ADAPTER_DEVICE_MATERIALS)
static const bool kOptedIn = true;
#else
static const bool kOptedIn = false;
#endif
#define FAIL(code, what) do { std::printf("FAILED: %s\n", what); return code; } while(0)

int main(int argc, char **argv) {
	const std::string what = argc > 1 ? argv[1] : "routing";
	if((snail::kDeviceTransparency != 0) != kOptedIn || (int)snail::kTreeMaxDepth != (int)SNAIL_MAT_TRANSP_MAX_DEPTH) FAIL(1, "kDeviceTransparency / kTreeMaxDepth");
	MockBVH bvh;
	bvh.nodes.resize(1); bvh.tris.resize(1);
	Scene<snail::HipBVH<MockBVH>> scene;
	scene.geometry.Upload(bvh, 0);
	scene.geometry.AttachMaterials((SnailMaterials *)(uintptr_t)0x20);
	const Camera cam{1.0f, {0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
	const std::vector<int> coords = {0, 0, 16, 64}, offsets = {0};
	std::vector<unsigned char> data(3 * 16 * 64);
	MipmapTexture img; img.w = 16; img.h = 16; img.pitch = 48; img.bytes.assign(48 * 16, 0);
	gVals[6] = 1;
	if(what == "truncated") {   // one call whose counter moves
		moves = 5; gVals[7] = 1;
		const TreeStats ts = Render(scene, cam, 16u, 64u, data.data(), coords, offsets, Options(), 3u, 4u);
		if(!kOptedIn) { if(hostCalls != 1 || treeTiles.n) FAIL(2, "without the macro a capable set is the host renderer's"); }
		else if(treeTiles.n != 1 || hostCalls != 1 || prefetched != 1 || ts.in != 77) FAIL(3, "a moved counter must reach the host renderer, whose TreeStats are returned");
		std::printf("truncated frame rendered again by the host renderer\n");
		return 0;
	}
	// 1. a set that can select: the tile list with gVals[7], [8], [9]
	gVals[7] = 1; gVals[8] = 1; gVals[9] = 1;
	TreeStats ts = Render(scene, cam, 16u, 64u, data.data(), coords, offsets, Options(), 3u, 4u);
	const int all = SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_AA4;
	if(kOptedIn) {
		if(treeTiles.n != 1 || treeTiles.depth != 8 || treeTiles.flags != all || !treeTiles.tint || hostCalls || oldTiles.n || ts.in != 3) FAIL(4, "tile list: _tree_ with depth 8");
	} else if(hostCalls != 1 || treeTiles.n || oldTiles.n || ts.in != 77) FAIL(5, "tile list: today's routing");
	// 2. the image: no tint; with gVals[8] the host renderer's either way
	gVals[8] = 0;
	ts = Render(scene, cam, img, Options(), 4);
	if(kOptedIn) { if(treeFrame.n != 1 || treeFrame.depth != 8 || treeFrame.flags != all || oldFrame.n || ts.in != 4) FAIL(6, "image: _tree_ with depth 8"); }
	else if(hostCalls != 2 || treeFrame.n || ts.in != 78) FAIL(7, "image: today's routing");
	const int hostBefore = hostCalls;
	gVals[8] = 1;
	ts = Render(scene, cam, img, Options(), 4);
	gVals[8] = 0;
	if(hostCalls != hostBefore + 1 || treeFrame.n > 1) FAIL(8, "an image with gVals[8] is the host renderer's");
	// 3. gVals[1]: the depth flag is passed on; gVals[5] without gVals[1] is the host renderer's
	gVals[1] = 1; gVals[5] = 1;
	ts = Render(scene, cam, 16u, 64u, data.data(), coords, offsets, Options(), 3u, 4u);
	if(kOptedIn && (treeTiles.n != 2 || !(treeTiles.flags & SNAIL_RENDER_DEPTH))) FAIL(9, "gVals[5] under gVals[1]");
	gVals[1] = 0;
	const int hb = hostCalls, tb = treeTiles.n;
	ts = Render(scene, cam, 16u, 64u, data.data(), coords, offsets, Options(), 3u, 4u);
	gVals[5] = 0;
	if(hostCalls != hb + 1 || treeTiles.n != tb) FAIL(10, "gVals[5] without gVals[1] is the host renderer's");
	// 4. a moved counter: the host renderer does the frame again, its TreeStats are returned, the prefetched frame is released
	moves = 9;
	const int hb2 = hostCalls, tb2 = treeTiles.n, fb2 = treeFrame.n;
	ts = Render(scene, cam, 16u, 64u, data.data(), coords, offsets, Options(), 3u, 4u);
	const TreeStats is = Render(scene, cam, img, Options(), 4);
	moves = 0;
	if(kOptedIn && (treeTiles.n != tb2 + 1 || treeFrame.n != fb2 + 1)) FAIL(11, "the device ran first");
	if(hostCalls != hb2 + 2 || ts.in != 77 || is.in != 78 || scene.geometry.HaveFrame()) FAIL(12, "a moved counter must reach the host renderer");
	// 5. a set that cannot select: the older functions, with or without the new macro
	canSelect = 0;
	const int hb3 = hostCalls, tb3 = treeTiles.n, fb3 = treeFrame.n;
	ts = Render(scene, cam, 16u, 64u, data.data(), coords, offsets, Options(), 3u, 4u);
	const TreeStats is2 = Render(scene, cam, img, Options(), 4);
	if(oldTiles.n != 1 || oldFrame.n != 1 || hostCalls != hb3 || treeTiles.n != tb3 || treeFrame.n != fb3 || ts.in != 1 || is2.in != 2) FAIL(13, "a set that cannot select: the older functions");
	// 6. no set: the host renderer
	scene.geometry.AttachMaterials(nullptr);
	ts = Render(scene, cam, 16u, 64u, data.data(), coords, offsets, Options(), 3u, 4u);
	if(hostCalls != hb3 + 1) FAIL(14, "without a set gVals[6] is the host renderer's");
	std::printf("materials tree adapter ok (%s SNAIL_ADAPTER_DEVICE_TRANSPARENCY), host renderer reached %d times, _tree_ %d + %d times\n", kOptedIn ? "with" : "without", hostCalls,
				treeTiles.n, treeFrame.n);
	return 0;
}
