// Compile-and-run check of the Render(...) overloads of include/snail_adapter.hpp for Scene<snail::HipDBVH<...>> with
// SNAIL_ADAPTER_INSTANCED_TILES defined, against MOCK types with the reference's member names (as tests/cpp/instances_shade_mock.cpp): the tile
// list with gVals[9], with gVals[9] + gVals[8] (rank 3) and with gVals[1], and the image with gVals[9], are made on the device
// (snail_instances_render_tiles / snail_instances_render_frame); the reference's own renderer -- a stub here -- is reached with gVals[5] alone,
// and then with a prefetched frame.
//   instances_tiles_mock <dir>
// reads the scene, camera, lights and tiles from <dir> (written by tests/test_gpu_instances_tiles.py::test_cpp_adapter_tile_list) and writes
//   out_aa.bin, out_tint.bin, out_depth.bin   the tile buffers (tiles back to back, 0xAB in a 5-byte gap after each)
//   out_img_aa.bin                            the antialiased image (pitch = 3 * resx + 1)
//   stats.txt                                 the TreeStats each Render returned
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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
	bool HasShadingData() const { return false; }
	const ShTriangle &GetSElement(int e, int) const { return shTris[e]; }
	Vec3f GetNormal(int e, int) const { return Vec3f{tris[e].f[12], tris[e].f[13], tris[e].f[14]}; }
	int GetMaterialId(int, int) const { return 0; }
	BBox GetBBox() const { return BBox{{nodes[0].b[0], nodes[0].b[1], nodes[0].b[2]}, {nodes[0].b[3], nodes[0].b[4], nodes[0].b[5]}}; }
};
struct ObjectInstance {       // src/dbvh/tree.h:7-188
	Vec3f rotation[3];
	Vec3f translation;
	const MockBVH *tree;
	BBox bbox;
};
struct MockDBVH {             // src/dbvh/tree.h:97-150
	typedef ObjectInstance CElement; typedef ShTriangle SElement;
	enum { isComplex = 1 };
	enum { isctFlags = 7 };
	enum { maxDepth = 64 };
	bool HasShadingData() const { return false; }
	ShTriangle GetSElement(int elem, int sub) const { return elements[elem].tree->GetSElement(sub, 0); }
	Vec3f GetNormal(int elem, int sub) const { return elements[elem].tree->GetNormal(sub, 0); }
	int GetMaterialId(int idx, int elem) const { return elements[elem].tree->GetMaterialId(idx, 0); }
	BBox GetBBox() const { return BBox{{nodes[0].b[0], nodes[0].b[1], nodes[0].b[2]}, {nodes[0].b[3], nodes[0].b[4], nodes[0].b[5]}}; }
	vector<ObjectInstance> elements;
	std::vector<Node> nodes;
};
template <class AccStruct> struct Scene {
	AccStruct geometry;
	Vec3f ambientLight{0.1f, 0.1f, 0.1f};
	vector<Light> lights;
};
// the reference's generic Render templates (src/render.h:16-23): reached with gVals[5] alone, and then with a prefetched frame
static int hostTileCalls = 0, hostTilePrefetched = 0;
template <class AccStruct>
TreeStats Render(const Scene<AccStruct> &scene, const Camera &, uint, uint, unsigned char *, const vector<int> &, const vector<int> &, const Options, uint, uint) {
	if(!gVals[5]) { std::puts("host tile Render called"); std::exit(3); }
	hostTileCalls++;
	hostTilePrefetched += scene.geometry.HaveFrame() ? 1 : 0;
	return TreeStats();
}
template <class AccStruct> TreeStats Render(const Scene<AccStruct> &, const Camera &, MipmapTexture &, const Options, uint) {
	std::puts("generic image Render called");
	std::exit(3);
}

#define SNAIL_ADAPTER_RENDER_OVERLOADS
#define SNAIL_ADAPTER_INSTANCED_TILES
#include "../../include/snail_adapter.hpp"

template <class T> static std::vector<T> slurp(const std::string &path) {
	FILE *f = std::fopen(path.c_str(), "rb");
	if(!f) { std::perror(path.c_str()); std::exit(2); }
	std::fseek(f, 0, SEEK_END); long n = std::ftell(f); std::fseek(f, 0, SEEK_SET);
	std::vector<T> v(n / sizeof(T)); if(n && std::fread(v.data(), 1, n, f) != (size_t)n) std::exit(2); std::fclose(f); return v;
}
template <class T> static void dump(FILE *f, const T *p, size_t n) { std::fwrite(p, sizeof(T), n, f); }

int main(int argc, char **argv) {
	if(argc < 2) { std::puts("compiled and linked"); return 0; }
	const std::string d = std::string(argv[1]) + "/";
	const std::vector<int> meta = slurp<int>(d + "meta.bin");   // resx, resy, hostSse, nBlas, depth0, depth1, ...
	const int resx = meta[0], resy = meta[1], nBlas = meta[3];
	std::vector<MockBVH> blas(nBlas);
	for(int b = 0; b < nBlas; b++) {
		blas[b].nodes = slurp<Node>(d + "blas" + std::to_string(b) + "_nodes.bin");
		blas[b].tris = slurp<Triangle>(d + "blas" + std::to_string(b) + "_tris.bin");
		blas[b].depth = meta[4 + b];
	}
	MockDBVH dbvh;
	dbvh.nodes = slurp<Node>(d + "top_nodes.bin");
	const std::vector<float> xf = slurp<float>(d + "xf12.bin");
	const std::vector<int> bi = slurp<int>(d + "blas_index.bin");
	for(size_t i = 0; i < bi.size(); i++) {
		ObjectInstance e;
		for(int r = 0; r < 3; r++) e.rotation[r] = Vec3f{xf[i * 12 + r * 3], xf[i * 12 + r * 3 + 1], xf[i * 12 + r * 3 + 2]};
		e.translation = Vec3f{xf[i * 12 + 9], xf[i * 12 + 10], xf[i * 12 + 11]};
		e.tree = &blas[bi[i]];
		dbvh.elements.push_back(e);
	}
	const std::vector<float> c = slurp<float>(d + "cam.bin");
	const Camera cam{c[12], {c[0], c[1], c[2]}, {c[3], c[4], c[5]}, {c[6], c[7], c[8]}, {c[9], c[10], c[11]}};
	Scene<snail::HipDBVH<MockDBVH>> scene;
	const std::vector<float> l7 = slurp<float>(d + "lights7.bin");
	for(size_t i = 0; i + 6 < l7.size(); i += 7) {
		const float r = l7[i + 6];
		scene.lights.push_back(Light{{l7[i], l7[i + 1], l7[i + 2]}, {l7[i + 3], l7[i + 4], l7[i + 5]}, r, r * r, 1.0f / r});
	}
	snail::HipDBVH<MockDBVH> &acc = scene.geometry;
	acc.Upload(dbvh, 0);
	if(meta[2] && !acc.SetArith(SNAIL_ARITH_HOST_SSE)) { std::fprintf(stderr, "SetArith(HOST_SSE): %s\n", snail_last_error()); return 3; }
	const std::vector<int> coords = slurp<int>(d + "tiles.bin");
	const int nTiles = (int)coords.size() / 4, gap = 5;
	std::vector<int> offsets;
	size_t total = 0;
	for(int k = 0; k < nTiles; k++) { offsets.push_back((int)total); total += (size_t)3 * coords[k * 4 + 2] * coords[k * 4 + 3] + gap; }
	FILE *fs = std::fopen((d + "stats.txt").c_str(), "w");
	struct Run { const char *key, *file; int depth, aa, tint; };
	const Run runs[3] = {{"aa", "out_aa.bin", 0, 1, 0}, {"tint", "out_tint.bin", 0, 1, 1}, {"depth", "out_depth.bin", 1, 0, 0}};
	for(const Run &r : runs) {
		gVals[1] = r.depth; gVals[9] = r.aa; gVals[8] = r.tint; gVals[7] = 0; gVals[5] = 0;
		std::vector<unsigned char> data(total, 0xAB);
		const TreeStats st = Render(scene, cam, (uint)resx, (uint)resy, data.data(), coords, offsets, Options(), 3u, 4u);
		if(acc.HaveFrame()) { std::puts("a prefetched frame was left behind"); return 5; }
		FILE *f = std::fopen((d + r.file).c_str(), "wb");
		dump(f, data.data(), data.size());
		std::fclose(f);
		std::fprintf(fs, "%s %u %u %u %u\n", r.key, st.in, st.it, st.rays, st.sk);
	}
	{ // gVals[5]: the reference's renderer, over a prefetched frame
		gVals[1] = gVals[9] = gVals[8] = 0; gVals[5] = 1;
		std::vector<unsigned char> data(total, 0xAB);
		(void)Render(scene, cam, (uint)resx, (uint)resy, data.data(), coords, offsets, Options(), 3u, 4u);
		gVals[5] = 0;
		if(hostTileCalls != 1 || hostTilePrefetched != 1 || acc.HaveFrame()) { std::printf("gVals[5]: host calls %d, prefetched %d\n", hostTileCalls, hostTilePrefetched); return 6; }
	}
	{ // the image with gVals[9]
		gVals[9] = 1;
		MipmapTexture img; img.w = resx; img.h = resy; img.pitch = resx * 3 + 1; img.bytes.assign((size_t)img.pitch * resy, 0xAB);
		const TreeStats st = Render(scene, cam, img, Options(), 4);
		gVals[9] = 0;
		FILE *f = std::fopen((d + "out_img_aa.bin").c_str(), "wb");
		dump(f, img.bytes.data(), img.bytes.size());
		std::fclose(f);
		std::fprintf(fs, "img_aa %u %u %u %u\n", st.in, st.it, st.rays, st.sk);
	}
	std::fclose(fs);
	if(snail::detail::RankTint(31)[1] != 1.7f || snail::detail::RankTint(3)[0] != 0.6f) return 7;
	std::puts("instances tiles adapter ok");
	return 0;
}
