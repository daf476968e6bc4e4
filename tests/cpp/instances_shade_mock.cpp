// Compile-and-run check of the image Render(...) overload of include/snail_adapter.hpp for Scene<snail::HipDBVH<...>> against MOCK types with the
// reference's member names (as tests/cpp/instances_mock.cpp): a frame with gVals[1] == 0 -- lit by the scene's lights, then with gVals[7] --
// is made on the device (snail_instances_render_image); the reference's own renderer, a stub here that exits with status 3, is NOT reached.
//   instances_shade_mock <dir>
// reads the scene, camera and lights from <dir> (written by tests/test_gpu_instances_shade.py::test_cpp_adapter_lit_image) and writes
//   out_lit.bin, out_refl.bin   the two images (pitch = 3 * resx + 1: the byte-wise store)
//   stats.txt                   the TreeStats each Render returned
#include <cstdint>
#include <cstdio>
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
// the reference's generic Render templates (src/render.h:16-23): the tile list of an instanced scene must arrive here, prefetched
template <class AccStruct>
TreeStats Render(const Scene<AccStruct> &scene, const Camera &, uint, uint, unsigned char *, const vector<int> &, const vector<int> &, const Options, uint, uint) {
	(void)scene;
	std::puts("host tile Render called");
	std::exit(3);
}
template <class AccStruct> TreeStats Render(const Scene<AccStruct> &, const Camera &, MipmapTexture &, const Options, uint) {
	std::puts("generic image Render called");
	std::exit(3);
}

#define SNAIL_ADAPTER_RENDER_OVERLOADS
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
	FILE *fs = std::fopen((d + "stats.txt").c_str(), "w");
	for(int refl = 0; refl < 2; refl++) {   // gVals[1] = 0; then gVals[7] = 1
		gVals[1] = 0; gVals[7] = refl;
		MipmapTexture img; img.w = resx; img.h = resy; img.pitch = resx * 3 + 1; img.bytes.assign((size_t)img.pitch * resy, 0xAB);
		const TreeStats st = Render(scene, cam, img, Options(), 4);
		if(acc.HaveFrame()) { std::puts("a prefetched frame was left behind"); return 5; }
		FILE *f = std::fopen((d + (refl ? "out_refl.bin" : "out_lit.bin")).c_str(), "wb");
		dump(f, img.bytes.data(), img.bytes.size());
		std::fclose(f);
		std::fprintf(fs, "%s %u %u %u %u\n", refl ? "refl" : "lit", st.in, st.it, st.rays, st.sk);
	}
	std::fclose(fs);
	std::puts("instances shade adapter ok");
	return 0;
}
