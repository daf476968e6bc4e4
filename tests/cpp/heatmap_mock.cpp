// Compile-and-run check of the Render(...) overloads of include/snail_adapter.hpp with SNAIL_ADAPTER_DEVICE_HEATMAP (and
// SNAIL_ADAPTER_INSTANCED_TILES) defined, against MOCK types with the reference's member names (as tests/cpp/instances_tiles_mock.cpp): with
// gVals[5] the tile list and the image of a plain scene (Scene<HipBVH>) and of an instanced scene (Scene<HipDBVH>) are made on the device -- the
// bytes and TreeStats of the C-ABI heat calls of include/snail_heatmap.h, compared here -- and the reference's own renderer, a stub, is never
// reached; gVals[5] with gVals[1] gives the depth frame; gVals[6] on a scene with shading data still reaches the stub.
//   heatmap_mock <dir>
// reads the scene, camera, lights and tiles from <dir> (the files of tests/test_gpu_instances_tiles.py::test_cpp_adapter_tile_list; the plain scene
// is BLAS 0) and writes out_plain_tiles.bin / out_inst_tiles.bin, the gVals[5] tile buffers (tiles back to back), for the caller to hold against
// the Python bindings.
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
	bool shading = false;   // (the mock's stand-in for a scene loaded with materials)
	bool HasShadingData() const { return shading; }
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
// the reference's generic Render templates (src/render.h:16-23): the host renderer.  Reached only where the test says so (gVals[6]).
static int hostCalls = 0;
template <class AccStruct>
TreeStats Render(const Scene<AccStruct> &, const Camera &, uint, uint, unsigned char *, const vector<int> &, const vector<int> &, const Options, uint, uint) {
	if(!gVals[6]) { std::puts("host tile Render called"); std::exit(3); }
	hostCalls++;
	return TreeStats();
}
template <class AccStruct> TreeStats Render(const Scene<AccStruct> &, const Camera &, MipmapTexture &, const Options, uint) {
	if(!gVals[6]) { std::puts("host image Render called"); std::exit(3); }
	hostCalls++;
	return TreeStats();
}

#define SNAIL_ADAPTER_RENDER_OVERLOADS
#define SNAIL_ADAPTER_INSTANCED_TILES
#define SNAIL_ADAPTER_DEVICE_HEATMAP
#include "../../include/snail_adapter.hpp"

template <class T> static std::vector<T> slurp(const std::string &path) {
	FILE *f = std::fopen(path.c_str(), "rb");
	if(!f) { std::perror(path.c_str()); std::exit(2); }
	std::fseek(f, 0, SEEK_END); long n = std::ftell(f); std::fseek(f, 0, SEEK_SET);
	std::vector<T> v(n / sizeof(T)); if(n && std::fread(v.data(), 1, n, f) != (size_t)n) std::exit(2); std::fclose(f); return v;
}
template <class T> static void dump(FILE *f, const T *p, size_t n) { std::fwrite(p, sizeof(T), n, f); }

static bool same(const TreeStats &a, const uint64_t (&st)[4]) { return a.in == st[0] && a.it == st[1] && a.rays == st[2] && a.sk == st[3]; }
#define FAIL(code, what) do { std::printf("FAILED: %s\n", what); return code; } while(0)

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
	const std::vector<float> c = slurp<float>(d + "cam.bin"), pc = slurp<float>(d + "plain_cam.bin");
	const Camera cam{c[12], {c[0], c[1], c[2]}, {c[3], c[4], c[5]}, {c[6], c[7], c[8]}, {c[9], c[10], c[11]}};
	const Camera pcam{pc[12], {pc[0], pc[1], pc[2]}, {pc[3], pc[4], pc[5]}, {pc[6], pc[7], pc[8]}, {pc[9], pc[10], pc[11]}};
	Scene<snail::HipDBVH<MockDBVH>> iscene;
	Scene<snail::HipBVH<MockBVH>> pscene;
	const std::vector<float> l7 = slurp<float>(d + "lights7.bin"), pl7 = slurp<float>(d + "plain_lights7.bin");
	for(size_t i = 0; i + 6 < l7.size(); i += 7) iscene.lights.push_back(Light{{l7[i], l7[i + 1], l7[i + 2]}, {l7[i + 3], l7[i + 4], l7[i + 5]}, l7[i + 6], l7[i + 6] * l7[i + 6], 1.0f / l7[i + 6]});
	for(size_t i = 0; i + 6 < pl7.size(); i += 7) pscene.lights.push_back(Light{{pl7[i], pl7[i + 1], pl7[i + 2]}, {pl7[i + 3], pl7[i + 4], pl7[i + 5]}, pl7[i + 6], pl7[i + 6] * pl7[i + 6], 1.0f / pl7[i + 6]});
	iscene.geometry.Upload(dbvh, 0);
	pscene.geometry.Upload(blas[0], 0);
	if(meta[2] && (!iscene.geometry.SetArith(SNAIL_ARITH_HOST_SSE) || !pscene.geometry.SetArith(SNAIL_ARITH_HOST_SSE))) { std::fprintf(stderr, "SetArith(HOST_SSE): %s\n", snail_last_error()); return 3; }
	const std::vector<int> coords = slurp<int>(d + "tiles.bin");
	const int nTiles = (int)coords.size() / 4;
	std::vector<int> offsets;
	std::vector<int64_t> off64;
	size_t total = 0;
	for(int k = 0; k < nTiles; k++) { offsets.push_back((int)total); off64.push_back((int64_t)total); total += (size_t)3 * coords[k * 4 + 2] * coords[k * 4 + 3]; }
	float ic[13], pcc[13];
	snail::detail::cam13(cam, ic); snail::detail::cam13(pcam, pcc);
	const int pitch = resx * 3 + 1;
	for(int refl = 0; refl < 2; refl++)
		for(int aa = 0; aa < 2; aa++) {
			const int flags = (refl ? SNAIL_RENDER_REFLECTIONS : 0) | (aa ? SNAIL_RENDER_AA4 : 0);
			gVals[5] = 1; gVals[7] = refl; gVals[9] = aa; gVals[1] = 0; gVals[8] = 0; gVals[6] = 0;
			uint64_t st[4] = {0, 0, 0, 0};
			// plain scene: tile list and image
			std::vector<unsigned char> a(total, 0xAB), b(total, 0xCD);
			TreeStats ts = Render(pscene, pcam, (uint)resx, (uint)resy, a.data(), coords, offsets, Options(), 3u, 4u);
			if(snail_render_heat_tiles(pscene.geometry.Handle(), pcc, resx, resy, coords.data(), off64.data(), nTiles, pl7.data(), (int)(pl7.size() / 7), flags, b.data(), st)) FAIL(4, snail_last_error());
			if(a != b || !same(ts, st)) FAIL(5, "plain tile list: not the bytes / stats of snail_render_heat_tiles");
			if(!refl && !aa) { FILE *f = std::fopen((d + "out_plain_tiles.bin").c_str(), "wb"); dump(f, a.data(), a.size()); std::fclose(f); }
			MipmapTexture img; img.w = resx; img.h = resy; img.pitch = pitch; img.bytes.assign((size_t)pitch * resy, 0xAB);
			std::vector<unsigned char> ref((size_t)pitch * resy, 0xAB);
			ts = Render(pscene, pcam, img, Options(), 4);
			uint64_t st2[4] = {0, 0, 0, 0};
			if(snail_render_heat_image(pscene.geometry.Handle(), pcc, resx, resy, pl7.data(), (int)(pl7.size() / 7), flags, ref.data(), pitch, st2)) FAIL(4, snail_last_error());
			if(img.bytes != ref || !same(ts, st2)) FAIL(6, "plain image: not the bytes / stats of snail_render_heat_image");
			// instanced scene: tile list (with the rank tint when gVals[8] is set) and image
			for(int tint = 0; tint < 2; tint++) {
				gVals[8] = tint;
				std::vector<unsigned char> ia(total, 0xAB), ib(total, 0xCD);
				uint64_t st3[4] = {0, 0, 0, 0};
				ts = Render(iscene, cam, (uint)resx, (uint)resy, ia.data(), coords, offsets, Options(), 3u, 4u);
				if(snail_instances_render_heat_tiles(iscene.geometry.Handle(), ic, resx, resy, coords.data(), off64.data(), nTiles, l7.data(), (int)(l7.size() / 7), flags,
													 tint ? snail::detail::RankTint(3) : nullptr, ib.data(), st3))
					FAIL(4, snail_last_error());
				if(ia != ib || !same(ts, st3)) FAIL(7, "instanced tile list: not the bytes / stats of snail_instances_render_heat_tiles");
				if(!refl && !aa && !tint) { FILE *f = std::fopen((d + "out_inst_tiles.bin").c_str(), "wb"); dump(f, ia.data(), ia.size()); std::fclose(f); }
			}
			gVals[8] = 0;
			img.bytes.assign((size_t)pitch * resy, 0xAB); ref.assign((size_t)pitch * resy, 0xAB);
			ts = Render(iscene, cam, img, Options(), 4);
			uint64_t st4[4] = {0, 0, 0, 0};
			if(snail_instances_render_heat_frame(iscene.geometry.Handle(), ic, resx, resy, l7.data(), (int)(l7.size() / 7), flags, ref.data(), pitch, st4)) FAIL(4, snail_last_error());
			if(img.bytes != ref || !same(ts, st4)) FAIL(8, "instanced image: not the bytes / stats of snail_instances_render_heat_frame");
			if(pscene.geometry.HaveFrame() || iscene.geometry.HaveFrame()) FAIL(9, "a prefetched frame was left behind");
		}
	{ // gVals[5] with gVals[1]: the depth frame, as without gVals[5]
		gVals[7] = gVals[9] = gVals[8] = 0; gVals[1] = 1;
		std::vector<unsigned char> a(total, 0xAB), b(total, 0xAB), ia(total, 0xAB), ib(total, 0xAB);
		gVals[5] = 1;
		(void)Render(pscene, pcam, (uint)resx, (uint)resy, a.data(), coords, offsets, Options(), 3u, 4u);
		(void)Render(iscene, cam, (uint)resx, (uint)resy, ia.data(), coords, offsets, Options(), 3u, 4u);
		gVals[5] = 0;
		(void)Render(pscene, pcam, (uint)resx, (uint)resy, b.data(), coords, offsets, Options(), 3u, 4u);
		(void)Render(iscene, cam, (uint)resx, (uint)resy, ib.data(), coords, offsets, Options(), 3u, 4u);
		if(a != b || ia != ib) FAIL(10, "gVals[5] + gVals[1]: not the depth frame");
		gVals[1] = 0;
	}
	{ // gVals[6] on a scene with shading data: still the reference's renderer, with or without gVals[5]
		blas[0].shading = true;
		std::vector<unsigned char> a(total, 0xAB);
		MipmapTexture img; img.w = resx; img.h = resy; img.pitch = pitch; img.bytes.assign((size_t)pitch * resy, 0xAB);
		gVals[6] = 1; gVals[5] = 1;
		(void)Render(pscene, pcam, (uint)resx, (uint)resy, a.data(), coords, offsets, Options(), 3u, 4u);
		(void)Render(pscene, pcam, img, Options(), 4);
		gVals[5] = 0;
		(void)Render(pscene, pcam, (uint)resx, (uint)resy, a.data(), coords, offsets, Options(), 3u, 4u);
		gVals[6] = 0;
		blas[0].shading = false;
		if(hostCalls != 3 || pscene.geometry.HaveFrame()) FAIL(11, "gVals[6] with shading data did not reach the host renderer three times");
		for(unsigned char v : a) if(v != 0xAB) FAIL(12, "the stub's buffer was written");
	}
	std::puts("heatmap adapter ok");
	return 0;
}
