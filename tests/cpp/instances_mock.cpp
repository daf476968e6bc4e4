// Compile-and-run check of snail::HipDBVH (include/snail_adapter.hpp) against MOCK types with the member names of the reference's
// DBVH / ObjectInstance / BVH / Scene / Context / ShadowContext / Camera / TreeStats / Options / MipmapTexture (src/dbvh/tree.h, src/bvh/tree.h,
// src/scene.h, src/ray_group.h, src/camera.h, src/tree_stats.h, src/render.h).  A test of the adapter templates, not a build of the reference.
//   instances_mock <dir>
// reads its inputs from <dir> (written by tests/test_gpu_instances.py::test_cpp_adapter_instanced) and writes, for the Python side to
// compare with tests/dbvh_ref.py:
//   out_primary.bin  t, u, v, instance, triId per pixel of a frame through HipDBVH::BeginFrame + per-packet TraversePrimary(Context<1,0>) copies
//   out_image.bin    Render(scene, camera, image, options, threads) with gVals[1]: the depth image made on the device
//   out_ry.bin       the generic packets through HipDBVH::TraversePrimary(Context<0,1>) (immediate path): distance, object, element, barycentric
//   out_sh.bin       the shadow packets through HipDBVH::TraverseShadow (immediate path): distance
//   stats.txt        the TreeStats each of them returned / accumulated
// and checks that the tile-list Render(...) reaches the reference's renderer with the frame prefetched.
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
	std::printf("host tile Render: prefetched %d x %d %d\n", scene.geometry.Frame().resx, scene.geometry.Frame().resy, (int)scene.geometry.HaveFrame());
	TreeStats st; st.it = 777; return st;
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
	const std::vector<int> meta = slurp<int>(d + "meta.bin");   // resx, resy, hostSse, nBlas, nRy, nSh, depth0, depth1, ...
	const int resx = meta[0], resy = meta[1], nBlas = meta[3], nRy = meta[4], nSh = meta[5];
	std::vector<MockBVH> blas(nBlas);
	for(int b = 0; b < nBlas; b++) {
		blas[b].nodes = slurp<Node>(d + "blas" + std::to_string(b) + "_nodes.bin");
		blas[b].tris = slurp<Triangle>(d + "blas" + std::to_string(b) + "_tris.bin");
		blas[b].depth = meta[6 + b];
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
	snail::HipDBVH<MockDBVH> &acc = scene.geometry;
	acc.Upload(dbvh, 0);
	if(acc.BlasCount() != nBlas) { std::fprintf(stderr, "%d BLAS handles for %d trees\n", acc.BlasCount(), nBlas); return 4; }
	if(meta[2] && !acc.SetArith(SNAIL_ARITH_HOST_SSE)) { std::fprintf(stderr, "SetArith(HOST_SSE): %s\n", snail_last_error()); return 3; }
	FILE *fs = std::fopen((d + "stats.txt").c_str(), "w");

	{ // ---- prefetched primary path ----
		acc.BeginFrame(cam, resx, resy);
		const size_t np = (size_t)resx * resy;
		std::vector<float> t(np), u(np), v(np);
		std::vector<int> inst(np), tri(np);
		Vec3q origin; for(int l = 0; l < 4; l++) { origin.x[l] = cam.pos.x; origin.y[l] = cam.pos.y; origin.z[l] = cam.pos.z; }
		TreeStats total;
		for(int y = 0; y < resy; y += 16) for(int x = 0; x < resx; x += 16) {
			floatq dist[64]; i32x4 obj[64], elem[64]; Vec2q bary[64]; TreeStats st;
			Context<1, 0> ctx{RayGroup<1, 0>{&origin, nullptr, nullptr, 64, nullptr}, dist, obj, elem, bary, &st};
			acc.SetPacket(x, y);
			acc.TraversePrimary(ctx);
			total.in += st.in; total.it += st.it; total.sk += st.sk;
			for(int q = 0; q < 64; q++) for(int l = 0; l < 4; l++) {
				const int px = x + (q & 3) * 4 + l, py = y + (q >> 2);
				if(px < resx && py < resy) {
					const size_t o = (size_t)py * resx + px;
					t[o] = dist[q].v[l]; u[o] = bary[q].x[l]; v[o] = bary[q].y[l]; inst[o] = obj[q].v[l]; tri[o] = elem[q].v[l];
				}
			}
		}
		acc.EndFrame();
		FILE *f = std::fopen((d + "out_primary.bin").c_str(), "wb");
		dump(f, t.data(), np); dump(f, u.data(), np); dump(f, v.data(), np); dump(f, inst.data(), np); dump(f, tri.data(), np);
		std::fclose(f);
		std::fprintf(fs, "primary %u %u %u\n", total.in, total.it, total.sk);
	}
	{ // ---- Render(scene, camera, image, options, threads), gVals[1]: on the device ----
		gVals[1] = 1;
		MipmapTexture img; img.w = resx; img.h = resy; img.pitch = resx * 3; img.bytes.assign((size_t)img.pitch * resy, 0);
		const TreeStats st = Render(scene, cam, img, Options(), 4);
		FILE *f = std::fopen((d + "out_image.bin").c_str(), "wb");
		dump(f, img.bytes.data(), img.bytes.size());
		std::fclose(f);
		std::fprintf(fs, "image %u %u %u %u\n", st.in, st.it, st.rays, st.sk);
		// the tile list: the reference's renderer over the prefetched frame
		std::vector<int> coords = {0, 0, 16, 64}, offsets = {0};
		std::vector<unsigned char> data(3 * 16 * 64);
		const TreeStats ts = Render(scene, cam, (uint)resx, (uint)resy, data.data(), coords, offsets, Options(), 0, 1);
		if(ts.it != 777 || acc.HaveFrame()) { std::puts("tile Render did not reach the host renderer"); return 5; }
		gVals[1] = 0;
	}
	{ // ---- immediate generic packets RayGroup<0,1> ----
		const std::vector<float> o = slurp<float>(d + "ry_origin.bin"), dir = slurp<float>(d + "ry_dir.bin"), idir = slurp<float>(d + "ry_idir.bin");
		std::vector<char> mask = slurp<char>(d + "ry_mask.bin");
		std::vector<float> dist = slurp<float>(d + "ry_dist.bin");
		std::vector<int> obj((size_t)nRy * 256, 0), elem((size_t)nRy * 256, 0);
		std::vector<float> bary((size_t)nRy * 512, 0.0f);
		TreeStats total;
		for(int p = 0; p < nRy; p++) {
			TreeStats st;
			Context<0, 1> ctx{RayGroup<0, 1>{(const Vec3q *)&o[(size_t)p * 768], (const Vec3q *)&dir[(size_t)p * 768], (const Vec3q *)&idir[(size_t)p * 768], 64,
											 &mask[(size_t)p * 64]},
							  (floatq *)&dist[(size_t)p * 256], (i32x4 *)&obj[(size_t)p * 256], (i32x4 *)&elem[(size_t)p * 256], (Vec2q *)&bary[(size_t)p * 512], &st};
			acc.TraversePrimary(ctx);
			total.in += st.in; total.it += st.it; total.sk += st.sk;
		}
		FILE *f = std::fopen((d + "out_ry.bin").c_str(), "wb");
		dump(f, dist.data(), dist.size()); dump(f, obj.data(), obj.size()); dump(f, elem.data(), elem.size()); dump(f, bary.data(), bary.size());
		std::fclose(f);
		std::fprintf(fs, "rays %u %u %u\n", total.in, total.it, total.sk);
	}
	{ // ---- immediate shadow packets ----
		const std::vector<float> o = slurp<float>(d + "sh_origin.bin"), dir = slurp<float>(d + "sh_dir.bin"), idir = slurp<float>(d + "sh_idir.bin");
		std::vector<float> dist = slurp<float>(d + "sh_dist.bin");
		TreeStats total;
		for(int p = 0; p < nSh; p++) {
			Vec3q org; for(int l = 0; l < 4; l++) { org.x[l] = o[p * 3]; org.y[l] = o[p * 3 + 1]; org.z[l] = o[p * 3 + 2]; }
			TreeStats st;
			ShadowContext ctx{RayGroup<1, 0>{&org, (const Vec3q *)&dir[(size_t)p * 768], (const Vec3q *)&idir[(size_t)p * 768], 64, nullptr},
							  (floatq *)&dist[(size_t)p * 256], &st};
			acc.TraverseShadow(ctx);
			total.in += st.in; total.it += st.it; total.sk += st.sk;
		}
		FILE *f = std::fopen((d + "out_sh.bin").c_str(), "wb");
		dump(f, dist.data(), dist.size());
		std::fclose(f);
		std::fprintf(fs, "shadow %u %u %u\n", total.in, total.it, total.sk);
	}
	std::fclose(fs);
	std::puts("instances adapter ok");
	return 0;
}
