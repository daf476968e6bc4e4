// The routing of HipBVH::RebuildShaded (include/snail_adapter.hpp) against a MOCK reference BVH and a mock C-ABI (as
// tests/cpp/materials_tree_mock.cpp): the snail_* functions it reaches are defined here and record how they were called, so nothing touches a
// device and the program does not link libsnailhip.so.
//   with a set attached      snail_materials_rebuild_dev with the caller's vertices, normals (or null), perm, info and stream
//   without one              Rebuild = snail_scene_rebuild_fast_dev, normals unused
//   Rebuild itself           snail_scene_rebuild_fast_dev whether or not a set is attached
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct Node { float b[6]; unsigned sub; int aux; };
struct Triangle { float f[16]; };
struct ShTriangle { float f[16]; };
struct MockBVH {
	typedef Triangle CElement; typedef ShTriangle SElement;
	enum { isctFlags = 1, maxDepth = 64, fastBuild = 1 };
	std::vector<Node> nodes; std::vector<Triangle> tris; int depth = 0;
};

#include "../../include/snail_adapter.hpp"

struct Call { int n = 0; const float *verts = nullptr, *nrm = nullptr; int nTris = -1; int32_t *perm = nullptr, *info = nullptr; void *stream = nullptr; SnailMaterials *set = nullptr; };
static Call sceneRebuild, setRebuild;
static int setRc = 0;
extern "C" {
const char *snail_last_error(void) { return "mock"; }
SnailScene *snail_scene_create_fast_dev(const float *, int, int, int32_t *, int32_t *, void *) { return (SnailScene *)(uintptr_t)0x10; }
void snail_scene_destroy(SnailScene *) {}
int snail_scene_arith(const SnailScene *, int *a) { if(a) *a = SNAIL_ARITH_IEEE; return 0; }
int snail_scene_set_arith(SnailScene *, int) { return 0; }
int snail_scene_rebuild_fast_dev(SnailScene *, const float *v, int n, int32_t *perm, int32_t *info, void *stream) {
	sceneRebuild.n++; sceneRebuild.verts = v; sceneRebuild.nTris = n; sceneRebuild.perm = perm; sceneRebuild.info = info; sceneRebuild.stream = stream;
	return 0;
}
int snail_materials_rebuild_dev(SnailMaterials *m, const float *v, const float *nrm, int32_t *perm, int32_t *info, void *stream) {
	setRebuild.n++; setRebuild.set = m; setRebuild.verts = v; setRebuild.nrm = nrm; setRebuild.perm = perm; setRebuild.info = info; setRebuild.stream = stream;
	return setRc;
}
}

#define FAIL(code, what) do { std::printf("FAILED: %s\n", what); return code; } while(0)

int main() {
	snail::HipBVH<MockBVH> bvh;
	float verts[9] = {0}, nrm[9] = {0};
	int32_t perm[1] = {0}, info[6] = {0};
	void *stream = (void *)(uintptr_t)0x30;
	SnailMaterials *set = (SnailMaterials *)(uintptr_t)0x20;
	if(bvh.RebuildShaded(verts, nrm, 1) || sceneRebuild.n || setRebuild.n) FAIL(1, "no handle: false, nothing reached");
	bvh.ConstructOnDevice(verts, 1, MockBVH::fastBuild);
	// without a set: Rebuild
	if(!bvh.RebuildShaded(verts, nrm, 1, perm, info, stream) || sceneRebuild.n != 1 || setRebuild.n) FAIL(2, "without a set RebuildShaded is Rebuild");
	if(sceneRebuild.verts != verts || sceneRebuild.nTris != 1 || sceneRebuild.perm != perm || sceneRebuild.info != info || sceneRebuild.stream != stream) FAIL(3, "Rebuild's arguments");
	// with a set: the set's rebuild, normals given or null
	bvh.AttachMaterials(set);
	if(!bvh.RebuildShaded(verts, nrm, 1, perm, info, stream) || setRebuild.n != 1 || sceneRebuild.n != 1) FAIL(4, "with a set RebuildShaded is snail_materials_rebuild_dev");
	if(setRebuild.set != set || setRebuild.verts != verts || setRebuild.nrm != nrm || setRebuild.perm != perm || setRebuild.info != info || setRebuild.stream != stream) FAIL(5, "the set's arguments");
	if(!bvh.RebuildShaded(verts, nullptr, 1) || setRebuild.n != 2 || setRebuild.nrm || setRebuild.perm || setRebuild.info || setRebuild.stream) FAIL(6, "face normals and the defaults");
	setRc = 1;
	if(bvh.RebuildShaded(verts, nrm, 1) || setRebuild.n != 3) FAIL(7, "a refusal is false");
	setRc = 0;
	// Rebuild itself is unchanged: the scene's, set or no set
	if(!bvh.Rebuild(verts, 1, perm, info, stream) || sceneRebuild.n != 2 || setRebuild.n != 3) FAIL(8, "Rebuild stays snail_scene_rebuild_fast_dev");
	bvh.AttachMaterials(nullptr);
	if(!bvh.RebuildShaded(verts, nullptr, 1) || sceneRebuild.n != 3 || setRebuild.n != 3) FAIL(9, "detached: Rebuild again");
	std::printf("materials dynamic adapter ok: scene rebuilds %d, set rebuilds %d\n", sceneRebuild.n, setRebuild.n);
	return 0;
}
