/* The fast builder's C-ABI (include/snail_bvh_fast.h) as PLAIN C (gcc -std=c99 -Wall -Werror -pedantic): the three functions link against
 * libsnailhip.so with the header's signatures, the host builder runs from a C host, and the argument checks of the device entry points that
 * need no GPU answer (tests/test_bvh_fast_host.py). */
#include <stdio.h>
#include <string.h>

#include "../../include/snail_bvh_fast.h"

#define ADDR(f) (void (*)(void))f,

int main(void) {
	void (*fns[])(void) = {
		ADDR(snail_bvh_build_fast) ADDR(snail_scene_create_fast_dev) ADDR(snail_scene_rebuild_fast_dev)
	};
	/* the header's signatures, taken as typed pointers: a mismatch does not compile under -Werror */
	int (*build)(void *, int, void *, int *, int *, int32_t *) = snail_bvh_build_fast;
	SnailScene *(*create)(const float *, int, int, int32_t *, int32_t *, void *) = snail_scene_create_fast_dev;
	int (*rebuild)(SnailScene *, const float *, int, int32_t *, int32_t *, void *) = snail_scene_rebuild_fast_dev;
	/* six triangles along x: more than a leaf holds, so the root is split */
	float verts[6 * 9];
	float tris[6 * 16], nodes[2 * 6 * 8];
	int32_t perm[6], info[4] = {7, 7, 7, 7};
	int nNodes = 0, depth = 0, i, k;
	for(i = 0; i < 6; i++) {
		const float x = (float)(5 - i);
		const float t[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0};
		for(k = 0; k < 9; k++) verts[i * 9 + k] = t[k] + (k % 3 == 0 ? 2.0f * x : 0.0f);
	}
	if(snail_tris_from_verts(verts, 6, tris) != 0) return 2;
	if(build(tris, 6, nodes, &nNodes, &depth, perm) != 0) return 3;
	if(nNodes != 3 || depth != 1) return 4;
	for(i = 0; i < 6; i++) if(perm[i] < 0 || perm[i] > 5) return 5;
	if(build(NULL, 6, nodes, &nNodes, &depth, perm) == 0 || !strstr(snail_last_error(), "snail_bvh_build_fast")) return 6;
	/* refused before anything touches a device, with a text; nothing is written.  (verts stands in for a device pointer: it is never read) */
	if(create(NULL, 6, 0, perm, info, NULL) != NULL || !strstr(snail_last_error(), "snail_scene_create_fast_dev")) return 7;
	if(create(verts, 0, 0, perm, info, NULL) != NULL) return 8;
	if(rebuild(NULL, verts, 6, perm, info, NULL) == 0 || !strstr(snail_last_error(), "snail_scene_rebuild_fast_dev")) return 9;
	if(info[0] != 7 || info[3] != 7) return 10;
	printf("C bvh fast ABI ok: %d symbols\n", (int)(sizeof(fns) / sizeof(fns[0])));
	return 0;
}
