/* The device top-level builder of instanced scenes (include/snail_instances_build.h, reached through include/snail_instances.h) as PLAIN C
 * (gcc -std=c99 -Wall -Werror -pedantic): both functions link against libsnailhip.so with the header's signatures, and the argument checks
 * that need no GPU answer from a C host (tests/test_instances_rebuild_abi.py). */
#include <stdio.h>
#include <string.h>

#include "../../include/snail_instances.h"

#define ADDR(f) (void (*)(void))f,

int main(void) {
	void (*fns[])(void) = {
		ADDR(snail_instances_rebuild_dev) ADDR(snail_instances_read_tree)
	};
	/* the header's signatures, taken as typed pointers: a mismatch does not compile under -Werror */
	int (*rebuild)(SnailInstances *, const float *, const int32_t *, int, int32_t *, int32_t *, void *) = snail_instances_rebuild_dev;
	int (*read_tree)(SnailInstances *, void *, int, int *, float *, int32_t *, int, int *) = snail_instances_read_tree;
	float xf[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
	int32_t perm[1] = {7}, info[4] = {7, 7, 7, 7};
	int nNodes = 7, n = 7;
	/* refused before anything touches a device, with a text; nothing is written.  (xf stands in for a device pointer: it is never read) */
	if(rebuild(NULL, xf, NULL, 1, perm, info, NULL) == 0 || !strstr(snail_last_error(), "snail_instances_rebuild_dev")) return 2;
	if(rebuild(NULL, xf, NULL, 0, perm, info, NULL) == 0 || !strstr(snail_last_error(), "0 instances")) return 3;
	if(rebuild(NULL, NULL, NULL, 1, perm, info, NULL) == 0 || !strstr(snail_last_error(), "null transforms")) return 4;
	if(read_tree(NULL, NULL, 0, &nNodes, NULL, NULL, 0, &n) == 0 || !strstr(snail_last_error(), "snail_instances_read_tree")) return 5;
	if(perm[0] != 7 || info[0] != 7 || info[3] != 7 || nNodes != 7 || n != 7) return 6;
	if(SNAIL_INSTANCES_MAX_DEPTH != 64) return 7;
	printf("C instances build ABI ok: %d symbols\n", (int)(sizeof(fns) / sizeof(fns[0])));
	return 0;
}
