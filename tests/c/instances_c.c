/* include/snail_instances.h as PLAIN C (gcc -std=c99 -Wall -Werror -pedantic): every function it declares links against libsnailhip.so,
 * and the builder runs from a C host without a GPU (tests/test_instances_abi.py). */
#include <stdio.h>
#include <string.h>

#include "../../include/snail_instances.h"

#define ADDR(f) (void (*)(void))f,

int main(void) {
	void (*fns[])(void) = {
		ADDR(snail_instances_build) ADDR(snail_instances_create) ADDR(snail_instances_update) ADDR(snail_instances_destroy)
		ADDR(snail_instances_trace_primary_dev) ADDR(snail_instances_trace_packets_dev) ADDR(snail_instances_trace_rays_dev)
		ADDR(snail_instances_trace_shadow_dev) ADDR(snail_instances_trace_rays) ADDR(snail_instances_trace_shadow)
		ADDR(snail_instances_trace_frame_packets) ADDR(snail_instances_render_depth)
	};
	/* three identity-rotated instances of one unit box along x */
	float xf[3 * 12];
	int32_t bi[3] = {0, 0, 0}, perm[3];
	float box[6] = {0, 0, 0, 1, 1, 1};
	unsigned char nodes[6 * 32];
	int nNodes = 0, depth = 0, k;
	memset(xf, 0, sizeof(xf));
	for(k = 0; k < 3; k++) { xf[k * 12 + 0] = xf[k * 12 + 4] = xf[k * 12 + 8] = 1.0f; xf[k * 12 + 9] = 3.0f * (float)k; }
	if(snail_instances_build(xf, bi, 3, box, 1, nodes, &nNodes, &depth, perm) != 0) { printf("build failed: %s\n", snail_last_error()); return 1; }
	bi[1] = 5;
	if(snail_instances_build(xf, bi, 3, box, 1, nodes, &nNodes, &depth, perm) == 0 || !strstr(snail_last_error(), "names BLAS")) return 2;
	printf("C instances ABI ok: %d symbols, %d nodes, depth %d\n", (int)(sizeof(fns) / sizeof(fns[0])), nNodes, depth);
	return 0;
}
