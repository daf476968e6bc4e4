/* The entry points of include/snail_instances_materials_heatmap.h as PLAIN C (gcc -std=c99 -Wall -Werror -pedantic): every function links
 * against libsnailhip.so, and the argument checks that need no GPU answer from a C host (tests/test_instances_materials_heat_host.py). */
#include <stdio.h>
#include <string.h>

#include "../../include/snail_instances_materials_heatmap.h"

#define ADDR(f) (void (*)(void))f,

int main(void) {
	void (*fns[])(void) = {
		ADDR(snail_instances_materials_packet_stats_dev) ADDR(snail_instances_materials_heat_packets_dev) ADDR(snail_instances_materials_render_heat_tiles)
		ADDR(snail_instances_materials_render_heat_frame)
	};
	float cam[13] = {0};
	uint8_t img[4 * 4 * 3];
	uint32_t ps[4] = {7, 7, 7, 7};
	uint64_t trunc = 0;
	int32_t rect[4] = {0, 0, 4, 4};
	int64_t off[1] = {0};
	const int both = SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_AA4;
	memset(img, 7, sizeof(img));
	/* SNAIL_RENDER_DEPTH and unknown bits are refused by a text naming `flags`, before maxDepth and the (null) handle are looked at */
	if(snail_instances_materials_render_heat_frame(NULL, cam, 4, 4, NULL, 0, SNAIL_RENDER_DEPTH, img, 12, 0, &trunc, NULL) == 0 ||
	   !strstr(snail_last_error(), "SNAIL_RENDER_DEPTH") || !strstr(snail_last_error(), "flags")) return 2;
	if(snail_instances_materials_render_heat_tiles(NULL, cam, 4, 4, rect, off, 1, NULL, 0, 8, NULL, img, 0, &trunc, NULL) == 0 || !strstr(snail_last_error(), "flags")) return 3;
	if(snail_instances_materials_heat_packets_dev(NULL, cam, 4, 4, NULL, 1, NULL, 0, 0x100, NULL, img, NULL, 0, &trunc, NULL, NULL) == 0 || !strstr(snail_last_error(), "flags"))
		return 4;
	/* the counters have no antialiased form */
	if(snail_instances_materials_packet_stats_dev(NULL, cam, 4, 4, NULL, 1, NULL, 0, SNAIL_RENDER_AA4, 8, ps, &trunc, NULL, NULL) == 0 || !strstr(snail_last_error(), "flags"))
		return 5;
	/* both bits are accepted by the image forms: maxDepth is what stops these */
	if(snail_instances_materials_render_heat_frame(NULL, cam, 4, 4, NULL, 0, both, img, 12, 0, &trunc, NULL) == 0 || !strstr(snail_last_error(), "maxDepth")) return 6;
	if(snail_instances_materials_render_heat_frame(NULL, cam, 4, 4, NULL, 0, both, img, 12, SNAIL_MAT_TRANSP_MAX_DEPTH + 1, &trunc, NULL) == 0 ||
	   !strstr(snail_last_error(), "maxDepth")) return 7;
	if(snail_instances_materials_render_heat_frame(NULL, cam, 4, 4, NULL, 0, both, img, 12, 8, NULL, NULL) == 0 || !strstr(snail_last_error(), "truncated")) return 8;
	if(snail_instances_materials_render_heat_frame(NULL, cam, 4, 4, NULL, 0, both, img, 12, 8, &trunc, NULL) == 0 || !strstr(snail_last_error(), "handle")) return 9;
	if(snail_instances_materials_packet_stats_dev(NULL, cam, 4, 4, NULL, 1, NULL, 0, SNAIL_RENDER_REFLECTIONS, 8, ps, &trunc, NULL, NULL) == 0 ||
	   !strstr(snail_last_error(), "handle")) return 10;
	if(img[0] != 7 || img[47] != 7 || ps[0] != 7 || ps[3] != 7 || trunc != 0) return 11;
	printf("C instances materials heat ABI ok: %d symbols\n", (int)(sizeof(fns) / sizeof(fns[0])));
	return 0;
}
