/* The entry points of include/snail_materials_tree.h as PLAIN C (gcc -std=c99 -Wall -Werror -pedantic): every function links against
 * libsnailhip.so, and the argument checks that need no GPU answer from a C host (tests/test_materials_tree_host.py). */
#include <stdio.h>
#include <string.h>

#include "../../include/snail_materials_tree.h"

#define ADDR(f) (void (*)(void))f,

int main(void) {
	void (*fns[])(void) = {
		ADDR(snail_materials_mirror_rays_dev) ADDR(snail_materials_tree_frame_packets_dev) ADDR(snail_materials_tree_render_tiles)
		ADDR(snail_materials_tree_render_frame) ADDR(snail_materials_set_level_budget) ADDR(snail_materials_level_bytes)
	};
	float amb[3] = {0.1f, 0.1f, 0.1f}, cam[13] = {0};
	uint8_t img[4 * 4 * 3];
	uint64_t trunc = 0;
	int32_t rect[4] = {0, 0, 4, 4};
	int64_t off[1] = {0};
	const int all = SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_DEPTH | SNAIL_RENDER_AA4;
	memset(img, 7, sizeof(img));
	if(SNAIL_MAT_LEVEL_BUDGET != 1073741824ull) return 1;
	/* unknown bits are refused by a text naming `flags`, before maxDepth and the (null) handle are looked at */
	if(snail_materials_tree_render_frame(NULL, cam, 4, 4, NULL, 0, amb, 0x100, img, 12, 0, &trunc, NULL) == 0 || !strstr(snail_last_error(), "flags")) return 2;
	if(snail_materials_tree_render_tiles(NULL, cam, 4, 4, rect, off, 1, NULL, 0, amb, 8, NULL, img, 0, &trunc, NULL) == 0 || !strstr(snail_last_error(), "flags")) return 3;
	if(snail_materials_tree_frame_packets_dev(NULL, cam, 4, 4, NULL, 1, NULL, 0, amb, -1, NULL, img, 0, &trunc, NULL, NULL) == 0 || !strstr(snail_last_error(), "flags")) return 4;
	/* every combination of the three is accepted: maxDepth is what stops these */
	if(snail_materials_tree_render_frame(NULL, cam, 4, 4, NULL, 0, amb, all, img, 12, 0, &trunc, NULL) == 0 || !strstr(snail_last_error(), "maxDepth")) return 5;
	if(snail_materials_tree_render_frame(NULL, cam, 4, 4, NULL, 0, amb, all, img, 12, SNAIL_MAT_TRANSP_MAX_DEPTH + 1, &trunc, NULL) == 0 || !strstr(snail_last_error(), "maxDepth")) return 6;
	if(snail_materials_tree_render_frame(NULL, cam, 4, 4, NULL, 0, amb, all, img, 12, 8, NULL, NULL) == 0 || !strstr(snail_last_error(), "truncated")) return 7;
	if(snail_materials_tree_render_frame(NULL, cam, 4, 4, NULL, 0, amb, all, img, 12, 8, &trunc, NULL) == 0 || !strstr(snail_last_error(), "handle")) return 8;
	if(snail_materials_mirror_rays_dev(NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == 0 ||
	   !strstr(snail_last_error(), "snail_materials_mirror_rays_dev")) return 9;
	if(snail_materials_set_level_budget(NULL, 1) == 0 || !strstr(snail_last_error(), "handle")) return 10;
	if(snail_materials_level_bytes(0, 0, 1) <= 0 || snail_materials_level_bytes(0, SNAIL_RENDER_DEPTH, 1) != 0 || snail_materials_level_bytes(0, 0, 9) != -1) return 11;
	if(img[0] != 7 || img[47] != 7 || trunc != 0) return 12;
	printf("C materials tree ABI ok: %d symbols\n", (int)(sizeof(fns) / sizeof(fns[0])));
	return 0;
}
