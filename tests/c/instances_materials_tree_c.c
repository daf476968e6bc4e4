/* The transparency continuation together with the bounce, tile lists, 4x antialiasing and the tint under full shading of instanced scenes
 * (include/snail_instances_materials_tree.h) as PLAIN C (gcc -std=c99 -Wall -Werror -pedantic): every function links against libsnailhip.so,
 * and the argument checks that need no GPU answer from a C host (tests/test_instances_materials_tree_abi.py). */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "../../include/snail_instances_materials_tree.h"

#define ADDR(f) (void (*)(void))f,

int main(void) {
	void (*fns[])(void) = {
		ADDR(snail_instances_materials_mirror_rays_dev) ADDR(snail_instances_materials_tree_frame_packets_dev)
		ADDR(snail_instances_materials_tree_render_tiles) ADDR(snail_instances_materials_tree_render_frame)
		ADDR(snail_instances_materials_set_level_budget) ADDR(snail_instances_materials_level_bytes)
	};
	float cam[13] = {0}, amb[3] = {0.1f, 0.1f, 0.1f}, tint[3] = {0.6f, 1.0f, 0.6f};
	uint8_t img[4 * 4 * 3], data[16 * 16 * 3];
	int32_t xy[2] = {0, 0}, tile[4] = {0, 0, 16, 16}, bad[4] = {0, 0, 0, 16};
	int64_t off[1] = {0};
	uint64_t trunc = 5;
	const int all = SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_DEPTH | SNAIL_RENDER_AA4;
	memset(img, 7, sizeof(img));
	memset(data, 7, sizeof(data));
	/* unknown bits are refused by a text that names `flags`, before anything else is looked at */
	if(snail_instances_materials_tree_frame_packets_dev(NULL, NULL, 0, 0, NULL, 1, NULL, 0, NULL, 8, NULL, NULL, 0, NULL, NULL, NULL) == 0 || !strstr(snail_last_error(), "flags")) return 2;
	if(snail_instances_materials_tree_render_tiles(NULL, NULL, 0, 0, NULL, NULL, 1, NULL, 0, NULL, all | 64, NULL, NULL, 0, NULL, NULL) == 0 || !strstr(snail_last_error(), "flags")) return 3;
	if(snail_instances_materials_tree_render_frame(NULL, NULL, 0, 0, NULL, 0, NULL, 16, NULL, 0, 0, NULL, NULL) == 0 || !strstr(snail_last_error(), "flags")) return 4;
	/* every known combination passes the flags; the depth is judged next */
	if(snail_instances_materials_tree_frame_packets_dev(NULL, cam, 4, 4, xy, 1, NULL, 0, amb, all, NULL, img, 0, &trunc, NULL, NULL) == 0 || !strstr(snail_last_error(), "maxDepth")) return 5;
	if(snail_instances_materials_tree_render_frame(NULL, cam, 4, 4, NULL, 0, amb, all, img, 12, SNAIL_MAT_TRANSP_MAX_DEPTH + 1, &trunc, NULL) == 0 ||
	   !strstr(snail_last_error(), "maxDepth")) return 6;
	/* a null truncated-lane word, a tint that is not finite, a bad tile rect: all before the handle */
	if(snail_instances_materials_tree_frame_packets_dev(NULL, cam, 4, 4, xy, 1, NULL, 0, amb, 0, NULL, img, 8, NULL, NULL, NULL) == 0 || !strstr(snail_last_error(), "truncated")) return 7;
	tint[1] = (float)INFINITY;
	if(snail_instances_materials_tree_render_tiles(NULL, cam, 16, 16, tile, off, 1, NULL, 0, amb, 0, tint, data, 8, &trunc, NULL) == 0 || !strstr(snail_last_error(), "tint")) return 8;
	if(snail_instances_materials_tree_render_tiles(NULL, cam, 16, 16, bad, off, 1, NULL, 0, amb, 0, NULL, data, 8, &trunc, NULL) == 0 || !strstr(snail_last_error(), "bad rect")) return 9;
	/* good arguments: the handle is looked at last */
	if(snail_instances_materials_tree_render_tiles(NULL, cam, 16, 16, tile, off, 1, NULL, 0, amb, all, NULL, data, 8, &trunc, NULL) == 0 || strstr(snail_last_error(), "flags") ||
	   !strstr(snail_last_error(), "handle")) return 10;
	if(snail_instances_materials_tree_render_frame(NULL, cam, 4, 4, NULL, 0, amb, 0, img, 12, 1, &trunc, NULL) == 0 || !strstr(snail_last_error(), "handle")) return 11;
	if(snail_instances_materials_set_level_budget(NULL, 1) == 0 || !strstr(snail_last_error(), "handle")) return 12;
	/* the mirror stage: no packets is no work; a null buffer is refused whatever the handle is */
	if(snail_instances_materials_mirror_rays_dev(NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) != 0) return 13;
	if(snail_instances_materials_mirror_rays_dev(NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == 0 ||
	   !strstr(snail_last_error(), "null buffer")) return 14;
	/* the bytes of one output packet: no device; -1 for what the frame functions refuse */
	if(snail_instances_materials_level_bytes(8, all, 8) != 0 || snail_instances_materials_level_bytes(0, 0, 0) != -1 || snail_instances_materials_level_bytes(0, 8, 1) != -1 ||
	   snail_instances_materials_level_bytes(SNAIL_MAX_LIGHTS + 1, 0, 1) != -1) return 15;
	/* the header's worked figure: (8 + 9) levels x 140.75 KiB + 4.5 KiB */
	if(snail_instances_materials_level_bytes(8, SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_AA4, 8) != 17 * 144128 + 4608) return 16;
	if(img[0] != 7 || img[47] != 7 || data[0] != 7 || data[767] != 7 || trunc != 5) return 17;
	printf("C instances materials tree ABI ok: %d symbols\n", (int)(sizeof(fns) / sizeof(fns[0])));
	return 0;
}
