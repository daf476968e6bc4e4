/* The entry points of include/snail_materials_transparency.h as PLAIN C (gcc -std=c99 -Wall -Werror -pedantic): every function links against
 * libsnailhip.so, and the argument checks that need no GPU answer from a C host (tests/test_materials_transparency_host.py). */
#include <stdio.h>
#include <string.h>

#include "../../include/snail_materials_transparency.h"

#define ADDR(f) (void (*)(void))f,

int main(void) {
	void (*fns[])(void) = {
		ADDR(snail_materials_create_transparent) ADDR(snail_materials_can_select_transparent) ADDR(snail_materials_shade_packets_transp_dev)
		ADDR(snail_materials_shade_rays_transp_dev) ADDR(snail_materials_continue_packets_dev) ADDR(snail_materials_transparent_dev)
		ADDR(snail_materials_transparent_packets_dev) ADDR(snail_materials_transparent_image)
	};
	float amb[3] = {0.1f, 0.1f, 0.1f};
	uint8_t img[4 * 4 * 3];
	uint64_t trunc = 0;
	int bad[3] = {SNAIL_RENDER_REFLECTIONS, SNAIL_RENDER_AA4, 0x100}, k;
	float cam[13] = {0};
	uint8_t rec[64] = {0}, texels[64] = {0};
	int32_t map[1] = {0}, op[1] = {0}, opBad[1] = {1};
	SnailMaterial mat;
	SnailTexture tex;
	memset(&mat, 0, sizeof(mat));
	mat.kind = SNAIL_MAT_TRANSPARENT; mat.nDotR = 1;
	tex.levels = texels; tex.width = 2; tex.height = 2;
	if(SNAIL_MAT_TRANSP_MAX_DEPTH != 8) return 1;
	/* the old creator keeps refusing the kind, by its own text */
	if(snail_materials_create(NULL, rec, 1, map, 1, &mat, 1, &tex, 1) != NULL || !strstr(snail_last_error(), "transparent kind")) return 2;
	/* the new one validates both texture indices before it looks at the scene ... */
	if(snail_materials_create_transparent(NULL, rec, 1, map, 1, &mat, 1, opBad, &tex, 1) != NULL || !strstr(snail_last_error(), "opacity texture index")) return 3;
	if(snail_materials_create_transparent(NULL, rec, 1, map, 1, &mat, 1, NULL, &tex, 1) != NULL || !strstr(snail_last_error(), "opacity texture array")) return 4;
	/* ... and accepts the kind: the null scene is what stops the call */
	if(snail_materials_create_transparent(NULL, rec, 1, map, 1, &mat, 1, op, &tex, 1) != NULL || strstr(snail_last_error(), "transparent kind") ||
	   !strstr(snail_last_error(), "snail_materials_create_transparent")) return 5;
	if(snail_materials_can_select_transparent(NULL) != -1) return 6;
	if(snail_materials_shade_packets_transp_dev(NULL, cam, 4, 4, NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == 0) return 7;
	if(snail_materials_shade_rays_transp_dev(NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == 0) return 8;
	if(snail_materials_continue_packets_dev(NULL, cam, 4, 4, NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == 0 ||
	   !strstr(snail_last_error(), "snail_materials_continue_packets_dev")) return 9;
	/* the frames: every nonzero flag is refused by a text naming `flags`, a depth outside 1..8 by one naming maxDepth, before the (null) handle */
	memset(img, 7, sizeof(img));
	for(k = 0; k < 3; k++) {
		if(snail_materials_transparent_image(NULL, cam, 4, 4, NULL, 0, amb, bad[k], img, 12, 8, &trunc, NULL) == 0 || !strstr(snail_last_error(), "flags")) return 10;
		if(snail_materials_transparent_dev(NULL, cam, 4, 4, NULL, 0, amb, bad[k], img, 12, 8, &trunc, NULL, NULL) == 0 || !strstr(snail_last_error(), "flags")) return 11;
		if(snail_materials_transparent_packets_dev(NULL, cam, 4, 4, NULL, 1, NULL, 0, amb, bad[k], img, 8, &trunc, NULL, NULL) == 0 || !strstr(snail_last_error(), "flags")) return 12;
	}
	if(snail_materials_transparent_image(NULL, cam, 4, 4, NULL, 0, amb, 0, img, 12, 0, &trunc, NULL) == 0 || !strstr(snail_last_error(), "maxDepth")) return 13;
	if(snail_materials_transparent_image(NULL, cam, 4, 4, NULL, 0, amb, 0, img, 12, SNAIL_MAT_TRANSP_MAX_DEPTH + 1, &trunc, NULL) == 0 || !strstr(snail_last_error(), "maxDepth")) return 14;
	if(snail_materials_transparent_image(NULL, cam, 4, 4, NULL, 0, amb, 0, img, 12, 8, &trunc, NULL) == 0 || !strstr(snail_last_error(), "handle")) return 15;
	if(img[0] != 7 || img[47] != 7 || trunc != 0) return 16;
	printf("C materials transparency ABI ok: %d symbols\n", (int)(sizeof(fns) / sizeof(fns[0])));
	return 0;
}
