/* The transparency continuation under full shading of instanced scenes (include/snail_instances_materials_transparency.h) as PLAIN C (gcc
 * -std=c99 -Wall -Werror -pedantic): every function links against libsnailhip.so, and the argument checks that need no GPU answer from a C
 * host (tests/test_instances_materials_transparency_host.py). */
#include <stdio.h>
#include <string.h>

#include "../../include/snail_instances_materials_transparency.h"

#define ADDR(f) (void (*)(void))f,

int main(void) {
	void (*fns[])(void) = {
		ADDR(snail_instances_materials_create_transparent) ADDR(snail_instances_materials_can_select_transparent)
		ADDR(snail_instances_materials_shade_packets_transp_dev) ADDR(snail_instances_materials_shade_rays_transp_dev)
		ADDR(snail_instances_materials_continue_packets_dev) ADDR(snail_instances_materials_transparent_dev)
		ADDR(snail_instances_materials_transparent_packets_dev) ADDR(snail_instances_materials_transparent_image)
	};
	float cam[13] = {0}, amb[3] = {0.1f, 0.1f, 0.1f};
	uint8_t img[4 * 4 * 3];
	uint64_t trunc = 5;
	int flags;
	memset(img, 7, sizeof(img));
	/* every flag, SNAIL_RENDER_REFLECTIONS included, is refused by a text that names `flags`, before the handle is looked at */
	for(flags = 1; flags < 8; flags++) {
		if(snail_instances_materials_transparent_image(NULL, cam, 4, 4, NULL, 0, amb, flags, img, 12, 8, &trunc, NULL) == 0 || !strstr(snail_last_error(), "flags")) return 2;
		if(snail_instances_materials_transparent_dev(NULL, cam, 4, 4, NULL, 0, amb, flags, img, 12, 8, &trunc, NULL, NULL) == 0 || !strstr(snail_last_error(), "flags")) return 3;
		if(snail_instances_materials_transparent_packets_dev(NULL, cam, 4, 4, NULL, 1, NULL, 0, amb, flags, img, 8, &trunc, NULL, NULL) == 0 ||
		   !strstr(snail_last_error(), "flags")) return 4;
	}
	/* flags 0: the depth is judged next, then the handle */
	if(snail_instances_materials_transparent_image(NULL, cam, 4, 4, NULL, 0, amb, 0, img, 12, 0, &trunc, NULL) == 0 || !strstr(snail_last_error(), "maxDepth")) return 5;
	if(snail_instances_materials_transparent_image(NULL, cam, 4, 4, NULL, 0, amb, 0, img, 12, SNAIL_MAT_TRANSP_MAX_DEPTH + 1, &trunc, NULL) == 0 ||
	   !strstr(snail_last_error(), "maxDepth")) return 6;
	if(snail_instances_materials_transparent_image(NULL, cam, 4, 4, NULL, 0, amb, 0, img, 12, 8, &trunc, NULL) == 0 || strstr(snail_last_error(), "flags") ||
	   !strstr(snail_last_error(), "handle")) return 7;
	if(snail_instances_materials_can_select_transparent(NULL) != -1) return 8;
	if(snail_instances_materials_create_transparent(NULL, NULL, 0, NULL, 0, NULL, NULL, 0) != NULL) return 9;
	/* the stages: no packets is no work; a null buffer is refused */
	if(snail_instances_materials_shade_rays_transp_dev(NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) != 0) return 10;
	if(snail_instances_materials_shade_rays_transp_dev(NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == 0 ||
	   !strstr(snail_last_error(), "null buffer")) return 11;
	if(snail_instances_materials_shade_packets_transp_dev(NULL, cam, 4, 4, NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) != 0) return 12;
	if(snail_instances_materials_continue_packets_dev(NULL, cam, 4, 4, NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL,
	                                                  NULL) != 0) return 13;
	if(img[0] != 7 || img[47] != 7 || trunc != 5) return 14;
	printf("C instances materials transparency ABI ok: %d symbols\n", (int)(sizeof(fns) / sizeof(fns[0])));
	return 0;
}
