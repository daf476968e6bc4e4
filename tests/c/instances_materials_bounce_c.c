/* The bounce under full shading of instanced scenes (include/snail_instances_materials_bounce.h) as PLAIN C (gcc -std=c99 -Wall -Werror
 * -pedantic): every function links against libsnailhip.so, and the argument checks that need no GPU answer from a C host
 * (tests/test_instances_materials_bounce_host.py). */
#include <stdio.h>
#include <string.h>

#include "../../include/snail_instances_materials_bounce.h"

#define ADDR(f) (void (*)(void))f,

int main(void) {
	void (*fns[])(void) = {
		ADDR(snail_instances_materials_mirror_packets_dev) ADDR(snail_instances_materials_shade_rays_dev) ADDR(snail_instances_materials_bounce_dev)
		ADDR(snail_instances_materials_bounce_packets_dev) ADDR(snail_instances_materials_bounce_image)
	};
	float cam[13] = {0}, amb[3] = {0.1f, 0.1f, 0.1f};
	uint8_t img[4 * 4 * 3];
	int flags;
	memset(img, 7, sizeof(img));
	/* every flag but 0 and SNAIL_RENDER_REFLECTIONS is refused by a text that names `flags`, before the handle is looked at */
	for(flags = 2; flags < 8; flags++) {
		if(snail_instances_materials_bounce_image(NULL, cam, 4, 4, NULL, 0, amb, flags, img, 12, NULL) == 0 || !strstr(snail_last_error(), "flags")) return 2;
		if(snail_instances_materials_bounce_dev(NULL, cam, 4, 4, NULL, 0, amb, flags, img, 12, NULL, NULL) == 0 || !strstr(snail_last_error(), "flags")) return 3;
		if(snail_instances_materials_bounce_packets_dev(NULL, cam, 4, 4, NULL, 1, NULL, 0, amb, flags, img, NULL, NULL) == 0 || !strstr(snail_last_error(), "flags")) return 4;
	}
	/* 0 and SNAIL_RENDER_REFLECTIONS are accepted: the null handle is what stops the call */
	for(flags = 0; flags < 2; flags++)
		if(snail_instances_materials_bounce_image(NULL, cam, 4, 4, NULL, 0, amb, flags, img, 12, NULL) == 0 || strstr(snail_last_error(), "flags") ||
		   !strstr(snail_last_error(), "handle")) return 5;
	if(SNAIL_RENDER_REFLECTIONS != 1) return 6;
	/* the stages: no packets is no work; a null buffer is refused; sound arguments are stopped by the missing handle */
	if(snail_instances_materials_shade_rays_dev(NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) != 0) return 7;
	if(snail_instances_materials_shade_rays_dev(NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == 0 || !strstr(snail_last_error(), "null buffer")) return 8;
	if(snail_instances_materials_mirror_packets_dev(NULL, cam, 4, 4, NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) != 0) return 9;
	if(snail_instances_materials_mirror_packets_dev(NULL, cam, 4, 4, NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == 0 ||
	   !strstr(snail_last_error(), "null buffer")) return 10;
	if(img[0] != 7 || img[47] != 7) return 11;
	printf("C instances materials bounce ABI ok: %d symbols\n", (int)(sizeof(fns) / sizeof(fns[0])));
	return 0;
}
