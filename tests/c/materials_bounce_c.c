/* The entry points of the bounce under full shading (include/snail_materials_bounce.h) as PLAIN C (gcc -std=c99 -Wall -Werror -pedantic):
 * every function links against libsnailhip.so, and the argument checks that need no GPU answer from a C host
 * (tests/test_materials_bounce_host.py). */
#include <stdio.h>
#include <string.h>

#include "../../include/snail_materials_bounce.h"

#define ADDR(f) (void (*)(void))f,

int main(void) {
	void (*fns[])(void) = {
		ADDR(snail_materials_mirror_packets_dev) ADDR(snail_materials_shade_rays_dev) ADDR(snail_materials_bounce_dev)
		ADDR(snail_materials_bounce_packets_dev) ADDR(snail_materials_bounce_image)
	};
	float cam[13] = {0}, amb[3] = {0.1f, 0.1f, 0.1f};
	uint8_t img[4 * 4 * 3];
	int bad[4] = {SNAIL_RENDER_DEPTH, SNAIL_RENDER_AA4, SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_DEPTH, 0x100}, k;
	memset(img, 7, sizeof(img));
	/* flags other than 0 and SNAIL_RENDER_REFLECTIONS: refused by their own text, before the (null) handle is looked at */
	for(k = 0; k < 4; k++) {
		if(snail_materials_bounce_image(NULL, cam, 4, 4, NULL, 0, amb, bad[k], img, 12, NULL) == 0 || !strstr(snail_last_error(), "flags")) return 1;
		if(snail_materials_bounce_dev(NULL, cam, 4, 4, NULL, 0, amb, bad[k], img, 12, NULL, NULL) == 0 || !strstr(snail_last_error(), "flags")) return 2;
		if(snail_materials_bounce_packets_dev(NULL, cam, 4, 4, NULL, 1, NULL, 0, amb, bad[k], img, NULL, NULL) == 0 || !strstr(snail_last_error(), "flags")) return 3;
	}
	/* the two flags that are accepted reach the handle check, which names the function */
	if(snail_materials_bounce_image(NULL, cam, 4, 4, NULL, 0, amb, 0, img, 12, NULL) == 0 || strstr(snail_last_error(), "flags") ||
	   !strstr(snail_last_error(), "snail_materials_bounce_image")) return 4;
	if(snail_materials_bounce_dev(NULL, cam, 4, 4, NULL, 0, amb, SNAIL_RENDER_REFLECTIONS, img, 12, NULL, NULL) == 0 || strstr(snail_last_error(), "flags")) return 5;
	if(snail_materials_bounce_packets_dev(NULL, cam, 4, 4, NULL, 1, NULL, 0, amb, SNAIL_RENDER_REFLECTIONS, img, NULL, NULL) == 0 || strstr(snail_last_error(), "flags")) return 6;
	if(snail_materials_mirror_packets_dev(NULL, cam, 4, 4, NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == 0) return 7;
	if(snail_materials_shade_rays_dev(NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == 0) return 8;
	if(img[0] != 7 || img[47] != 7) return 9;
	printf("C materials bounce ABI ok: %d symbols\n", (int)(sizeof(fns) / sizeof(fns[0])));
	return 0;
}
