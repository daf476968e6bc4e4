/* The lit-frame entry points of instanced scenes (include/snail_instances_shade.h, reached through include/snail_instances.h) as PLAIN C
 * (gcc -std=c99 -Wall -Werror -pedantic): every function links against libsnailhip.so, and the argument checks that need no GPU answer from
 * a C host (tests/test_instances_shade_host.py). */
#include <stdio.h>
#include <string.h>

#include "../../include/snail_instances.h"

#define ADDR(f) (void (*)(void))f,

int main(void) {
	void (*fns[])(void) = {
		ADDR(snail_instances_render_whitted_dev) ADDR(snail_instances_render_whitted_packets_dev) ADDR(snail_instances_render_image)
	};
	float cam[13] = {0}, amb[3] = {0.1f, 0.1f, 0.1f}, col[3] = {1, 1, 1};
	uint8_t img[4 * 4 * 3];
	memset(img, 7, sizeof(img));
	/* a null handle is refused before anything touches a device, with a text */
	if(snail_instances_render_image(NULL, cam, 4, 4, NULL, 0, amb, col, 0, img, 12, NULL) == 0 || !strstr(snail_last_error(), "snail_instances_render_image")) return 2;
	if(snail_instances_render_whitted_dev(NULL, cam, 4, 4, NULL, 0, amb, col, 0, img, 12, NULL, NULL) == 0) return 3;
	if(snail_instances_render_whitted_packets_dev(NULL, cam, 4, 4, NULL, 1, NULL, 0, amb, col, 0, img, NULL, NULL) == 0) return 4;
	if(img[0] != 7 || img[47] != 7) return 5;
	if(SNAIL_RENDER_AA4 != 4 || SNAIL_WHITTED_REFLECTIONS != 1 || SNAIL_MAX_LIGHTS != 8) return 6;
	printf("C instances shade ABI ok: %d symbols\n", (int)(sizeof(fns) / sizeof(fns[0])));
	return 0;
}
