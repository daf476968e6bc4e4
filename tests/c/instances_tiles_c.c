/* The tile renderer of instanced scenes (include/snail_instances_tiles.h, reached through include/snail_instances.h) as PLAIN C
 * (gcc -std=c99 -Wall -Werror -pedantic): every function links against libsnailhip.so, and the argument checks that need no GPU answer from
 * a C host (tests/test_instances_tiles_host.py). */
#include <stdio.h>
#include <string.h>

#include "../../include/snail_instances.h"

#define ADDR(f) (void (*)(void))f,

int main(void) {
	void (*fns[])(void) = {
		ADDR(snail_instances_shade_packets_dev) ADDR(snail_instances_render_tiles) ADDR(snail_instances_render_frame)
	};
	float cam[13] = {0}, amb[3] = {0.1f, 0.1f, 0.1f}, col[3] = {1, 1, 1}, tint[3] = {0.6f, 1.0f, 1.0f};
	int32_t coords[4] = {0, 0, 4, 4};
	int64_t offsets[1] = {0};
	uint8_t img[4 * 4 * 3];
	memset(img, 7, sizeof(img));
	/* a null handle is refused before anything touches a device, with a text */
	if(snail_instances_render_tiles(NULL, cam, 4, 4, coords, offsets, 1, NULL, 0, amb, col, SNAIL_RENDER_AA4, tint, img, NULL) == 0 ||
	   !strstr(snail_last_error(), "snail_instances_render_tiles"))
		return 2;
	if(snail_instances_render_frame(NULL, cam, 4, 4, NULL, 0, amb, col, SNAIL_RENDER_AA4, img, 12, NULL) == 0) return 3;
	if(snail_instances_shade_packets_dev(NULL, cam, 4, 4, NULL, 1, NULL, 0, amb, col, 0, tint, img, NULL, NULL) == 0) return 4;
	if(img[0] != 7 || img[47] != 7) return 5;
	if(SNAIL_RENDER_REFLECTIONS != 1 || SNAIL_RENDER_DEPTH != 2 || SNAIL_RENDER_AA4 != 4 || SNAIL_MAX_LIGHTS != 8) return 6;
	printf("C instances tiles ABI ok: %d symbols\n", (int)(sizeof(fns) / sizeof(fns[0])));
	return 0;
}
