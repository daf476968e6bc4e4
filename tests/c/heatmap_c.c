/* Per-packet TreeStats and the heat-map (include/snail_heatmap.h) as PLAIN C (gcc -std=c99 -Wall -Werror -pedantic): every function links
 * against libsnailhip.so, and the argument checks that need no GPU answer from a C host (tests/test_heatmap_host.py). */
#include <stdio.h>
#include <string.h>

#include "../../include/snail_heatmap.h"

#define ADDR(f) (void (*)(void))f,

int main(void) {
	void (*fns[])(void) = {
		ADDR(snail_packet_stats_dev) ADDR(snail_render_heat_packets_dev) ADDR(snail_render_heat_tiles) ADDR(snail_render_heat_image)
		ADDR(snail_instances_packet_stats_dev) ADDR(snail_instances_heat_packets_dev) ADDR(snail_instances_render_heat_tiles) ADDR(snail_instances_render_heat_frame)
	};
	float cam[13] = {0}, tint[3] = {0.6f, 1.0f, 1.0f};
	int32_t coords[4] = {0, 0, 4, 4};
	int64_t offsets[1] = {0};
	uint8_t img[4 * 4 * 3];
	memset(img, 7, sizeof(img));
	/* a null handle is refused before anything touches a device, with a text that names the function */
	if(snail_render_heat_tiles(NULL, cam, 4, 4, coords, offsets, 1, NULL, 0, SNAIL_RENDER_AA4, img, NULL) == 0 || !strstr(snail_last_error(), "snail_render_heat_tiles")) return 2;
	if(snail_render_heat_image(NULL, cam, 4, 4, NULL, 0, 0, img, 12, NULL) == 0 || !strstr(snail_last_error(), "snail_render_heat_image")) return 3;
	if(snail_render_heat_packets_dev(NULL, cam, 4, 4, NULL, 0, NULL, 0, 0, img, NULL, NULL, NULL) == 0 || !strstr(snail_last_error(), "snail_render_heat_packets_dev")) return 4;
	if(snail_packet_stats_dev(NULL, cam, 4, 4, NULL, 0, NULL, 0, 0, (uint32_t *)(void *)img, NULL, NULL) == 0 || !strstr(snail_last_error(), "snail_packet_stats_dev")) return 5;
	if(snail_instances_render_heat_tiles(NULL, cam, 4, 4, coords, offsets, 1, NULL, 0, SNAIL_RENDER_AA4, tint, img, NULL) == 0 ||
	   !strstr(snail_last_error(), "snail_instances_render_heat_tiles"))
		return 8;
	if(snail_instances_render_heat_frame(NULL, cam, 4, 4, NULL, 0, 0, img, 12, NULL) == 0 || !strstr(snail_last_error(), "snail_instances_render_heat_frame")) return 9;
	if(snail_instances_heat_packets_dev(NULL, cam, 4, 4, NULL, 0, NULL, 0, 0, tint, img, NULL, NULL, NULL) == 0 || !strstr(snail_last_error(), "snail_instances_heat_packets_dev"))
		return 10;
	if(snail_instances_packet_stats_dev(NULL, cam, 4, 4, NULL, 0, NULL, 0, 0, (uint32_t *)(void *)img, NULL, NULL) == 0 ||
	   !strstr(snail_last_error(), "snail_instances_packet_stats_dev"))
		return 11;
	/* depth shading has no heat-map */
	if(snail_render_heat_image(NULL, cam, 4, 4, NULL, 0, SNAIL_RENDER_DEPTH, img, 12, NULL) == 0 || !strstr(snail_last_error(), "SNAIL_RENDER_DEPTH")) return 6;
	if(img[0] != 7 || img[47] != 7) return 7;
	printf("C heatmap ABI ok: %d symbols\n", (int)(sizeof(fns) / sizeof(fns[0])));
	return 0;
}
