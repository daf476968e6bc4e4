/* The entry points of the tile renderer of full-shaded plain scenes (include/snail_materials_tiles.h) as PLAIN C (gcc -std=c99 -Wall -Werror
 * -pedantic): every function links against libsnailhip.so with the header's signature, and the argument checks that need no GPU answer from
 * a C host (tests/test_materials_tiles_host.py). */
#include <stdio.h>
#include <string.h>

#include "../../include/snail_materials_tiles.h"

#define ADDR(f) (void (*)(void))f,

int main(void) {
	void (*fns[])(void) = {
		ADDR(snail_materials_frame_packets_dev) ADDR(snail_materials_render_tiles) ADDR(snail_materials_render_frame)
	};
	/* the header's signatures, spelled out: a mismatch is a compile error */
	int (*fp)(SnailMaterials *, const float[13], int, int, const int32_t *, int, const float *, int, const float[3], int, const float *, uint8_t *, uint64_t *, void *) =
		snail_materials_frame_packets_dev;
	int (*ft)(SnailMaterials *, const float[13], int, int, const int32_t *, const int64_t *, int, const float *, int, const float[3], int, const float *, uint8_t *,
			  uint64_t[4]) = snail_materials_render_tiles;
	int (*ff)(SnailMaterials *, const float[13], int, int, const float *, int, const float[3], int, uint8_t *, int, uint64_t[4]) = snail_materials_render_frame;
	float cam[13] = {0}, amb[3] = {0.1f, 0.1f, 0.1f};
	int32_t coords[4] = {0, 0, 4, 4}, xy[2] = {0, 0};
	int64_t off[1] = {0};
	uint8_t img[4 * 4 * 3];
	int all = SNAIL_RENDER_REFLECTIONS | SNAIL_RENDER_DEPTH | SNAIL_RENDER_AA4, k;
	memset(img, 7, sizeof(img));
	/* unknown flag bits: refused by a text that names `flags`, before the (null) handle is looked at */
	if(fp(NULL, cam, 4, 4, xy, 1, NULL, 0, amb, 8, NULL, img, NULL, NULL) == 0 || !strstr(snail_last_error(), "flags")) return 1;
	if(ft(NULL, cam, 4, 4, coords, off, 1, NULL, 0, amb, 0x100, NULL, img, NULL) == 0 || !strstr(snail_last_error(), "flags")) return 2;
	if(ff(NULL, cam, 4, 4, NULL, 0, amb, -1, img, 12, NULL) == 0 || !strstr(snail_last_error(), "flags")) return 3;
	/* every combination of the three flags reaches the handle check, which names the function */
	for(k = 0; k <= all; k++) {
		if(fp(NULL, cam, 4, 4, xy, 1, NULL, 0, amb, k, NULL, img, NULL, NULL) == 0 || strstr(snail_last_error(), "flags") ||
		   !strstr(snail_last_error(), "snail_materials_frame_packets_dev")) return 4;
		if(ft(NULL, cam, 4, 4, coords, off, 1, NULL, 0, amb, k, NULL, img, NULL) == 0 || strstr(snail_last_error(), "flags") ||
		   !strstr(snail_last_error(), "snail_materials_render_tiles")) return 5;
		if(ff(NULL, cam, 4, 4, NULL, 0, amb, k, img, 12, NULL) == 0 || strstr(snail_last_error(), "flags") || !strstr(snail_last_error(), "snail_materials_render_frame")) return 6;
	}
	if(img[0] != 7 || img[47] != 7) return 7;
	printf("C materials tiles ABI ok: %d symbols\n", (int)(sizeof(fns) / sizeof(fns[0])));
	return 0;
}
