/* The full-shading entry points (include/snail_materials.h) as PLAIN C (gcc -std=c99 -Wall -Werror -pedantic): every function links
 * against libsnailhip.so, the host functions compute, and the argument checks that need no GPU answer from a C host
 * (tests/test_materials_abi.py). */
#include <stdio.h>
#include <string.h>

#include "../../include/snail_materials.h"

#define ADDR(f) (void (*)(void))f,

int main(void) {
	void (*fns[])(void) = {
		ADDR(snail_shtris_pack) ADDR(snail_texture_size) ADDR(snail_texture_build) ADDR(snail_materials_create) ADDR(snail_materials_destroy)
		ADDR(snail_materials_shade_packets_dev) ADDR(snail_render_materials_dev) ADDR(snail_render_materials_packets_dev)
		ADDR(snail_render_materials_image)
	};
	float cam[13] = {0}, amb[3] = {0.1f, 0.1f, 0.1f};
	uint8_t img[4 * 4 * 3], tex[2 * 2 * 3 + 3 + 8], level0[12] = {10, 20, 30, 50, 60, 70, 90, 100, 110, 130, 140, 150};
	float uv[6] = {0, 0, 1, 0, 0, 1}, nrm[9] = {0, 0, 1, 0, 1, 0, 1, 0, 0}, rec[16];
	int32_t mat = 3, map[1] = {-1};
	uint8_t flat = 1;
	uint32_t id;
	SnailMaterial m;
	int levels = 0;
	memset(img, 7, sizeof(img));
	if(sizeof(SnailMaterial) != 40) return 1;
	/* a null handle is refused before anything touches a device, with a text */
	if(snail_render_materials_image(NULL, cam, 4, 4, NULL, 0, amb, 0, img, 12, NULL) == 0 || !strstr(snail_last_error(), "snail_render_materials_image")) return 2;
	if(snail_render_materials_dev(NULL, cam, 4, 4, NULL, 0, amb, 0, img, 12, NULL, NULL) == 0) return 3;
	if(snail_render_materials_packets_dev(NULL, cam, 4, 4, NULL, 1, NULL, 0, amb, 0, img, NULL, NULL) == 0) return 4;
	if(snail_materials_shade_packets_dev(NULL, cam, 4, 4, NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL) == 0) return 5;
	/* nonzero flags: refused by their own text */
	if(snail_render_materials_image(NULL, cam, 4, 4, NULL, 0, amb, 1, img, 12, NULL) == 0 || !strstr(snail_last_error(), "flags")) return 6;
	if(img[0] != 7 || img[47] != 7) return 7;
	/* the host functions */
	if(snail_texture_size(2, 2, &levels) != 15 || levels != 2) return 8;
	if(snail_texture_size(3, 2, &levels) != 0) return 9;
	if(snail_texture_build(level0, 2, 2, tex, 15, &levels) != 0 || levels != 2 || tex[12] != (10 + 50 + 90 + 130) / 4) return 10;
	if(snail_texture_build(level0, 2, 2, tex, 14, &levels) == 0) return 11;
	if(snail_shtris_pack(uv, nrm, &mat, &flat, 1, NULL, rec) != 0 || rec[2] != 1.0f || rec[9] != 0.0f || rec[10] != 1.0f || rec[11] != -1.0f) return 12;
	memcpy(&id, rec + 15, 4);
	if(id != (0x80000000u | 3u)) return 13;
	/* a transparent material is refused at creation (no scene needed to learn that) */
	memset(&m, 0, sizeof(m));
	m.kind = SNAIL_MAT_TRANSPARENT;
	mat = 0;
	if(snail_shtris_pack(uv, nrm, &mat, &flat, 1, NULL, rec) != 0) return 14;
	if(snail_materials_create(NULL, rec, 1, map, 1, &m, 1, NULL, 0) != NULL || !strstr(snail_last_error(), "transparent")) return 15;
	snail_materials_destroy(NULL);
	printf("C materials ABI ok: %d symbols\n", (int)(sizeof(fns) / sizeof(fns[0])));
	return 0;
}
