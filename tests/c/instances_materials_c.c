/* The full-shading entry points of instanced scenes (include/snail_instances_materials.h) as PLAIN C (gcc -std=c99 -Wall -Werror -pedantic):
 * every function links against libsnailhip.so, and the argument checks that need no GPU answer from a C host
 * (tests/test_instances_materials_host.py). */
#include <stdio.h>
#include <string.h>

#include "../../include/snail_instances_materials.h"

#define ADDR(f) (void (*)(void))f,

int main(void) {
	void (*fns[])(void) = {
		ADDR(snail_instances_materials_create) ADDR(snail_instances_materials_destroy) ADDR(snail_instances_materials_shade_packets_dev)
		ADDR(snail_instances_render_materials_dev) ADDR(snail_instances_render_materials_packets_dev) ADDR(snail_instances_render_materials_image)
	};
	float cam[13] = {0}, amb[3] = {0.1f, 0.1f, 0.1f};
	uint8_t img[4 * 4 * 3];
	float uv[6] = {0, 0, 1, 0, 0, 1}, nrm[9] = {0, 0, 1, 0, 1, 0, 1, 0, 0}, rec[16];
	int32_t mat = 0, map[1] = {-1};
	uint8_t flat = 1;
	SnailMaterial m;
	SnailBlasShading sh;
	memset(img, 7, sizeof(img));
	/* a null handle is refused before anything touches a device, with a text */
	if(snail_instances_render_materials_image(NULL, cam, 4, 4, NULL, 0, amb, 0, img, 12, NULL) == 0 || !strstr(snail_last_error(), "snail_instances_render_materials_image")) return 2;
	if(snail_instances_render_materials_dev(NULL, cam, 4, 4, NULL, 0, amb, 0, img, 12, NULL, NULL) == 0) return 3;
	if(snail_instances_render_materials_packets_dev(NULL, cam, 4, 4, NULL, 1, NULL, 0, amb, 0, img, NULL, NULL) == 0) return 4;
	if(snail_instances_materials_shade_packets_dev(NULL, cam, 4, 4, NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == 0) return 5;
	/* nonzero flags: refused by their own text */
	if(snail_instances_render_materials_image(NULL, cam, 4, 4, NULL, 0, amb, 1, img, 12, NULL) == 0 || !strstr(snail_last_error(), "flags")) return 6;
	if(img[0] != 7 || img[47] != 7) return 7;
	/* a transparent material is refused at creation (no handle needed to learn that); sound data is stopped by the missing handle */
	if(snail_shtris_pack(uv, nrm, &mat, &flat, 1, NULL, rec) != 0) return 8;
	sh.shtris64 = rec; sh.nTris = 1; sh.matMap = map; sh.nMap = 1;
	memset(&m, 0, sizeof(m));
	m.kind = SNAIL_MAT_TRANSPARENT;
	if(snail_instances_materials_create(NULL, &sh, 1, &m, 1, NULL, 0) != NULL || !strstr(snail_last_error(), "transparent")) return 9;
	if(snail_instances_materials_create(NULL, &sh, 1, NULL, 0, NULL, 0) != NULL || !strstr(snail_last_error(), "invalid instances handle")) return 10;
	if(snail_instances_materials_create(NULL, NULL, 0, NULL, 0, NULL, 0) != NULL) return 11;
	snail_instances_materials_destroy(NULL);
	printf("C instances materials ABI ok: %d symbols\n", (int)(sizeof(fns) / sizeof(fns[0])));
	return 0;
}
