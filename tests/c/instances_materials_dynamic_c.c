/* The entry points of include/snail_instances_materials_dynamic.h as PLAIN C (gcc -std=c99 -Wall -Werror -pedantic): every function links
 * against libsnailhip.so, and the refusals that need no GPU are made with their texts (tests/test_instances_materials_dynamic_host.py). */
#include <stdio.h>
#include <string.h>

#include "../../include/snail_instances_materials_dynamic.h"

#define ADDR(f) (void (*)(void))f,

static int refused(int rc, const char *text) {
	if(rc != 0 && strstr(snail_last_error(), text)) return 1;
	printf("rc %d, \"%s\" lacks \"%s\"\n", rc, snail_last_error(), text);
	return 0;
}

int main(void) {
	void (*fns[])(void) = { ADDR(snail_instances_materials_create_dev) ADDR(snail_instances_materials_rebuild_dev) ADDR(snail_instances_materials_update_dev) };
	const int32_t map[1] = {-1};
	float dummy[9] = {0};
	int32_t perm[1] = {0};
	uint8_t rec[64] = {0};
	SnailBlasShadingDev per[2];
	SnailBlasRebuild list[2];
	/* a static BLAS's entry is SnailBlasShading's four fields, in its order, at the start */
	if(sizeof(SnailBlasShadingDev) < sizeof(SnailBlasShading) + 6 * sizeof(void *)) return 1;
	memset(per, 0, sizeof(per));
	/* the creator, before any device call: nothing given; neither records nor device data; both; bad host data with the BLAS named; the handle */
	if(snail_instances_materials_create_dev(NULL, NULL, 0, NULL, 0, NULL, NULL, 0, NULL) != NULL || !strstr(snail_last_error(), "no per-BLAS shading data")) return 2;
	per[0].shtris64 = rec; per[0].nTris = 1; per[0].matMap = map; per[0].nMap = 1;
	per[1].nTris = 1; per[1].matMap = map; per[1].nMap = 1;
	if(snail_instances_materials_create_dev(NULL, per, 2, NULL, 0, NULL, NULL, 0, NULL) != NULL || !strstr(snail_last_error(), "BLAS 1: no host records, and a null uv")) return 3;
	per[1].d_uv6 = dummy; per[1].d_matIdx = perm; per[1].d_perm = perm;
	if(snail_instances_materials_create_dev(NULL, per, 2, NULL, 0, NULL, NULL, 0, NULL) != NULL || !strstr(snail_last_error(), "neither normals nor vertices")) return 4;
	per[1].d_verts9 = dummy;
	per[0].d_nrm9 = dummy;
	if(snail_instances_materials_create_dev(NULL, per, 2, NULL, 0, NULL, NULL, 0, NULL) != NULL || !strstr(snail_last_error(), "BLAS 0: host records AND device data")) return 5;
	per[0].d_nrm9 = NULL;
	per[1].nMap = 0;
	if(snail_instances_materials_create_dev(NULL, per, 2, NULL, 0, NULL, NULL, 0, NULL) != NULL || !strstr(snail_last_error(), "(the shading data of BLAS 1)")) return 6;
	per[1].nMap = 1;
	if(snail_instances_materials_create_dev(NULL, per, 2, NULL, 0, NULL, NULL, 0, NULL) != NULL || !strstr(snail_last_error(), "invalid instances handle")) return 7;
	/* the two list calls: the list is judged before the set */
	memset(list, 0, sizeof(list));
	if(!refused(snail_instances_materials_rebuild_dev(NULL, list, 0, NULL), "no BLAS listed")) return 10;
	if(!refused(snail_instances_materials_update_dev(NULL, NULL, 1, NULL), "no BLAS listed")) return 11;
	list[0].blas = -1;
	if(!refused(snail_instances_materials_rebuild_dev(NULL, list, 1, NULL), "BLAS index -1 is out of range")) return 12;
	list[0].blas = 2; list[0].d_verts9 = dummy; list[0].d_perm = perm;
	list[1] = list[0];
	if(!refused(snail_instances_materials_rebuild_dev(NULL, list, 2, NULL), "BLAS 2 is listed twice")) return 13;
	if(!refused(snail_instances_materials_update_dev(NULL, list, 2, NULL), "BLAS 2 is listed twice")) return 14;
	list[1].blas = 0; list[1].d_verts9 = NULL;
	if(!refused(snail_instances_materials_rebuild_dev(NULL, list, 2, NULL), "entry 1 (BLAS 0): null vertices")) return 15;
	if(!refused(snail_instances_materials_update_dev(NULL, list, 2, NULL), "entry 1 (BLAS 0): null perm, or neither normals nor vertices")) return 16;
	list[1].d_nrm9 = dummy;      /* normals alone serve an update */
	if(!refused(snail_instances_materials_update_dev(NULL, list, 2, NULL), "snail_instances_materials_update_dev: invalid instanced material set handle")) return 17;
	list[1].d_verts9 = dummy;
	if(!refused(snail_instances_materials_rebuild_dev(NULL, list, 2, NULL), "snail_instances_materials_rebuild_dev: invalid instanced material set handle")) return 18;
	printf("C instances materials dynamic ABI ok: %d symbols\n", (int)(sizeof(fns) / sizeof(fns[0])));
	return 0;
}
