/* The entry points of include/snail_bvh_fast_batch.h and include/snail_instances_materials_rebuild_all.h as PLAIN C (gcc -std=c99 -Wall
 * -Werror -pedantic): every function links against libsnailhip.so, and the refusals that need no GPU are made with their texts
 * (tests/test_bvh_fast_batch_host.py). */
#include <stdio.h>
#include <string.h>

#include "../../include/snail_bvh_fast_batch.h"
#include "../../include/snail_instances_materials_dynamic.h"
#include "../../include/snail_instances_materials_rebuild_all.h"

#define ADDR(f) (void (*)(void))f,
#define ALL(f) (void (*)(void))f,

static int refused(int rc, const char *text) {
	if(rc != 0 && strstr(snail_last_error(), text)) return 1;
	printf("rc %d, \"%s\" lacks \"%s\"\n", rc, snail_last_error(), text);
	return 0;
}

int main(void) {
	void (*batch[])(void) = { ADDR(snail_scenes_rebuild_fast_dev) };
	void (*all[])(void) = { ALL(snail_instances_materials_rebuild_all_dev) };
	float dummy[9] = {0};
	SnailFastRebuild list[2];
	SnailBlasRebuild blist[2];
	memset(list, 0, sizeof(list));
	memset(blist, 0, sizeof(blist));
	/* the batched rebuild: a null list, nList <= 0; then the entries, before any handle is touched */
	if(!refused(snail_scenes_rebuild_fast_dev(NULL, 1, NULL), "no handle listed")) return 1;
	if(!refused(snail_scenes_rebuild_fast_dev(list, 0, NULL), "no handle listed")) return 2;
	if(!refused(snail_scenes_rebuild_fast_dev(list, -4, NULL), "no handle listed")) return 3;
	list[0].d_verts9 = dummy; list[0].nTris = 1;
	if(!refused(snail_scenes_rebuild_fast_dev(list, 2, NULL), "entry 0: invalid scene handle")) return 4;
	/* the one-call frame step: the list is judged first, as snail_instances_materials_rebuild_dev's, then the set */
	if(!refused(snail_instances_materials_rebuild_all_dev(NULL, NULL, 1, dummy, NULL, 1, NULL, NULL, NULL), "snail_instances_materials_rebuild_all_dev: no BLAS listed")) return 10;
	if(!refused(snail_instances_materials_rebuild_all_dev(NULL, blist, 0, dummy, NULL, 1, NULL, NULL, NULL), "no BLAS listed")) return 11;
	blist[0].blas = 1; blist[1].blas = 1; blist[0].d_verts9 = dummy; blist[1].d_verts9 = dummy;
	if(!refused(snail_instances_materials_rebuild_all_dev(NULL, blist, 2, dummy, NULL, 1, NULL, NULL, NULL), "BLAS 1 is listed twice")) return 12;
	blist[1].blas = 0; blist[1].d_verts9 = NULL;
	if(!refused(snail_instances_materials_rebuild_all_dev(NULL, blist, 2, dummy, NULL, 1, NULL, NULL, NULL), "entry 1 (BLAS 0): null vertices")) return 13;
	blist[1].d_verts9 = dummy;
	if(!refused(snail_instances_materials_rebuild_all_dev(NULL, blist, 2, dummy, NULL, 1, NULL, NULL, NULL), "snail_instances_materials_rebuild_all_dev: invalid instanced material set handle")) return 14;
	printf("C bvh fast batch ABI ok: %d + %d symbols\n", (int)(sizeof(batch) / sizeof(batch[0])), (int)(sizeof(all) / sizeof(all[0])));
	return 0;
}
