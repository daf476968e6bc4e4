/* The entry points of include/snail_materials_dynamic.h as PLAIN C (gcc -std=c99 -Wall -Werror -pedantic): every function links against
 * libsnailhip.so.
 *   materials_dynamic_c          the argument checks that need no GPU (tests/test_materials_dynamic_host.py)
 *   materials_dynamic_c gpu      create, rebuild, render a 32 x 32 image, an identity update, render again and compare
 *                                (tests/test_gpu_materials_dynamic.py) -- device memory through the HIP runtime's C interface, declared here */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/snail_materials_dynamic.h"
#include "../../include/snail_materials.h"

#define ADDR(f) (void (*)(void))f,

/* the three functions of the HIP runtime this program needs (libamdhip64, which libsnailhip.so brings along) */
extern int hipMalloc(void **ptr, size_t size);
extern int hipMemcpy(void *dst, const void *src, size_t size, int kind);
extern int hipDeviceSynchronize(void);
#define H2D 1
#define D2H 2

static void *upload(const void *src, size_t bytes) {
	void *d = NULL;
	if(hipMalloc(&d, bytes) != 0 || hipMemcpy(d, src, bytes, H2D) != 0) { printf("device copy failed\n"); exit(20); }
	return d;
}

static int gpu(void) {
	/* a 6 x 6 sheet of quads in front of the camera, bent by `bend` */
	enum { N = 6, NT = N * N * 2, RES = 32 };
	static float verts[2][NT * 9], uv[NT * 6];
	static int32_t matIdx[NT];
	static uint8_t flat[NT], img[2][RES * RES * 3];
	int pose, i, j, k, t = 0;
	for(pose = 0; pose < 2; pose++) {
		t = 0;
		for(i = 0; i < N; i++)
			for(j = 0; j < N; j++) {
				const float bend = pose ? 0.35f : 0.1f;
				float q[4][3];
				const int ci[4] = {i, i + 1, i + 1, i}, cj[4] = {j, j, j + 1, j + 1};
				const int order[6] = {0, 1, 2, 0, 2, 3};
				for(k = 0; k < 4; k++) {
					q[k][0] = -1.5f + 0.5f * (float)ci[k]; q[k][1] = -1.5f + 0.5f * (float)cj[k];
					q[k][2] = 3.0f + bend * (float)((ci[k] * 7 + cj[k] * 3) % 5);
				}
				for(k = 0; k < 6; k++) {
					memcpy(&verts[pose][(t + k / 3) * 9 + (k % 3) * 3], q[order[k]], 12);
					uv[(t + k / 3) * 6 + (k % 3) * 2] = 0.25f * (float)ci[order[k]];
					uv[(t + k / 3) * 6 + (k % 3) * 2 + 1] = 0.25f * (float)cj[order[k]];
				}
				matIdx[t] = (i + j) % 3; matIdx[t + 1] = (i + 2 * j) % 3;
				flat[t] = (uint8_t)(i & 1); flat[t + 1] = 0;
				t += 2;
			}
	}
	{
		static uint8_t texels[8 * 8 * 3], levels[8 * 8 * 3 * 2];
		const float cam[13] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 1.0f}, amb[3] = {0.2f, 0.2f, 0.2f};
		const float lights[7] = {0.5f, 1.0f, 0.0f, 1.0f, 0.9f, 0.8f, 30.0f};
		const int32_t map[3] = {-1, 0, 1};
		SnailMaterial mats[2];
		SnailTexture tex;
		int32_t info[6] = {-1, -1, -1, -1, -1, -1}, info2[2] = {-1, -1};
		uint64_t stats[4] = {0, 0, 0, 0};
		float *dV[2], *dUV;
		int32_t *dMat, *dPerm, *dInfo;
		uint8_t *dFlat;
		SnailScene *sc;
		SnailMaterials *ms;
		int levelsN = 0;
		for(i = 0; i < 8 * 8 * 3; i++) texels[i] = (uint8_t)(40 + (i * 37) % 200);
		if(snail_texture_size(8, 8, NULL) > (int64_t)sizeof(levels) || snail_texture_build(texels, 8, 8, levels, (int64_t)sizeof(levels), &levelsN) != 0) return 21;
		memset(mats, 0, sizeof(mats));
		mats[0].kind = SNAIL_MAT_TEX; mats[0].nDotR = 1; mats[0].texture = 0;
		mats[1].kind = SNAIL_MAT_SIMPLE; mats[1].diffuse[0] = 0.9f; mats[1].diffuse[1] = 0.4f; mats[1].diffuse[2] = 0.2f;
		tex.levels = levels; tex.width = 8; tex.height = 8;
		dV[0] = (float *)upload(verts[0], sizeof(verts[0])); dV[1] = (float *)upload(verts[1], sizeof(verts[1]));
		dUV = (float *)upload(uv, sizeof(uv)); dMat = (int32_t *)upload(matIdx, sizeof(matIdx)); dFlat = (uint8_t *)upload(flat, sizeof(flat));
		dPerm = (int32_t *)upload(matIdx, sizeof(matIdx)); dInfo = (int32_t *)upload(info, sizeof(info));
		sc = snail_scene_create_fast_dev(dV[0], NT, 0, dPerm, NULL, NULL);
		if(!sc) { printf("create scene: %s\n", snail_last_error()); return 22; }
		/* refused: a perm that was never given, then the real thing with face normals */
		if(snail_materials_create_dev(sc, dUV, dMat, dFlat, NT, NULL, NULL, dV[0], map, 3, mats, 2, NULL, &tex, 1, NULL) != NULL) return 23;
		ms = snail_materials_create_dev(sc, dUV, dMat, dFlat, NT, dPerm, NULL, dV[0], map, 3, mats, 2, NULL, &tex, 1, NULL);
		if(!ms) { printf("create set: %s\n", snail_last_error()); return 24; }
		if(snail_materials_rebuild_dev(ms, dV[1], NULL, dPerm, dInfo, NULL) != 0) { printf("rebuild: %s\n", snail_last_error()); return 25; }
		if(snail_render_materials_image(ms, cam, RES, RES, lights, 1, amb, 0, img[0], RES * 3, stats) != 0) { printf("render: %s\n", snail_last_error()); return 26; }
		if(hipMemcpy(info, dInfo, sizeof(info), D2H) != 0 || info[0] != 0 || info[3] != NT || info[4] != 1 || info[5] != 0) {
			printf("info %d %d %d %d %d %d\n", info[0], info[1], info[2], info[3], info[4], info[5]);
			return 27;
		}
		/* an identity update: the same perm, the same vertices -> the same records, the same image */
		if(snail_materials_update_dev(ms, dPerm, NULL, dV[1], dInfo, NULL) != 0) { printf("update: %s\n", snail_last_error()); return 28; }
		if(snail_render_materials_image(ms, cam, RES, RES, lights, 1, amb, 0, img[1], RES * 3, stats) != 0) { printf("render 2: %s\n", snail_last_error()); return 29; }
		if(hipMemcpy(info2, dInfo, sizeof(info2), D2H) != 0 || info2[0] != 1 || info2[1] != 0) return 30;
		if(memcmp(img[0], img[1], sizeof(img[0])) != 0) return 31;
		for(i = 0, k = 0; i < RES * RES * 3; i++) k += img[0][i] != img[0][0];
		if(k == 0) return 32;   /* (an image of one byte value would compare equal whatever the records hold) */
		/* a rebuild behind the set's back: the next frame is refused by a text naming the rebuild, and an update brings it back */
		if(snail_scene_rebuild_fast_dev(sc, dV[0], NT, dPerm, NULL, NULL) != 0) return 33;
		if(snail_render_materials_image(ms, cam, RES, RES, lights, 1, amb, 0, img[1], RES * 3, stats) == 0 || !strstr(snail_last_error(), "rebuilt")) return 34;
		if(snail_materials_update_dev(ms, dPerm, NULL, dV[0], NULL, NULL) != 0) return 35;
		if(snail_render_materials_image(ms, cam, RES, RES, lights, 1, amb, 0, img[1], RES * 3, stats) != 0) return 36;
		if(hipDeviceSynchronize() != 0) return 37;
		snail_materials_destroy(ms);
		snail_scene_destroy(sc);
		printf("C materials dynamic frames ok: %d differing bytes inside the image\n", k);
	}
	return 0;
}

int main(int argc, char **argv) {
	void (*fns[])(void) = { ADDR(snail_materials_create_dev) ADDR(snail_materials_rebuild_dev) ADDR(snail_materials_update_dev) };
	const int32_t map[1] = {-1};
	float dummy[9] = {0};
	int32_t perm[1] = {0};
	if(argc > 1 && strcmp(argv[1], "gpu") == 0) return gpu();
	/* before any device call: the null arrays, the host-side material data (the creators' shared check), the handles */
	if(snail_materials_create_dev(NULL, dummy, perm, NULL, 1, NULL, dummy, NULL, map, 1, NULL, 0, NULL, NULL, 0, NULL) != NULL || !strstr(snail_last_error(), "perm")) return 2;
	if(snail_materials_create_dev(NULL, dummy, perm, NULL, 1, perm, NULL, NULL, map, 1, NULL, 0, NULL, NULL, 0, NULL) != NULL || !strstr(snail_last_error(), "normals")) return 3;
	if(snail_materials_create_dev(NULL, dummy, perm, NULL, 1, perm, dummy, NULL, map, 0, NULL, 0, NULL, NULL, 0, NULL) != NULL || !strstr(snail_last_error(), "map entry")) return 4;
	if(snail_materials_create_dev(NULL, dummy, perm, NULL, 1, perm, dummy, NULL, map, 1, NULL, 0, NULL, NULL, 0, NULL) != NULL || !strstr(snail_last_error(), "scene handle")) return 5;
	if(snail_materials_rebuild_dev(NULL, dummy, NULL, NULL, NULL, NULL) == 0 || !strstr(snail_last_error(), "material set handle")) return 6;
	if(snail_materials_update_dev(NULL, perm, dummy, NULL, NULL, NULL) == 0 || !strstr(snail_last_error(), "material set handle")) return 7;
	printf("C materials dynamic ABI ok: %d symbols\n", (int)(sizeof(fns) / sizeof(fns[0])));
	return 0;
}
