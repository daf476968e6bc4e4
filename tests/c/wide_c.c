/* The entry points of include/snail_wide.h as PLAIN C (gcc -std=c99 -Wall -Werror -pedantic): every function links against
 * libsnailhip.so, and the refusals that need no GPU -- the arguments are judged before the handle is looked at -- are made with their
 * texts (tests/test_wide_host.py). */
#include <stdio.h>
#include <string.h>

#include "../../include/snail_wide.h"

#define ADDR(f) (void (*)(void))f,

static int refused(int rc, const char *text) {
	if(rc != 0 && strstr(snail_last_error(), text)) return 1;
	printf("rc %d, \"%s\" lacks \"%s\"\n", rc, snail_last_error(), text);
	return 0;
}

int main(void) {
	void (*wide[])(void) = { ADDR(snail_wide_trace_dev) ADDR(snail_wide_trace) ADDR(snail_photons_trace_dev) ADDR(snail_photons_trace) };
	float f[21] = {0};
	int32_t idx[2] = {0, 1}, vis[4], n = 7;
	uint64_t st[2] = {0, 0};
	SnailPhoton ph[2];
	if(sizeof(SnailPhoton) != 32) { printf("SnailPhoton is %d bytes\n", (int)sizeof(SnailPhoton)); return 20; }
	/* the walk: negative counts, null required buffers, a negative start node -- all with a null handle, which is reported last */
	if(!refused(snail_wide_trace_dev(NULL, -1, f, f, NULL, NULL, 0, f, 0, NULL, NULL, NULL), "snail_wide_trace_dev: negative count")) return 1;
	if(!refused(snail_wide_trace_dev(NULL, 2, f, f, NULL, idx, -2, f, 0, NULL, NULL, NULL), "negative count")) return 2;
	if(!refused(snail_wide_trace_dev(NULL, 2, NULL, f, NULL, NULL, 0, f, 0, NULL, NULL, NULL), "null ray array")) return 3;
	if(!refused(snail_wide_trace_dev(NULL, 2, f, NULL, NULL, NULL, 0, f, 0, NULL, NULL, NULL), "null ray array")) return 4;
	if(!refused(snail_wide_trace_dev(NULL, 2, f, f, NULL, NULL, 0, NULL, 0, NULL, NULL, NULL), "null ray array")) return 5;
	if(!refused(snail_wide_trace_dev(NULL, 2, f, f, NULL, NULL, 0, f, -1, NULL, NULL, NULL), "startNode -1 outside the tree")) return 6;
	if(!refused(snail_wide_trace_dev(NULL, 2, f, f, NULL, NULL, 0, f, 0, vis, st, NULL), "snail_wide_trace_dev: invalid scene handle")) return 7;
	if(snail_wide_trace_dev(NULL, 0, NULL, NULL, NULL, NULL, 0, NULL, 0, NULL, NULL, NULL) != 0) return 8;   /* no ray: nothing to do */
	if(!refused(snail_wide_trace(NULL, -3, f, f, NULL, NULL, 0, f, 0, NULL, NULL), "snail_wide_trace: negative count")) return 9;
	if(!refused(snail_wide_trace(NULL, 2, f, f, f, idx, 2, NULL, 0, NULL, NULL), "null ray array")) return 10;
	if(!refused(snail_wide_trace(NULL, 2, f, f, f, idx, 2, f, -5, NULL, NULL), "startNode -5 outside the tree")) return 11;
	if(!refused(snail_wide_trace(NULL, 2, f, f, f, idx, 2, f, 0, vis, st), "snail_wide_trace: invalid scene handle")) return 12;
	if(snail_wide_trace(NULL, 0, NULL, NULL, NULL, NULL, 0, NULL, 0, NULL, NULL) != 0) return 13;
	/* the photon pass: the number of lights, the count, the buffers */
	if(!refused(snail_photons_trace_dev(NULL, -1, 1, f, f, f, ph, &n, NULL, NULL), "snail_photons_trace_dev: -1 lights outside 0..8")) return 14;
	if(!refused(snail_photons_trace_dev(NULL, SNAIL_MAX_LIGHTS + 1, 1, f, f, f, ph, &n, NULL, NULL), "9 lights outside 0..8")) return 15;
	if(!refused(snail_photons_trace_dev(NULL, 1, -1, f, f, f, ph, &n, NULL, NULL), "negative count")) return 16;
	if(!refused(snail_photons_trace_dev(NULL, 1, 1, f, f, f, ph, NULL, NULL, NULL), "null photon count")) return 17;
	if(!refused(snail_photons_trace_dev(NULL, 1, 1, NULL, f, f, ph, &n, NULL, NULL), "null buffer")) return 18;
	if(!refused(snail_photons_trace_dev(NULL, 1, 1, f, f, NULL, ph, &n, NULL, NULL), "null buffer")) return 19;
	if(!refused(snail_photons_trace_dev(NULL, 1, 1, f, f, f, NULL, &n, NULL, NULL), "null buffer")) return 21;
	if(!refused(snail_photons_trace_dev(NULL, 1, 1, f, f, f, ph, &n, NULL, NULL), "snail_photons_trace_dev: invalid scene handle")) return 22;
	if(!refused(snail_photons_trace(NULL, 9, 1, f, f, f, ph, &n, st), "snail_photons_trace: 9 lights outside 0..8")) return 23;
	if(!refused(snail_photons_trace(NULL, 2, -4, f, f, f, ph, &n, st), "negative count")) return 24;
	if(!refused(snail_photons_trace(NULL, 2, 1, f, NULL, f, ph, &n, st), "null buffer")) return 25;
	if(!refused(snail_photons_trace(NULL, 2, 1, f, f, f, ph, &n, st), "snail_photons_trace: invalid scene handle")) return 26;
	if(n != 7) return 27;   /* a refused call writes nothing */
	printf("C wide ABI ok: %d symbols\n", (int)(sizeof(wide) / sizeof(wide[0])));
	return 0;
}
