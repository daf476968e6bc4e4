// materials_mirror_body.inc -- the body of k_mat_mirror / k_mat_mirror_heat (materials.inc), included into each kernel with SNAIL_MIRROR_PSTATS 0 / 1.
// Text, not an inlined function template: with the body moved into one, the resource report of k_mat_mirror itself moved (47 -> 50 VGPRs, in the
// table arithmetic 48 -> 54), and the kernels of today's launches stay the code they were (DESIGN.md section 7).  MatArgs A is the kernel's argument.
	const int lane = threadIdx.x & 63;
	const int li = (int)blockIdx.x;
	if(li >= A.s.nPackets) return;
	const PacketPos P = packetOf(A.s, li);
	const size_t quad = P.pidx * 64 + lane;
	const float inf = __builtin_inff();
	Samples S;
	float d[3][4];
	matRays(A.s, P, lane, d);
	matLoadSamples<SRC_PRIMARY>(A, P, lane, S);
	float rd[3][4], ro[3][4], rdist[4];
	unsigned sel = 0;
#pragma unroll
	for(int l = 0; l < 4; l++) {
		const float dt = S.nrm[0][l] * d[0][l] + S.nrm[1][l] * d[1][l] + S.nrm[2][l] * d[2][l];
		const float dt2 = dt + dt;
#pragma unroll
		for(int c = 0; c < 3; c++) {
			const float r = d[c][l] - S.nrm[c][l] * dt2;
			rd[c][l] = S.hit[l] ? r : 0.0f;
			ro[c][l] = S.hit[l] ? S.pos[c][l] + r * 0.001f : 0.0f;
		}
		rdist[l] = S.hit[l] ? inf : -inf;
		sel |= S.hit[l] ? (1u << l) : 0u;
	}
	float4 *po = (float4 *)(A.s.rOrg + quad * 12), *pd = (float4 *)(A.s.rDir + quad * 12), *pi = (float4 *)(A.s.rIDir + quad * 12);
#pragma unroll
	for(int c = 0; c < 3; c++) {
		po[c] = make_float4(ro[c][0], ro[c][1], ro[c][2], ro[c][3]);
		pd[c] = make_float4(rd[c][0], rd[c][1], rd[c][2], rd[c][3]);
	}
#pragma unroll
	for(int c = 0; c < 3; c++) {   // SafeInv (src/rtbase.h:117-120); table arithmetic: a component's four look-ups in one batch
		float x4[4], r4[4];
#pragma unroll
		for(int l = 0; l < 4; l++) x4[l] = rd[c][l] + 0.00000001f;
#if SNAIL_ARITH_SSE
		InvN<4>(x4, r4);
#else
#pragma unroll
		for(int l = 0; l < 4; l++) r4[l] = Inv(x4[l]);
#endif
		pi[c] = make_float4(r4[0], r4[1], r4[2], r4[3]);
	}
	A.s.rMask[quad] = (unsigned char)sel;
	*(float4 *)(A.s.rDist + quad * 4) = make_float4(rdist[0], rdist[1], rdist[2], rdist[3]);
	*(int4 *)(A.s.rObj + quad * 4) = make_int4(0, 0, 0, 0);
	unsigned cnt = 0;
#pragma unroll
	for(int l = 0; l < 4; l++) cnt += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(S.hit[l]));
	const Counters none = {0, 0, 0, 0, 0};
	flushStats(A.s.stats, none, cnt, lane);
#if SNAIL_MIRROR_PSTATS
	bookPacketLate<ShadeArgs>(P.pidx, none, cnt, lane);
#endif
