// instances_materials_trace_level_body.inc -- the body of k_imat_trace_level<DEEP> / k_imat_trace_level_heat<DEEP>
// (instances_materials_transparency.inc), included into each kernel with SNAIL_TRACE_LEVEL_PSTATS 0 / 1.  Text, not an inlined function template,
// as materials_mirror_body.inc is: with the body moved into a template <bool DEEP, bool PSTATS> device function, the resource report of
// k_imat_trace_level itself moved (219 -> 221 and 221 -> 223 VGPRs, scalar spills 22 -> 18, in the table arithmetic 37 -> 27), whichever way the
// record and the LDS array were handed over, and the kernels of today's launches stay the code they were (DESIGN.md section 7).  ILevelArgs L is the
// kernel's argument, DEEP its template argument.
	__shared__ float lds[LDS_FLOATS_PER_WAVE];
	const InstArgs &A = L.i;
	const int lane = threadIdx.x & 63;
	const int p = (int)blockIdx.x;
	if(p >= A.nPackets || orderSkipped(L.order, p)) return;
	const int size = A.size;
	const bool live = lane < size;
	const size_t q = (size_t)p * size + (live ? lane : 0);
	float d[3][4], id[3][4], org[3][4];
	loadQuad3(A.dir, q, d);
	loadQuad3(A.idir, q, id);
	loadQuad3(A.origin, q, org);
	const unsigned mask4 = A.mask[q] & 15u;
	const float4 dv = *(const float4 *)(A.distance + q * 4);
	const int4 ov = *(const int4 *)(A.object + q * 4), ev = *(const int4 *)(A.element + q * 4);
	float dist[4] = {dv.x, dv.y, dv.z, dv.w};
	int obj[4] = {ov.x, ov.y, ov.z, ov.w}, elem[4] = {ev.x, ev.y, ev.z, ev.w};
	float bu[4], bv[4];
	{
		const float4 b0 = *(const float4 *)(A.bary + q * 8), b1 = *(const float4 *)(A.bary + q * 8 + 4);
		bu[0] = b0.x; bu[1] = b0.y; bu[2] = b0.z; bu[3] = b0.w;
		bv[0] = b1.x; bv[1] = b1.y; bv[2] = b1.z; bv[3] = b1.w;
	}
	Counters st = {0, 0, 0, 0, 0};
	instWalk<false, true, false, true, DEEP>(A, size, lane, org, d, id, mask4, dist, obj, elem, bu, bv, lds, st);
	flushStats(A.stats, st, 0u, lane);
#if SNAIL_TRACE_LEVEL_PSTATS
	bookPacket(A.pstats, (size_t)p, st, 0u, lane);
#endif
	if(live) {
		*(float4 *)(A.distance + q * 4) = make_float4(dist[0], dist[1], dist[2], dist[3]);
		*(int4 *)(A.object + q * 4) = make_int4(obj[0], obj[1], obj[2], obj[3]);
		*(int4 *)(A.element + q * 4) = make_int4(elem[0], elem[1], elem[2], elem[3]);
		*(float4 *)(A.bary + q * 8) = make_float4(bu[0], bu[1], bu[2], bu[3]);
		*(float4 *)(A.bary + q * 8 + 4) = make_float4(bv[0], bv[1], bv[2], bv[3]);
	}
