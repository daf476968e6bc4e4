// bvh_fast_commit_body.inc -- the body of k_fast_commit (bvh_fast.inc) as TEXT, included inside the kernel that runs it (as
// materials_mirror_body.inc is): the single-tree kernel and the batched one of bvh_fast_batch.inc compile the same statements, and the single-tree
// kernel's code stays what it was before the batched builder existed (a __device__ function taking the record by reference came out with other
// register counts).  The including kernel provides A, the tree's argument record,
// and the macros SNAIL_BODY_BLOCK / SNAIL_BODY_GRID: the workgroup's index and the number of workgroups WITHIN THE TREE'S SHARE of the launch
// (blockIdx.x / gridDim.x when the launch serves one tree).
	const BuildHdr &H = *A.hdr;
	const int g = SNAIL_BODY_BLOCK * blockDim.x + threadIdx.x, stride = SNAIL_BODY_GRID * blockDim.x;
	const int status = H.status != 0 ? H.status : (A.needSane && H.insane) ? 3 : 0;
	if(status != 0) {
		if(g == 0 && A.info) { A.info[0] = status; A.info[1] = 0; A.info[2] = 0; A.info[3] = A.n; }
		return;
	}
	const int nTemp = H.nTemp;
	for(int t = g; t < nTemp; t += stride) {
		const TNode nd = A.tn[t];
		const int idx = t == 0 ? 0 : 1 + 2 * (A.startCnt[nd.pfirst] + nd.pchain) + nd.side;
		const unsigned sub = nd.inner ? (unsigned)(1 + 2 * (A.startCnt[nd.first] + nd.chain)) : ((unsigned)nd.first | 0x80000000u);
		const unsigned in[8] = {__float_as_uint(nd.lo[0]), __float_as_uint(nd.lo[1]), __float_as_uint(nd.lo[2]), __float_as_uint(nd.hi[0]),
								__float_as_uint(nd.hi[1]), __float_as_uint(nd.hi[2]), sub, (unsigned)nd.aux};
		A.nodes[(size_t)idx * 2] = make_uint4(in[0], in[1], in[2], in[3]);
		A.nodes[(size_t)idx * 2 + 1] = make_uint4(in[4], in[5], in[6], in[7]);
		if(A.pf) {
			unsigned out[8];
			dev::pfEncode(in, out, A.trisOff);
			A.pf[(size_t)(idx + 1) * 2] = make_uint4(out[0], out[1], out[2], out[3]);
			A.pf[(size_t)(idx + 1) * 2 + 1] = make_uint4(out[4], out[5], out[6], out[7]);
		}
	}
	for(int i = g; i < A.n; i += stride) {
		const int s = A.src[i];
		float p[9], rec[16];
		for(int k = 0; k < 9; k++) p[k] = A.verts[(size_t)s * 9 + k];
		(void)dev::lbvh::triRecord(p, rec);
		uint4 *o = A.tris + (size_t)i * 4;
		for(int q = 0; q < 4; q++)
			o[q] = make_uint4(__float_as_uint(rec[q * 4]), __float_as_uint(rec[q * 4 + 1]), __float_as_uint(rec[q * 4 + 2]), __float_as_uint(rec[q * 4 + 3]));
		if(A.perm) A.perm[i] = s;
	}
	if(g == 0) {
		const int nNodes = 1 + 2 * H.totalInner;
		A.cur[0] = nNodes; A.cur[1] = H.depth; A.cur[2] = H.insane ? 0 : 1; A.cur[3] = 0;
		if(A.info) { A.info[0] = 0; A.info[1] = nNodes; A.info[2] = H.depth; A.info[3] = A.n; }
	}
