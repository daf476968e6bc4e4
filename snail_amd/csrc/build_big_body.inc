// build_big_body.inc -- the body of k_build_big (build_common.inc) as TEXT, included inside the kernel that runs it (as
// materials_mirror_body.inc is): the single-tree kernel and the batched one of bvh_fast_batch.inc compile the same statements, and the single-tree
// kernel's code stays what it was before the batched builder existed (a __device__ function taking the record by reference came out with other
// register counts).  The including kernel provides A, the tree's argument record; the policy P, level0, level1, the __shared__ SplitLds S and int levelCount,
// and the macros SNAIL_BODY_BLOCK / SNAIL_BODY_GRID: the workgroup's index and the number of workgroups WITHIN THE TREE'S SHARE of the launch
// (blockIdx.x / gridDim.x when the launch serves one tree).
	BuildHdr &H = *A.hdr;
	if(H.status == 1) return;
	for(int level = level0; level < level1; level++) {
		__syncthreads();
		if(threadIdx.x == 0) levelCount = atomicAdd(&H.qCount[level], 0);   // (read where this workgroup's own atomics of the level before landed)
		__syncthreads();
		const int cnt = levelCount;
		if(cnt == 0) return;      // no node of this depth: none deeper either
		const int *in = A.queue[level & 1];
		int *out = A.queue[(level + 1) & 1];
		for(int item = SNAIL_BODY_BLOCK; item < cnt; item += SNAIL_BODY_GRID) {
			__syncthreads();
			splitNode<256, P>(A, in[item], S);
			if(threadIdx.x == 0 && S.child >= 0) {
				const int id[2] = {S.child, S.child + 1}, c[2] = {S.cL, S.cR};
				for(int s = 0; s < 2; s++) {
					if(c[s] > kSmall) out[atomicAdd(&H.qCount[level + 1], 1)] = id[s];
					else if(c[s] >= P::minSplit) A.small[atomicAdd(&H.nSmall, 1)] = id[s];
				}
			}
		}
	}
