// build_small_body.inc -- the body of k_build_small (build_common.inc) as TEXT, included inside the kernel that runs it (as
// materials_mirror_body.inc is): the single-tree kernel and the batched one of bvh_fast_batch.inc compile the same statements, and the single-tree
// kernel's code stays what it was before the batched builder existed (a __device__ function taking the record by reference came out with other
// register counts).  The including kernel provides A, the tree's argument record; the policy P, the __shared__ SplitLds S and int stack[kLevels + 8],
// and the macros SNAIL_BODY_BLOCK / SNAIL_BODY_GRID: the workgroup's index and the number of workgroups WITHIN THE TREE'S SHARE of the launch
// (blockIdx.x / gridDim.x when the launch serves one tree).
	BuildHdr &H = *A.hdr;
	if(H.status == 1) return;
	const int cnt = H.nSmall;
	for(int item = SNAIL_BODY_BLOCK; item < cnt; item += SNAIL_BODY_GRID) {
		__syncthreads();
		if(threadIdx.x == 0) stack[0] = A.small[item];
		int sp = 1;
		while(sp > 0) {
			__syncthreads();
			const int t = stack[--sp];
			__syncthreads();
			splitNode<64, P>(A, t, S);
			// (the children of a node at depth d sit at d + 1 <= 64 and none is made below that: at most one pending sibling per level)
			const int c = S.child;
			if(c >= 0) {
				if(S.cR >= P::minSplit && sp < kLevels + 6) { if(threadIdx.x == 0) stack[sp] = c + 1; sp++; }
				if(S.cL >= P::minSplit && sp < kLevels + 6) { if(threadIdx.x == 0) stack[sp] = c; sp++; }
			}
		}
	}
