// dbvh_build.cpp -- host-side top-level tree over rigid instances: the reference's DBVH::Construct / FindSplit
// (src/dbvh/tree.cpp:23-172) and ObjectInstance::ComputeBBox (:4-21), with the reference's exact fp32 operation order.
//
// The instance id a hit reports is the instance's slot in the builder's array, which std::partition reorders
// (src/dbvh/tree.cpp:117-118), so the element order is part of the contract.  The partition is restated here in
// the form libstdc++ runs for bidirectional iterators (bits/stl_algo.h __partition: skip true from the front, skip
// false from the back, swap, repeat) instead of relying on whatever the C++ library at hand does.
//
// One deliberate deviation: when the node's extent on the split axis is 0 or not finite, the reference computes
// (c - sub) * mul = 0 * inf or x * 0 and indexes bins[int(NaN)] (undefined behaviour).  Here a bin index that is
// NaN or below 0 is bin 0 and one above the last bin is the last bin -- in the binning and in the partition
// predicate alike.  With coincident centres every instance lands in bin 0, one side of the split is empty and the
// reference's median split follows.  Nodes use the 32-byte record of the BVH (DBVH::Node, src/dbvh/tree.h:125-133).
#include "../../include/snail_instances.h"

#include <cmath>
#include <cstring>
#include <vector>

extern void snail_set_error(const char *fmt, ...);

namespace snail_dbvh {

struct Node32 { float bmin[3], bmax[3]; uint32_t sub; int32_t aux; };
static_assert(sizeof(Node32) == 32, "DBVH::Node is 32 bytes");

static inline float fmin2(float a, float b) { return a < b ? a : b; } // veclib/vecbase.h:75-76, _mm_min_ps / _mm_max_ps
static inline float fmax2(float a, float b) { return a > b ? a : b; }

struct Box {
	float lo[3], hi[3];
	void add(const Box &o) { // BBox::operator+= (src/bounding_box.h:21-25)
		for(int k = 0; k < 3; k++) { lo[k] = fmin2(lo[k], o.lo[k]); hi[k] = fmax2(hi[k], o.hi[k]); }
	}
	float area() const { // BoxSA (src/dbvh/tree.cpp:40-42): (Width * (Depth + Height) + Depth * Height) * 2
		const float w = hi[0] - lo[0], h = hi[1] - lo[1], d = hi[2] - lo[2];
		return (w * (d + h) + d * h) * 2.0f;
	}
	float center(int a) const { return (lo[a] + hi[a]) * 0.5f; }
};

// ObjectInstance::ComputeBBox (src/dbvh/tree.cpp:4-21); r = rows of the rotation, t = translation, b = the BLAS root box
static Box instanceBox(const float *xf12, const float *b6) {
	const float *r0 = xf12, *r1 = xf12 + 3, *r2 = xf12 + 6, *t = xf12 + 9;
	const float *r[3] = {r0, r1, r2};
	const float x0 = b6[0], x1 = b6[3];
	const float y[4] = {b6[1], b6[1], b6[4], b6[4]}, z[4] = {b6[2], b6[5], b6[2], b6[5]};
	Box out;
	for(int c = 0; c < 3; c++) {
		float p0[4], p1[4], mn[4], mx[4];
		for(int l = 0; l < 4; l++) {
			p0[l] = y[l] * r[c][1] + z[l] * r[c][2];
			p1[l] = x1 * r[c][0] + p0[l];
			p0[l] = p0[l] + x0 * r[c][0];
			mn[l] = fmin2(p0[l], p1[l]);
			mx[l] = fmax2(p0[l], p1[l]);
		}
		// Minimize / Maximize (src/rtbase_math.h:63-64)
		out.lo[c] = fmin2(fmin2(mn[0], mn[1]), fmin2(mn[2], mn[3])) + t[c];
		out.hi[c] = fmax2(fmax2(mx[0], mx[1]), fmax2(mx[2], mx[3])) + t[c];
	}
	return out;
}

// int((c - sub) * mul) with the defined deviation above
static inline int binOf(float c, float sub, float mul, int nBins) {
	const float v = (c - sub) * mul;
	if(!(v >= 0.0f)) return 0;
	if(!(v < (float)nBins)) return nBins - 1;
	return (int)v;
}

struct Builder {
	std::vector<Box> box;    // per builder slot
	std::vector<int32_t> src;  // builder slot -> caller's instance
	Node32 *nodes = nullptr;
	int nNodes = 0, depth = 0;

	void leaf(int nNode, int first, int count, int sdepth) {
		depth = depth > sdepth ? depth : sdepth;
		nodes[nNode].sub = (uint32_t)first | 0x80000000u;
		nodes[nNode].aux = count;
	}
	int push(const Box &b) {
		Node32 &n = nodes[nNodes];
		for(int k = 0; k < 3; k++) { n.bmin[k] = b.lo[k]; n.bmax[k] = b.hi[k]; }
		n.sub = 0; n.aux = 0;
		return nNodes++;
	}
	// DBVH::FindSplit (src/dbvh/tree.cpp:46-152); an explicit stack keeps the reference's pre-order numbering
	void run(int n) {
		struct Job { int node, first, count, depth; };
		std::vector<Job> stack;
		stack.push_back({0, 0, n, 0});
		while(!stack.empty()) {
			const Job j = stack.back();
			stack.pop_back();
			split(j.node, j.first, j.count, j.depth, stack);
		}
	}
	template <class Stack>
	void split(int nNode, int first, int count, int sdepth, Stack &stack) {
		if(count <= 1) { leaf(nNode, first, count, sdepth); return; }
		Box bbox;
		for(int k = 0; k < 3; k++) { bbox.lo[k] = nodes[nNode].bmin[k]; bbox.hi[k] = nodes[nNode].bmax[k]; }
		float size[3];
		for(int k = 0; k < 3; k++) size[k] = bbox.hi[k] - bbox.lo[k];
		const int axis = size[1] > size[0] ? (size[2] > size[1] ? 2 : 1) : (size[2] > size[0] ? 2 : 0); // MaxAxis, src/rtbase.h:136-138
		const int nBins = count < 8 ? 8 : 16;
		const float inf = INFINITY;
		Box bins[16];
		int binCount[16];
		for(int b = 0; b < nBins; b++) {
			for(int k = 0; k < 3; k++) { bins[b].lo[k] = inf; bins[b].hi[k] = -inf; }
			binCount[b] = 0;
		}
		const float mul = (float)nBins * (1.0f - 0.0001f) / (bbox.hi[axis] - bbox.lo[axis]);
		const float sub = bbox.lo[axis];
		for(int i = 0; i < count; i++) {
			const Box &b = box[first + i];
			const float c = (b.hi[axis] + b.lo[axis]) * 0.5f;
			const int bin = binOf(c, sub, mul, nBins);
			binCount[bin]++;
			bins[bin].add(b);
		}
		Box leftBoxes[16], rightBoxes[16];
		int leftCounts[16], rightCounts[16];
		rightBoxes[nBins - 1] = bins[nBins - 1]; rightCounts[nBins - 1] = binCount[nBins - 1];
		leftBoxes[0] = bins[0]; leftCounts[0] = binCount[0];
		for(int b = 1; b < nBins; b++) {
			leftBoxes[b] = leftBoxes[b - 1]; leftBoxes[b].add(bins[b]);
			leftCounts[b] = leftCounts[b - 1] + binCount[b];
		}
		for(int b = nBins - 2; b >= 0; b--) {
			rightBoxes[b] = rightBoxes[b + 1]; rightBoxes[b].add(bins[b]);
			rightCounts[b] = rightCounts[b + 1] + binCount[b];
		}
		float minCost = inf;
		const float noSplitCost = 1.0f * (float)count * bbox.area();
		int minIdx = 1;
		for(int b = 1; b < nBins; b++) {
			const float cost = (leftCounts[b - 1] ? leftBoxes[b - 1].area() * (float)leftCounts[b - 1] : 0.0f) +
							   (rightCounts[b] ? rightBoxes[b].area() * (float)rightCounts[b] : 0.0f);
			if(cost < minCost) { minCost = cost; minIdx = b; }
		}
		minCost = 0.0f + 1.0f * minCost;
		if(noSplitCost < minCost) { leaf(nNode, first, count, sdepth); return; }

		// std::partition(&elements[first], &elements[first + count], TestBoxes(...)), libstdc++'s bidirectional form
		{
			auto pred = [&](int i) { return binOf(box[i].center(axis), sub, mul, nBins) < minIdx; };
			int lo = first, hi = first + count;
			for(;;) {
				for(;;) {
					if(lo == hi) goto PARTITIONED;
					if(pred(lo)) lo++;
					else break;
				}
				hi--;
				for(;;) {
					if(lo == hi) goto PARTITIONED;
					if(!pred(hi)) hi--;
					else break;
				}
				std::swap(box[lo], box[hi]);
				std::swap(src[lo], src[hi]);
				lo++;
			}
		PARTITIONED:;
		}
		Box leftBox = leftBoxes[minIdx - 1], rightBox = rightBoxes[minIdx];
		int leftCount = leftCounts[minIdx - 1], rightCount = rightCounts[minIdx];
		if(leftCount == 0 || rightCount == 0) { // median split over the partitioned order (:123-134)
			const int mid = count / 2;
			leftBox = box[first];
			rightBox = box[first + count - 1];
			for(int i = 1; i < mid; i++) leftBox.add(box[first + i]);
			for(int i = mid; i < count; i++) rightBox.add(box[first + i]);
			leftCount = mid;
			rightCount = count - leftCount;
		}
		const int subNode = nNodes;
		// only the second assignment of firstNode survives (:141-143)
		const int firstNode = leftBox.lo[axis] == rightBox.lo[axis] ? (leftBox.hi[axis] < rightBox.hi[axis] ? 0 : 1) : 0;
		nodes[nNode].sub = (uint32_t)subNode;
		nodes[nNode].aux = (int32_t)((uint32_t)axis | ((uint32_t)firstNode << 16));
		push(leftBox);
		push(rightBox);
		// FindSplit(left) runs before FindSplit(right): the right job goes on the stack first
		stack.push_back({subNode + 1, first + leftCount, rightCount, sdepth + 1});
		stack.push_back({subNode + 0, first, leftCount, sdepth + 1});
	}
};

} // namespace snail_dbvh

extern "C" int snail_instances_build(const float *xf12, const int32_t *blasIdx, int n, const float *blasBBox6, int nBlas, void *nodes32,
									 int *nNodes, int *depth, int32_t *perm) {
	using namespace snail_dbvh;
	if(n <= 0 || n > (1 << 30) || !xf12 || !blasIdx || nBlas <= 0 || !blasBBox6 || !nodes32 || !nNodes || !depth) {
		snail_set_error("snail_instances_build: bad arguments");
		return 1;
	}
	for(size_t i = 0; i < (size_t)n * 12; i++)
		if(!std::isfinite(xf12[i])) { snail_set_error("snail_instances_build: instance %d has a non-finite transform", (int)(i / 12)); return 1; }
	for(size_t b = 0; b < (size_t)nBlas * 6; b++)
		if(!std::isfinite(blasBBox6[b])) { snail_set_error("snail_instances_build: BLAS %d has a non-finite box", (int)(b / 6)); return 1; }
	Builder B;
	B.box.resize(n);
	B.src.resize(n);
	for(int i = 0; i < n; i++) {
		if(blasIdx[i] < 0 || blasIdx[i] >= nBlas) { snail_set_error("snail_instances_build: instance %d names BLAS %d of %d", i, blasIdx[i], nBlas); return 1; }
		B.box[i] = instanceBox(xf12 + (size_t)i * 12, blasBBox6 + (size_t)blasIdx[i] * 6);
		B.src[i] = i;
	}
	// DBVH::Construct (:158-172): the root box is elements[0]'s, grown by the others in order
	std::vector<Node32> tmp((size_t)2 * n);
	B.nodes = tmp.data();
	Box root = B.box[0];
	for(int i = 1; i < n; i++) root.add(B.box[i]);
	B.push(root);
	B.run(n);
	if(B.depth > SNAIL_INSTANCES_MAX_DEPTH) {
		snail_set_error("snail_instances_build: the tree is %d levels deep, more than DBVH::maxDepth = %d", B.depth, SNAIL_INSTANCES_MAX_DEPTH);
		return 2;
	}
	memcpy(nodes32, tmp.data(), (size_t)B.nNodes * sizeof(Node32));
	*nNodes = B.nNodes;
	*depth = B.depth;
	if(perm) memcpy(perm, B.src.data(), (size_t)n * sizeof(int32_t));
	return 0;
}
