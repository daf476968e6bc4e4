// instances_materials_dynamic.inc -- the ShTriangle records of SEVERAL BLASes of an instanced material set packed in ONE launch
// (include/snail_instances_materials_dynamic.h).  An animated instanced scene re-packs a handful of small BLASes per frame; one k_shd_pack
// launch per BLAS would pay the launch latency once per BLAS.  Plain fp32 as materials_dynamic.inc (included before this file), whose
// per-record body (shdPackRecord) and info words (shdInfoWords) these kernels call: the bytes are k_shd_pack's.
//   k_ishd_pack   workgroup -> table entry by a prefix of per-entry workgroup counts (decided from blockIdx: wave-uniform), then record i of it
//   k_ishd_info   every entry's info words, after the pack (one workgroup of one wave per entry), and its zeroed-triangle counter back to 0
// The table goes BY VALUE in the kernel argument, kIshdMax entries per launch (a longer list takes several launches): no device table to
// fill, so no staging, no event and no allocation per call.
namespace devshd {

enum { kIshdMax = 16 };

struct IPackArgs {
	PackArgs e[kIshdMax];
	int first[kIshdMax + 1];   // first[k] = the workgroups of the entries before k; first[count] = the grid
	int count;
};

__global__ void __launch_bounds__(256) k_ishd_pack(IPackArgs T) {
	const int g = blockIdx.x;
	if(g >= T.first[T.count]) return;
	int k = 0;
	for(int q = 1; q < kIshdMax; q++)
		if(q < T.count && g >= T.first[q]) k = q;   // (first is non-decreasing: the last entry that starts at or before g)
	const PackArgs &A = T.e[k];
	const int i = (g - T.first[k]) * 256 + (int)threadIdx.x;
	if(i >= A.n) return;
	shdPackRecord(A, i);
}

__global__ void k_ishd_info(IPackArgs T) {
	const int k = blockIdx.x;   // (one wave per entry: the table is indexed by a wave-uniform value here too)
	if(k >= T.count || threadIdx.x != 0) return;
	shdInfoWords(T.e[k]);
	*T.e[k].zeroed = 0;   // for the entry's next pack, which is ordered behind this launch: a batched call enqueues no memset per BLAS
}

} // namespace devshd
