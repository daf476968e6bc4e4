// heatmap.inc -- the reference's "scene complexity visualization" (gVals[5], src/scene_trace.cpp:513-517) on the device: the store stage that turns
// per-packet TreeStats into colours (included by snail_hip.hip once, after the two arithmetics' kernels; the C-ABI of include/snail_heatmap.h is
// heatmap_host.inc).
//
// The counters themselves are booked by the walking stages of the staged pipeline (dev::bookPacket in k_primary, k_light, k_rays and their deferred
// passes, and the mirrored packets' ray counts in k_final<.., DST_MIRROR>): renderWhitted with a HeatOut runs every walk of the lit frame -- the
// counters ARE the result -- and replaces the colour stores (k_final<.., DST_FRAME / DST_COLOR>, the fused tail of k_light) by dev_heat::k_heat_store.
// Plain fp32, one conversion and one separately rounded multiply per channel: the same bits in both arithmetics, so the kernels exist once.
namespace dev_heat {

// Vec3q(float(intersects) * (0.002f / size), float(iterations) * (0.02f / size), float(skips * 0.25f)), size = 64 quads: (r, g, b)
__device__ __forceinline__ void heatColour(const unsigned *__restrict__ w, float (&c)[3]) {
	c[0] = (float)w[0] * (0.002f / 64.0f);
	c[1] = (float)w[1] * (0.02f / 64.0f);
	c[2] = (float)w[3] * 0.25f;   // unsigned * float converts the counter first (usual arithmetic conversions)
}

// The four double-resolution packets of every packet of a list (4x antialiasing, src/render.cpp:71-110): sub-packet k of packet p at
// (2x + 16 (k & 1), 2y + 16 (k >> 1)), stored at 4 p + k.  xy null: the frame's own grid, packet p = cy * pw + cx at (16 cx, 16 cy).
__global__ __launch_bounds__(256) void k_heat_aa_packets(const int2 *__restrict__ xy, int pw, int nPackets, int2 *__restrict__ xy2) {
	const int i = (int)(blockIdx.x * 256 + threadIdx.x);
	if(i >= nPackets * 4) return;
	const int p = i >> 2, k = i & 3;
	const int2 a = xy ? xy[p] : make_int2((p % pw) * 16, (p / pw) * 16);
	xy2[i] = make_int2(a.x * 2 + ((k & 1) ? 16 : 0), a.y * 2 + ((k & 2) ? 16 : 0));
}

// One wave per packet, lane = quad (row lane >> 2, pixels 4 (lane & 3) .. + 3): every ray of the packet gets the packet's colour, hits and misses
// alike, then ConvColor -> packet-major B,G,R [nPackets][256][3].  AA: pstats holds the FOUR sub-packets' counters [nPackets][4][4]; the 8x8
// quadrant (k & 1, k >> 1) of the packet is the 2x2 reduction of sub-packet k's (uniform) colour c_k, in the reference's operation order
// ((c_k + c_k) * 0.25) + ((c_k + c_k) * 0.25) -- what dev::k_aa_reduce computes from float colours, without the 3 KB per sub-packet in between.
template <bool AA>
__global__ __launch_bounds__(64) void k_heat_store(const unsigned *__restrict__ pstats, int nPackets, unsigned char *__restrict__ bgrPackets) {
	const int p = (int)blockIdx.x, lane = (int)threadIdx.x;
	if(p >= nPackets) return;
	float c[3];
	if(AA) {
		const int row = lane >> 2, qc = lane & 3;
		const int k = (row >= 8 ? 2 : 0) + (qc >= 2 ? 1 : 0);
		float s[3];
		heatColour(pstats + ((size_t)p * 4 + k) * 4, s);
#pragma unroll
		for(int ch = 0; ch < 3; ch++) c[ch] = (s[ch] + s[ch]) * 0.25f + (s[ch] + s[ch]) * 0.25f;
	} else heatColour(pstats + (size_t)p * 4, c);
	const unsigned b = (unsigned)dev::convChannelW(c[2]), g = (unsigned)dev::convChannelW(c[1]), r = (unsigned)dev::convChannelW(c[0]);
	// four pixels B,G,R B,G,R B,G,R B,G,R = three dwords
	unsigned *o = (unsigned *)(bgrPackets + ((size_t)p * 256 + (size_t)lane * 4) * 3);
	o[0] = b | (g << 8) | (r << 16) | (b << 24);
	o[1] = g | (r << 8) | (b << 16) | (g << 24);
	o[2] = r | (b << 8) | (g << 16) | (r << 24);
}

// The instanced scenes' tile renderer goes on from FLOAT colours (dev::k_inst_store: 2x2 reduction, rank tint, ConvColor, bytes or planes): every ray
// of packet p gets the packet's colour, [nPackets][256][3] (r, g, b).  One wave per packet, lane = quad: twelve floats = three float4.
__global__ __launch_bounds__(64) void k_heat_colours(const unsigned *__restrict__ pstats, int nPackets, float *__restrict__ col) {
	const int p = (int)blockIdx.x, lane = (int)threadIdx.x;
	if(p >= nPackets) return;
	float c[3];
	heatColour(pstats + (size_t)p * 4, c);
	float4 *o = (float4 *)(col + ((size_t)p * 256 + (size_t)lane * 4) * 3);
	o[0] = make_float4(c[0], c[1], c[2], c[0]);
	o[1] = make_float4(c[1], c[2], c[0], c[1]);
	o[2] = make_float4(c[2], c[0], c[1], c[2]);
}

} // namespace dev_heat
