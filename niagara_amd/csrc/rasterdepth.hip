// rasterdepth.hip — depth-only rasteriser of the visible clusters for gfx950.
//
// Fills the [raster] box of niagara's frame (src/niagara.cpp:1765-1788) on a part without a graphics pipeline: for every slot of the
// grid clustersubmit wrote, the meshlet's vertices go to screen space with nv_trianglecull's arithmetic, snap to 8 sub-pixel bits, and
// every triangle that survives the rejection and facing rules is walked over the pixel centres it covers (top-left fill rule, exact
// int64 edge functions).  The depth is interpolated in fp32 in a fixed order and written with an integer max on its bits (reverse-Z,
// GREATER): the result does not depend on the order in which waves run.  The rule set is restated one sample at a time by
// tests/raster_ref.c; both raster paths below must equal it bit for bit.
//
// Shape.  A persistent grid; a wave owns a contiguous run of slots and fetches their headers lane-parallel (lane = slot, as
// trianglecull_kernel does), then takes the slots one after the other: lane = vertex for the vertex stage (snapped X, Y, z and a
// reject bit into LDS), lane = triangle for the setup (two passes for 96 triangles).  A triangle whose clipped bounding box holds at
// most `smallLimit` pixel centres is walked by its own lane right there; a larger one is queued in LDS and walked afterwards by the
// whole wave, lane = pixel of an 8 x 8 stamp.  Before each atomic the lane loads the current value and skips the atomic when it would
// not raise it (values only grow during a launch: a stale load costs an extra atomic, never a wrong result).
//
// CLIP (NV_OPT_RASTER_NEAR_CLIP 1) is a second instantiation: the vertex stage also keeps each vertex's clip x, y, w and d = w - z in LDS, a
// triangle that crosses the near plane becomes one or two pieces (raster.h: rd_clip), and each piece takes the road a triangle takes.  The
// queue entry of a large piece carries the piece number; the wave runs rd_clip again on the same inputs (same bits).  CLIP = false is
// the kernel without any of it.
//
// STABLE (NV_OPT_RASTER_VISIBILITY_ID 1) changes the visibility word only: bits(z) << 34 | ((mvi << 7 | triangle) + 1) with mvi the cluster's
// meshlet-visibility index, fetched with the slot's header, instead of bits(z) << 32 | slot << 7 | triangle.  STABLE = false is the kernel
// without it, instruction for instruction.
//
// The kernel's text and its launch are rasterdepth.h's (shared with rasterdepth_alpha.hip, which instantiates them with ALPHA: DESIGN.md §4.20); this
// file instantiates the four kernels of nv_rasterdepth and holds the totals launch every raster entry point uses.
#include "rasterdepth.h"

namespace nv
{

// adds the K per-workgroup partial sums of a launch to the caller's K totals (one workgroup)
template <int K>
__global__ __launch_bounds__(256) void rasterdepth_totals_kernel(const unsigned long long* __restrict__ partials, uint32_t blocks,
                                                                 unsigned long long* __restrict__ totals)
{
	__shared__ unsigned long long s_part[4][K];
	unsigned long long t[K] = {};
	for (uint32_t i = threadIdx.x; i < blocks; i += 256)
#pragma unroll
		for (int k = 0; k < K; ++k)
			t[k] += partials[(size_t)i * K + k];
#pragma unroll
	for (int k = 0; k < K; ++k)
		for (int o = 32; o > 0; o >>= 1)
			t[k] += __shfl_xor(t[k], o, 64);
	if ((threadIdx.x & 63u) == 0)
		for (int k = 0; k < K; ++k)
			s_part[threadIdx.x >> 6][k] = t[k];
	__syncthreads();
	if (threadIdx.x < K)
		totals[threadIdx.x] += s_part[0][threadIdx.x] + s_part[1][threadIdx.x] + s_part[2][threadIdx.x] + s_part[3][threadIdx.x];
}

// counters = 4 (the raster totals) or 2 (the alpha totals {dropped, unevaluated} of an ALPHA launch)
int launch_raster_totals(hipStream_t stream, const unsigned long long* partials, uint32_t blocks, unsigned long long* totals, uint32_t counters)
{
	if (counters == 4u)
		hipLaunchKernelGGL(rasterdepth_totals_kernel<4>, dim3(1), dim3(256), 0, stream, partials, blocks, totals);
	else
		hipLaunchKernelGGL(rasterdepth_totals_kernel<2>, dim3(1), dim3(256), 0, stream, partials, blocks, totals);
	return (int)hipGetLastError();
}

int launch_rasterdepth(hipStream_t stream, const RasterArgs& a, uint32_t gridBlocks, bool nearClip, bool stableIds)
{
	return launch_rasterdepth_as<false>(stream, a, gridBlocks, nearClip, stableIds);
}

} // namespace nv
