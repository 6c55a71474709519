// rasterdepth_alpha.hip — nv_rasterdepth_textured: the depth rasteriser of the visible clusters with the POST alpha discard as coverage
// (mesh.frag.glsl:88).
//
// The pass is rasterdepth.h's kernel — slot headers, vertex stage, set-up, clipping, both raster paths: shared with nv_rasterdepth, not copied —
// instantiated with ALPHA.  With the slot's header a lane also fetches the draw's materialIndex, the material's albedoTexture and
// diffuseFactor.a and the texture's descriptor, each load behind the check that keeps it inside its table; the slot's road is wave-uniform.  The
// vertex stage of an alpha-tested slot keeps one more float4 per vertex in LDS (clip x, y, w and the packed texcoord); a covered sample sets up
// the ORIGINAL triangle from them as the attribute pass does (fragalpha.h), samples the albedo texture through texmath.h's `textureSampler`
// (8 taps) and is dropped, before any load or atomic on the targets, when albedo.a < 0.5.  Alpha is evaluated for EVERY covered sample of an
// alpha-tested slot, so the kept and dropped counts do not depend on the order of the GPU's work.  smallLimit picks the path of every slot's
// triangles, alpha-tested or not: a lane that walks its own small triangle issues its own taps.
#include "rasterdepth.h"

namespace nv
{

// adds the per-workgroup {dropped, unevaluated} of a launch to the caller's two alpha totals (one workgroup)
__global__ __launch_bounds__(256) void rasterdepth_alpha_totals_kernel(const unsigned long long* __restrict__ partials, uint32_t blocks,
                                                                       unsigned long long* __restrict__ totals)
{
	__shared__ unsigned long long s_part[4][2];
	unsigned long long t0 = 0, t1 = 0;
	for (uint32_t i = threadIdx.x; i < blocks; i += 256)
	{
		t0 += partials[(size_t)i * 2];
		t1 += partials[(size_t)i * 2 + 1];
	}
	for (int o = 32; o > 0; o >>= 1)
	{
		t0 += __shfl_xor(t0, o, 64);
		t1 += __shfl_xor(t1, o, 64);
	}
	if ((threadIdx.x & 63u) == 0)
	{
		s_part[threadIdx.x >> 6][0] = t0;
		s_part[threadIdx.x >> 6][1] = t1;
	}
	__syncthreads();
	if (threadIdx.x < 2)
		totals[threadIdx.x] += s_part[0][threadIdx.x] + s_part[1][threadIdx.x] + s_part[2][threadIdx.x] + s_part[3][threadIdx.x];
}

// the launch of the kernel above, for nv_rasterdepth_blocks' launcher too
int launch_raster_alpha_totals(hipStream_t stream, const unsigned long long* partials, uint32_t blocks, unsigned long long* totals)
{
	hipLaunchKernelGGL(rasterdepth_alpha_totals_kernel, dim3(1), dim3(256), 0, stream, partials, blocks, totals);
	return (int)hipGetLastError();
}

int launch_rasterdepth_alpha(hipStream_t stream, const RasterAlphaArgs& a, uint32_t gridBlocks, bool nearClip, bool stableIds)
{
	gridBlocks = gridBlocks / 8 * RD_BLOCKS_PER_CU; // the caller passes 8 workgroups per CU, the size of `partials` and `alphaPartials`
	if (stableIds && a.visibility) // (as launch_rasterdepth)
	{
		if (nearClip)
			hipLaunchKernelGGL((rasterdepth_kernel<true, true, true, RasterAlphaArgs>), dim3(gridBlocks), dim3(RD_THREADS), 0, stream, a);
		else
			hipLaunchKernelGGL((rasterdepth_kernel<false, true, true, RasterAlphaArgs>), dim3(gridBlocks), dim3(RD_THREADS), 0, stream, a);
	}
	else if (nearClip)
		hipLaunchKernelGGL((rasterdepth_kernel<true, false, true, RasterAlphaArgs>), dim3(gridBlocks), dim3(RD_THREADS), 0, stream, a);
	else
		hipLaunchKernelGGL((rasterdepth_kernel<false, false, true, RasterAlphaArgs>), dim3(gridBlocks), dim3(RD_THREADS), 0, stream, a);
	hipError_t e = hipGetLastError();
	if (e == hipSuccess && a.totals)
		e = (hipError_t)launch_raster_totals(stream, a.partials, gridBlocks, a.totals);
	if (e == hipSuccess && a.alphaTotals)
		e = (hipError_t)launch_raster_alpha_totals(stream, a.alphaPartials, gridBlocks, a.alphaTotals);
	return (int)e;
}

} // namespace nv
