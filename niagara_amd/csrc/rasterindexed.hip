// rasterindexed.hip — depth-only rasteriser of niagara's indexed draws for gfx950.
//
// The classic render path (src/niagara.cpp:1680-1694: vkCmdDrawIndexedIndirectCount(dcb, dccb, maxDrawCount) through mesh.vert.glsl) on a
// part without a graphics pipeline.  Command i < min(dccb[0], drawCount) draws unless instanceCount == 0 or drawId >= drawCount; its
// triangle t < indexCount / 3 has the corners ib[firstIndex + 3t + k] + vertexOffset (mod 2^32) under the transform draws[drawId].  A
// triangle with an index position at or past indexCapacity, or a corner at or past vertexCapacity, is skipped: every load stays in range.
// Everything else is raster.h's, unchanged, so the same triangle under the same draw writes the bits nv_rasterdepth writes through the
// cluster path.  tests/raster_indexed_ref.c restates it on the CPU.
//
// Shape: balanced over triangles, not commands (one command can be a whole 29 k-triangle mesh).  Three launches, no inter-workgroup wait:
//   1. ri_count_kernel: per command its chunks of RI_CHUNK triangles; an inclusive scan of them over each workgroup's contiguous range of
//      commands (chunkEnds) and per workgroup its chunk sum, commands drawn and triangles (the fixed part of the scratch);
//   2. ri_scan_kernel (one workgroup): the exclusive prefix of the workgroup sums, so that the end of command i's chunks in the launch is
//      blockChunks[i / perBlock] + chunkEnds[i], and totals 0-1;
//   3. rasterindexed_kernel: a persistent grid; a wave owns a contiguous run of chunks, finds the command of its first chunk with a
//      64-wide search over those ends, and walks chunk after chunk with lane = triangle: 3 index loads, 3 corner transforms (no vertex
//      cache), setup; a small triangle is walked by its own lane, a large one queued in LDS (its three snapped corners) and walked by
//      the wave in 8 x 8 stamps, as in rasterdepth.hip.
// CLIP (NV_OPT_RASTER_NEAR_CLIP 1) is a second instantiation of the raster kernel: the corners' clip coordinates stay in registers, a triangle
// that crosses the near plane becomes one or two pieces (raster.h: rd_clip), and the chunk's first pieces, then its second pieces, take the
// road the triangles take (the queue is drained after each, so it stays at 64 entries).  CLIP = false is the kernel without any of it.
// Chunk positions are 32-bit and saturate: one launch draws at most 2^32 - 1 chunks (2.7e11 triangles); triangles past that are not drawn.
#include "rasterindexed.h"

namespace nv
{

// library scratch of nv_rasterdepth_indexed over up to drawCount commands: {commands, triangles} and the chunk sum per count workgroup
// (fixed, 20 KiB), then one word per command
size_t rasterindexed_scratch_bytes(uint32_t drawCount)
{
	return (size_t)RI_SCAN_BLOCKS * 2 * sizeof(unsigned long long) + (size_t)(RI_SCAN_BLOCKS + 2) * sizeof(uint32_t) + (size_t)drawCount * sizeof(uint32_t);
}

// inclusive 64-bit scan over the workgroup; `total` receives the workgroup's sum.  Every thread calls it (two barriers).
NV_DEV unsigned long long ri_block_scan(unsigned long long v, unsigned long long* s_wave, unsigned long long& total)
{
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	for (int o = 1; o < 64; o <<= 1)
	{
		const unsigned long long u = __shfl_up(v, o, 64);
		if (lane >= (uint32_t)o)
			v += u;
	}
	if (lane == 63)
		s_wave[wave] = v;
	__syncthreads();
	unsigned long long before = 0, sum = 0;
	for (uint32_t k = 0; k < (uint32_t)RI_WAVES; ++k)
	{
		const unsigned long long w = s_wave[k];
		before += k < wave ? w : 0ull;
		sum += w;
	}
	__syncthreads(); // s_wave is rewritten by the next call
	total = sum;
	return before + v;
}

// the workgroup's sums of two per-thread values, in thread 0
NV_DEV void ri_block_sum2(unsigned long long& a, unsigned long long& b, unsigned long long (*s_tot)[2])
{
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	for (int o = 32; o > 0; o >>= 1)
	{
		a += __shfl_xor(a, o, 64);
		b += __shfl_xor(b, o, 64);
	}
	if (lane == 0)
	{
		s_tot[wave][0] = a;
		s_tot[wave][1] = b;
	}
	__syncthreads();
	a = b = 0;
	if (threadIdx.x == 0)
		for (int k = 0; k < RI_WAVES; ++k)
		{
			a += s_tot[k][0];
			b += s_tot[k][1];
		}
}

__global__ __launch_bounds__(RI_THREADS) void ri_count_kernel(RasterIndexedArgs a)
{
	__shared__ unsigned long long s_wave[RI_WAVES];
	__shared__ unsigned long long s_tot[RI_WAVES][2];
	const uint32_t n = min(a.count[0], a.drawCount);
	const unsigned long long begin64 = (unsigned long long)blockIdx.x * a.perBlock;
	const uint32_t begin = (uint32_t)min(begin64, (unsigned long long)a.drawCount);
	const uint32_t end = (uint32_t)min(begin64 + a.perBlock, (unsigned long long)a.drawCount);
	unsigned long long carry = 0, cmds = 0, tris = 0;
	for (uint32_t base = begin; base < end; base += RI_THREADS) // (workgroup-uniform)
	{
		const uint32_t i = base + threadIdx.x;
		unsigned long long c = 0;
		if (i < end && i < n)
		{
			const NvMeshDrawCommand cmd = a.commands[i];
			if (cmd.instanceCount != 0 && cmd.drawId < a.drawCount) // instanceCount > 1 draws the same depth again
			{
				cmds += 1;
				tris += cmd.indexCount / 3u;
				c = (ri_triangles(cmd.indexCount, cmd.firstIndex, a.indexCapacity) + RI_CHUNK - 1) / RI_CHUNK;
			}
		}
		unsigned long long sum;
		const unsigned long long e = carry + ri_block_scan(c, s_wave, sum);
		if (i < end)
			a.chunkEnds[i] = ri_sat(e);
		carry += sum;
	}
	ri_block_sum2(cmds, tris, s_tot);
	if (threadIdx.x == 0)
	{
		a.blockChunks[blockIdx.x] = ri_sat(carry);
		a.blockTotals[blockIdx.x * 2] = cmds;
		a.blockTotals[blockIdx.x * 2 + 1] = tris;
	}
}

__global__ __launch_bounds__(RI_THREADS) void ri_scan_kernel(RasterIndexedArgs a)
{
	__shared__ unsigned long long s_wave[RI_WAVES];
	__shared__ unsigned long long s_tot[RI_WAVES][2];
	constexpr uint32_t PER = RI_SCAN_BLOCKS / RI_THREADS;
	unsigned long long v[PER], mine = 0, cmds = 0, tris = 0;
#pragma unroll
	for (uint32_t k = 0; k < PER; ++k)
	{
		const uint32_t j = threadIdx.x * PER + k;
		v[k] = j < a.scanBlocks ? a.blockChunks[j] : 0ull;
		mine += v[k];
		if (j < a.scanBlocks)
		{
			cmds += a.blockTotals[j * 2];
			tris += a.blockTotals[j * 2 + 1];
		}
	}
	unsigned long long total;
	unsigned long long before = ri_block_scan(mine, s_wave, total) - mine;
#pragma unroll
	for (uint32_t k = 0; k < PER; ++k)
	{
		const uint32_t j = threadIdx.x * PER + k;
		if (j < a.scanBlocks)
			a.blockChunks[j] = ri_sat(before);
		before += v[k];
	}
	ri_block_sum2(cmds, tris, s_tot);
	if (threadIdx.x == 0)
	{
		a.blockChunks[a.scanBlocks] = ri_sat(total);
		if (a.totals)
		{
			a.totals[0] += cmds;
			a.totals[1] += tris;
		}
	}
}

// the count and scan launches both entry points start with; the scratch pointers and the launch shape go into `a`
void launch_rasterindexed_prepare(hipStream_t stream, RasterIndexedArgs& a, void* scratch)
{
	a.blockTotals = static_cast<unsigned long long*>(scratch);
	a.blockChunks = reinterpret_cast<uint32_t*>(a.blockTotals + RI_SCAN_BLOCKS * 2);
	a.chunkEnds = a.blockChunks + RI_SCAN_BLOCKS + 2;
	const uint32_t wanted = (uint32_t)(((unsigned long long)a.drawCount + RI_THREADS - 1) / RI_THREADS);
	a.scanBlocks = wanted == 0 ? 1u : (wanted < RI_SCAN_BLOCKS ? wanted : RI_SCAN_BLOCKS);
	a.perBlock = (uint32_t)(((unsigned long long)a.drawCount + a.scanBlocks - 1) / a.scanBlocks);
	hipLaunchKernelGGL(ri_count_kernel, dim3(a.scanBlocks), dim3(RI_THREADS), 0, stream, a);
	hipLaunchKernelGGL(ri_scan_kernel, dim3(1), dim3(RI_THREADS), 0, stream, a);
}

int launch_rasterindexed(hipStream_t stream, RasterIndexedArgs a, void* scratch, uint32_t gridBlocks, bool nearClip)
{
	return launch_rasterindexed_as(stream, a, scratch, gridBlocks, nearClip);
}

} // namespace nv
