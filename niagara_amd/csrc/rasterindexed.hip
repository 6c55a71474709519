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
#include "raster.h"

namespace nv
{

constexpr int RI_WAVES = 4;
constexpr int RI_THREADS = RI_WAVES * 64;
constexpr uint32_t RI_CHUNK = 64;         // triangles per chunk (lane = triangle)
constexpr uint32_t RI_SCAN_BLOCKS = 1024; // workgroups of the count launch at most (the fixed part of the scratch)
static_assert(RI_SCAN_BLOCKS % RI_THREADS == 0, "the scan launch takes RI_SCAN_BLOCKS / RI_THREADS entries per thread");
#ifndef RI_BLOCKS_PER_CU
#define RI_BLOCKS_PER_CU 6 // <= 8: the partial totals are sized for 8 workgroups per CU (context.hip)
#endif

// library scratch of nv_rasterdepth_indexed over up to drawCount commands: {commands, triangles} and the chunk sum per count workgroup
// (fixed, 20 KiB), then one word per command
size_t rasterindexed_scratch_bytes(uint32_t drawCount)
{
	return (size_t)RI_SCAN_BLOCKS * 2 * sizeof(unsigned long long) + (size_t)(RI_SCAN_BLOCKS + 2) * sizeof(uint32_t) + (size_t)drawCount * sizeof(uint32_t);
}

NV_DEV uint32_t ri_sat(unsigned long long v) { return v < 0xffffffffull ? (uint32_t)v : 0xffffffffu; }

// triangles of a drawing command whose three index positions lie below the capacity: triangle t's last position firstIndex + 3t + 2 is below
// it iff t < (indexCapacity - firstIndex) / 3, so they are a prefix of the command's triangles
NV_DEV uint32_t ri_triangles(uint32_t indexCount, uint32_t firstIndex, uint32_t indexCapacity)
{
	const uint32_t room = indexCapacity > firstIndex ? (indexCapacity - firstIndex) / 3u : 0u;
	const uint32_t n = indexCount / 3u;
	return n < room ? n : room;
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

// the end (last chunk + 1) of command i's chunks in the launch, saturated
NV_DEV uint32_t ri_end(const RasterIndexedArgs& a, uint32_t i)
{
	return ri_sat((unsigned long long)a.blockChunks[i / a.perBlock] + a.chunkEnds[i]);
}

// The first command i in [lo, hi) with ri_end(i) > k; there is one (k < ri_end(hi - 1)).  All 64 lanes, wave-uniform arguments.  The next 64
// commands are tried first (a wave walking forward finds its next command there), then 64 evenly spaced probes narrow the range.
NV_DEV uint32_t ri_find(const RasterIndexedArgs& a, uint32_t k, uint32_t lo, uint32_t hi, uint32_t lane)
{
	for (;;)
	{
		const uint32_t span = hi - lo;
		const uint64_t near = __ballot(lane < span && ri_end(a, lo + lane) > k);
		if (near)
			return lo + (uint32_t)__builtin_ctzll(near);
		lo += 64u; // (span > 64: the answer lies further on)
		const uint32_t rest = hi - lo;
		if (rest <= 64u)
			continue;
		const uint32_t p = lo + (uint32_t)(((uint64_t)(lane + 1u) * rest) >> 6) - 1u; // lane 63 probes hi - 1
		const uint32_t j = (uint32_t)__builtin_ctzll(__ballot(ri_end(a, p) > k));
		hi = lo + (uint32_t)(((uint64_t)(j + 1u) * rest) >> 6);
		lo = lo + (uint32_t)(((uint64_t)j * rest) >> 6);
	}
}

template <bool CLIP>
__global__ __launch_bounds__(RI_THREADS) void rasterindexed_kernel(RasterIndexedArgs a)
{
	__shared__ int4 s_queue[RI_WAVES][RI_CHUNK][3]; // large pieces of the current chunk (one piece number at a time): their snapped corners

	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t chunks = load_uniform_u32(a.blockChunks + a.scanBlocks); // written by the scan launch
	const uint32_t n = min(load_uniform_u32(a.count), a.drawCount);
	const uint32_t numWaves = gridDim.x * RI_WAVES;
	const uint32_t w = blockIdx.x * RI_WAVES + wave;
	const uint32_t per = chunks / numWaves + (chunks % numWaves ? 1u : 0u); // contiguous chunks per wave
	const unsigned long long begin64 = (unsigned long long)w * per;
	const uint32_t begin = (uint32_t)min(begin64, (unsigned long long)chunks);
	const uint32_t end = (uint32_t)min(begin64 + per, (unsigned long long)chunks);
	const int32_t W = (int32_t)a.width, H = (int32_t)a.height;
	const bool bothFaces = a.globals.cullData.postPass != 0;
	int4(*queue)[3] = s_queue[wave];

	uint32_t drawn = 0;             // per lane
	unsigned long long samples = 0; // per lane
	// the current command (wave-uniform): its chunk range, triangles in range, index base and vertex offset, transform
	uint32_t next = 0, cmdBegin = 0, cmdEnd = 0, tris = 0, firstIndex = 0, vertexOffset = 0;
	f3 q = { 0.0f, 0.0f, 0.0f };
	float qw = 1.0f, scale = 0.0f, px = 0.0f, py = 0.0f, pz = 0.0f;

	for (uint32_t k = begin; k < end; ++k)
	{
		if (k >= cmdEnd)
		{
			const uint32_t i = ri_find(a, k, next, n, lane);
			next = i + 1u;
			cmdBegin = __builtin_amdgcn_readfirstlane(i ? ri_end(a, i - 1u) : 0u);
			cmdEnd = __builtin_amdgcn_readfirstlane(ri_end(a, i));
			const NvMeshDrawCommand c = a.commands[i]; // a command with chunks draws: drawId < drawCount
			tris = __builtin_amdgcn_readfirstlane(ri_triangles(c.indexCount, c.firstIndex, a.indexCapacity));
			firstIndex = __builtin_amdgcn_readfirstlane(c.firstIndex);
			vertexOffset = __builtin_amdgcn_readfirstlane(c.vertexOffset);
			const float4* dp = reinterpret_cast<const float4*>(a.draws + __builtin_amdgcn_readfirstlane(c.drawId));
			const float4 d0 = dp[0], d1 = dp[1];
			q = { d1.x, d1.y, d1.z };
			qw = d1.w, scale = d0.w, px = d0.x, py = d0.y, pz = d0.z;
		}

		// ---- lane = triangle: indices, corners (mesh.vert.glsl:41-57, per corner), setup; small ones walked here, large ones queued
		const uint32_t t = (k - cmdBegin) * RI_CHUNK + lane; // (a command has < 2^26 chunks)
		// The two branches repeat each other's text on purpose: written as one loop over pieces, the CLIP = false instantiation compiles to other
		// code than the kernel had before the option (other registers, other schedule); kept apart, it is that kernel instruction for instruction.
		if constexpr (!CLIP)
		{
			RdTri tri;
			bool live = false, large = false;
			int4 ca = make_int4(0, 0, 0, 1), cb = ca, cc = ca;
			if (t < tris)
			{
				const unsigned long long at = (unsigned long long)firstIndex + 3ull * t; // at + 2 < indexCapacity (ri_triangles)
				const uint32_t va = a.indices[at] + vertexOffset, vb = a.indices[at + 1] + vertexOffset, vc = a.indices[at + 2] + vertexOffset;
				if (va < a.vertexCapacity && vb < a.vertexCapacity && vc < a.vertexCapacity) // (0xFFFFFFFF included: no primitive restart)
				{
					ca = rd_vertex(a.globals, *reinterpret_cast<const uint2*>(a.vertices + va), q, qw, scale, px, py, pz, H);
					cb = rd_vertex(a.globals, *reinterpret_cast<const uint2*>(a.vertices + vb), q, qw, scale, px, py, pz, H);
					cc = rd_vertex(a.globals, *reinterpret_cast<const uint2*>(a.vertices + vc), q, qw, scale, px, py, pz, H);
					live = rd_setup_corners(ca, cb, cc, bothFaces, W, H, tri);
				}
			}
			if (live)
			{
				drawn += 1;
				if (tri.x0 <= tri.x1 && tri.y0 <= tri.y1)
				{
					const uint32_t boxPixels = (uint32_t)(tri.x1 - tri.x0 + 1) * (uint32_t)(tri.y1 - tri.y0 + 1);
					large = boxPixels > a.smallLimit;
					if (!large)
						for (int32_t y = tri.y0; y <= tri.y1; ++y)
							for (int32_t x = tri.x0; x <= tri.x1; ++x)
								samples += rd_sample(tri, x, y, a.width, a.depth, nullptr, 0u) ? 1u : 0u;
				}
			}
			const uint64_t qb = __ballot(large);
			rd_lds_order(); // the previous chunk's queue readers are done
			if (large)
			{
				const uint32_t slot = (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(qb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)qb, 0u));
				queue[slot][0] = ca;
				queue[slot][1] = cb;
				queue[slot][2] = cc;
			}
			rd_lds_order();

			// ---- large triangles, the whole wave: lane = pixel of an 8 x 8 stamp
			const uint32_t queued = (uint32_t)__builtin_popcountll(qb);
			for (uint32_t e = 0; e < queued; ++e)
			{
				RdTri tq;
				rd_setup_corners(queue[e][0], queue[e][1], queue[e][2], bothFaces, W, H, tq); // (true: it was queued; same inputs, same bits)
				const uint32_t sw = (uint32_t)(tq.x1 - tq.x0) / 8u + 1u, sh = (uint32_t)(tq.y1 - tq.y0) / 8u + 1u;
				const int32_t lx = (int32_t)(lane & 7u), ly = (int32_t)(lane >> 3);
				for (uint32_t sy = 0; sy < sh; ++sy)
				{
					const int32_t y = tq.y0 + (int32_t)sy * 8 + ly;
					for (uint32_t sx = 0; sx < sw; ++sx)
					{
						const int32_t x = tq.x0 + (int32_t)sx * 8 + lx;
						if (x <= tq.x1 && y <= tq.y1)
							samples += rd_sample(tq, x, y, a.width, a.depth, nullptr, 0u) ? 1u : 0u;
					}
				}
			}
		}
		else
		{
			uint32_t pieces = 0;
			int4 p0 = make_int4(0, 0, 0, 1), p1 = p0, p2 = p0, p3 = p0;
			if (t < tris)
			{
				const unsigned long long at = (unsigned long long)firstIndex + 3ull * t; // at + 2 < indexCapacity (ri_triangles)
				const uint32_t va = a.indices[at] + vertexOffset, vb = a.indices[at + 1] + vertexOffset, vc = a.indices[at + 2] + vertexOffset;
				if (va < a.vertexCapacity && vb < a.vertexCapacity && vc < a.vertexCapacity) // (0xFFFFFFFF included: no primitive restart)
				{
					const uint2 ra = *reinterpret_cast<const uint2*>(a.vertices + va), rb = *reinterpret_cast<const uint2*>(a.vertices + vb);
					const uint2 rc = *reinterpret_cast<const uint2*>(a.vertices + vc);
					float4 ka, kb, kc;
					const int4 ca = rd_vertex_clip(a.globals, ra, q, qw, scale, px, py, pz, H, ka);
					const int4 cb = rd_vertex_clip(a.globals, rb, q, qw, scale, px, py, pz, H, kb);
					const int4 cc = rd_vertex_clip(a.globals, rc, q, qw, scale, px, py, pz, H, kc);
					pieces = rd_clip(a.globals, ca, cb, cc, ka, kb, kc, H, p0, p1, p2, p3);
				}
			}
			for (uint32_t p = 0; p < 2u; ++p)
			{
				if (!__ballot(p < pieces)) // (wave-uniform)
					break;
				RdTri tri;
				bool large = false;
				const int4 cb = rd_sel(p != 0u, p2, p1), cc = rd_sel(p != 0u, p3, p2);
				const bool live = p < pieces && rd_setup_corners(p0, cb, cc, bothFaces, W, H, tri);
				if (live)
				{
					drawn += 1;
					if (tri.x0 <= tri.x1 && tri.y0 <= tri.y1)
					{
						const uint32_t boxPixels = (uint32_t)(tri.x1 - tri.x0 + 1) * (uint32_t)(tri.y1 - tri.y0 + 1);
						large = boxPixels > a.smallLimit;
						if (!large)
							for (int32_t y = tri.y0; y <= tri.y1; ++y)
								for (int32_t x = tri.x0; x <= tri.x1; ++x)
									samples += rd_sample(tri, x, y, a.width, a.depth, nullptr, 0u) ? 1u : 0u;
					}
				}
				const uint64_t qb = __ballot(large);
				rd_lds_order(); // the previous queue's readers are done
				if (large)
				{
					const uint32_t slot = (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(qb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)qb, 0u));
					queue[slot][0] = p0;
					queue[slot][1] = cb;
					queue[slot][2] = cc;
				}
				rd_lds_order();

				// ---- large pieces, the whole wave: lane = pixel of an 8 x 8 stamp
				const uint32_t queued = (uint32_t)__builtin_popcountll(qb);
				for (uint32_t e = 0; e < queued; ++e)
				{
					RdTri tq;
					rd_setup_corners(queue[e][0], queue[e][1], queue[e][2], bothFaces, W, H, tq); // (true: it was queued; same inputs, same bits)
					const uint32_t sw = (uint32_t)(tq.x1 - tq.x0) / 8u + 1u, sh = (uint32_t)(tq.y1 - tq.y0) / 8u + 1u;
					const int32_t lx = (int32_t)(lane & 7u), ly = (int32_t)(lane >> 3);
					for (uint32_t sy = 0; sy < sh; ++sy)
					{
						const int32_t y = tq.y0 + (int32_t)sy * 8 + ly;
						for (uint32_t sx = 0; sx < sw; ++sx)
						{
							const int32_t x = tq.x0 + (int32_t)sx * 8 + lx;
							if (x <= tq.x1 && y <= tq.y1)
								samples += rd_sample(tq, x, y, a.width, a.depth, nullptr, 0u) ? 1u : 0u;
						}
					}
				}
			}
		}
	}

	// totals 2-3: per-workgroup partial sums, plain stores (0 in slots 0-1: the scan launch added those); launch_raster_totals adds them up
	__shared__ unsigned long long s_tot[RI_WAVES][2];
	unsigned long long d = drawn, smp = samples;
	for (int o = 32; o > 0; o >>= 1)
	{
		d += __shfl_xor(d, o, 64);
		smp += __shfl_xor(smp, o, 64);
	}
	if (lane == 0)
	{
		s_tot[wave][0] = d;
		s_tot[wave][1] = smp;
	}
	__syncthreads();
	if (threadIdx.x < 4)
	{
		unsigned long long t = 0;
		if (threadIdx.x >= 2)
#pragma unroll
			for (int k = 0; k < RI_WAVES; ++k)
				t += s_tot[k][threadIdx.x - 2];
		a.partials[(size_t)blockIdx.x * 4 + threadIdx.x] = t;
	}
}

int launch_rasterindexed(hipStream_t stream, RasterIndexedArgs a, void* scratch, uint32_t gridBlocks, bool nearClip)
{
	a.blockTotals = static_cast<unsigned long long*>(scratch);
	a.blockChunks = reinterpret_cast<uint32_t*>(a.blockTotals + RI_SCAN_BLOCKS * 2);
	a.chunkEnds = a.blockChunks + RI_SCAN_BLOCKS + 2;
	const uint32_t wanted = (uint32_t)(((unsigned long long)a.drawCount + RI_THREADS - 1) / RI_THREADS);
	a.scanBlocks = wanted == 0 ? 1u : (wanted < RI_SCAN_BLOCKS ? wanted : RI_SCAN_BLOCKS);
	a.perBlock = (uint32_t)(((unsigned long long)a.drawCount + a.scanBlocks - 1) / a.scanBlocks);
	hipLaunchKernelGGL(ri_count_kernel, dim3(a.scanBlocks), dim3(RI_THREADS), 0, stream, a);
	hipLaunchKernelGGL(ri_scan_kernel, dim3(1), dim3(RI_THREADS), 0, stream, a);
	gridBlocks = gridBlocks / 8 * RI_BLOCKS_PER_CU; // the caller passes 8 workgroups per CU, the size of `partials`
	if (nearClip)
		hipLaunchKernelGGL(rasterindexed_kernel<true>, dim3(gridBlocks), dim3(RI_THREADS), 0, stream, a);
	else
		hipLaunchKernelGGL(rasterindexed_kernel<false>, dim3(gridBlocks), dim3(RI_THREADS), 0, stream, a);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess || !a.totals)
		return (int)e;
	return launch_raster_totals(stream, a.partials, gridBlocks, a.totals, 4);
}

} // namespace nv
