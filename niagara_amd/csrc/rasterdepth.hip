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
#include "raster.h"

namespace nv
{

constexpr int RD_WAVES = 4;
constexpr int RD_THREADS = RD_WAVES * 64;
constexpr uint32_t RD_CHUNK = 64; // slots whose headers a wave fetches together (lane = slot)
#ifndef RD_BLOCKS_PER_CU
#define RD_BLOCKS_PER_CU 6 // <= 8: the partial totals are sized for 8 workgroups per CU (context.hip)
#endif

// the id of triangle t in the visibility word: slot << 7 | t, or the stable form's id34 (raster.h)
template <bool STABLE>
NV_DEV auto rd_id(uint32_t index, uint32_t mvi, uint32_t t)
{
	if constexpr (STABLE)
		return ((unsigned long long)mvi << 7 | t) + 1ull;
	else
		return index << 7 | t;
}

template <bool CLIP, bool STABLE>
__global__ __launch_bounds__(RD_THREADS) void rasterdepth_kernel(RasterArgs a)
{
	constexpr uint32_t PIECES = CLIP ? 2u : 1u; // pieces of a triangle at most
	__shared__ int4 s_vtx[RD_WAVES][64];       // per vertex of the current slot: X, Y, z bits, reject (CLIP: | RD_OUTSIDE)
	__shared__ float4 s_clip[RD_WAVES][64];    // CLIP only: clip x, y, w and d = w - z (NaN: a non-finite component)
	__shared__ uint32_t s_queue[RD_WAVES][96 * PIECES]; // large pieces of the current slot: t | piece << 7 | ia << 8 | ib << 16 | ic << 24

	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t gx = a.cc4[1], gz = a.cc4[3];
	const uint32_t slots = gx * a.cc4[2] * gz;
	const uint32_t numWaves = gridDim.x * RD_WAVES;
	const uint32_t w = blockIdx.x * RD_WAVES + wave;
	const uint32_t per = (slots + numWaves - 1) / numWaves; // contiguous slots per wave
	const uint32_t begin = w * per < slots ? w * per : slots;
	const uint32_t end = begin + per < slots ? begin + per : slots;
	const int32_t W = (int32_t)a.width, H = (int32_t)a.height;
	const bool bothFaces = a.globals.cullData.postPass != 0;
	const uint8_t* data8 = reinterpret_cast<const uint8_t*>(a.meshletData);
	const uint16_t* data16 = reinterpret_cast<const uint16_t*>(a.meshletData);
	int4* vtx = s_vtx[wave];
	uint32_t* queue = s_queue[wave];
	float4* cvx = nullptr;
	if constexpr (CLIP)
		cvx = s_clip[wave];

	uint32_t clusters = 0, triangles = 0; // wave-uniform
	uint32_t drawn = 0;                   // per lane
	unsigned long long samples = 0;       // per lane

	for (uint32_t chunk = begin; chunk < end; chunk += RD_CHUNK)
	{
		const uint32_t cnt = end - chunk < RD_CHUNK ? end - chunk : RD_CHUNK;
		// lane = slot: grid position -> index (the mesh shader's x + 256 y + CLUSTER_TILE z) -> cluster index -> command -> headers
		uint32_t hIndex = 0, hCi = ~0u, hDataOffset = 0, hBaseVertex = 0, hCounts = 0;
		uint32_t hMvi = 0; // STABLE only: the cluster's meshlet-visibility index, command.meshletVisibilityOffset + lane (the bit nv_clustercull keeps for it)
		float4 hD0 = make_float4(0, 0, 0, 0), hD1 = make_float4(0, 0, 0, 1);
		if (lane < cnt)
		{
			const uint32_t k = chunk + lane, x = k % gx, r = k / gx;
			hIndex = x + (r / gz) * 256u + (r % gz) * NV_CLUSTER_TILE;
			hCi = a.clusterIndices[hIndex];
		}
		if (hCi != ~0u)
		{
			const uint32_t* cmd = reinterpret_cast<const uint32_t*>(a.commands + (hCi & 0xffffffu));
			const uint32_t drawId = cmd[0], taskOffset = cmd[1];
			const uint32_t* mw = reinterpret_cast<const uint32_t*>(a.meshlets + taskOffset + (hCi >> 24));
			hDataOffset = mw[3];
			hBaseVertex = mw[4];
			hCounts = mw[5] & 0xffffffu; // vertexCount | triangleCount << 8 | shortRefs << 16
			if constexpr (STABLE)
				hMvi = cmd[4] + (hCi >> 24);
			const float4* dp = reinterpret_cast<const float4*>(a.draws + drawId);
			hD0 = dp[0];
			hD1 = dp[1];
		}

		for (uint32_t s = 0; s < cnt; ++s)
		{
			const uint32_t ci = rd_rl(hCi, s);
			if (ci == ~0u)
				continue;
			const uint32_t index = rd_rl(hIndex, s);
			const uint32_t dataOffset = rd_rl(hDataOffset, s), baseVertex = rd_rl(hBaseVertex, s), counts = rd_rl(hCounts, s);
			const uint32_t vcRaw = counts & 0xffu, tcRaw = counts >> 8 & 0xffu, shortRefs = (counts >> 16 & 0xffu) == 1u;
			const uint32_t ve = vcRaw < 64u ? vcRaw : 64u, te = tcRaw < 96u ? tcRaw : 96u;
			const uint32_t indexOffset = dataOffset + (shortRefs ? (vcRaw + 1) / 2 : vcRaw);
			clusters += 1;
			triangles += tcRaw;
			// STABLE: a cluster whose index does not fit the word's 27 bits writes depth and no visibility word
			uint32_t mvi = 0;
			unsigned long long* vis = a.visibility;
			if constexpr (STABLE)
			{
				mvi = rd_rl(hMvi, s);
				vis = mvi < RD_STABLE_MVI_END ? vis : nullptr;
			}

			rd_lds_order(); // the previous slot's readers are done
			// ---- vertex stage, lane = vertex (nv_trianglecull's arithmetic, src/shaders/meshlet.mesh.glsl:121-160)
			const f3 q = { __uint_as_float(rd_rl(__float_as_uint(hD1.x), s)), __uint_as_float(rd_rl(__float_as_uint(hD1.y), s)),
			               __uint_as_float(rd_rl(__float_as_uint(hD1.z), s)) };
			const float qw = __uint_as_float(rd_rl(__float_as_uint(hD1.w), s)), scale = __uint_as_float(rd_rl(__float_as_uint(hD0.w), s));
			const float px = __uint_as_float(rd_rl(__float_as_uint(hD0.x), s)), py = __uint_as_float(rd_rl(__float_as_uint(hD0.y), s));
			const float pz = __uint_as_float(rd_rl(__float_as_uint(hD0.z), s));
			if (lane < ve)
			{
				const uint32_t ref = shortRefs ? (uint32_t)data16[dataOffset * 2 + lane] : a.meshletData[dataOffset + lane];
				const uint2 pv = *reinterpret_cast<const uint2*>(a.vertices + ref + baseVertex);
				if constexpr (CLIP)
				{
					float4 cv;
					vtx[lane] = rd_vertex_clip(a.globals, pv, q, qw, scale, px, py, pz, H, cv);
					cvx[lane] = cv;
				}
				else
					vtx[lane] = rd_vertex(a.globals, pv, q, qw, scale, px, py, pz, H);
			}
			rd_lds_order();

			// ---- triangle setup, lane = triangle; small ones are walked here by their own lane, large ones queued
			uint32_t queued = 0; // wave-uniform
			for (uint32_t tb = 0; tb < te; tb += 64)
			{
				// The two branches repeat each other's text on purpose: written as one loop over pieces, the CLIP = false instantiation compiles to other
				// code than the kernel had before the option (other registers, other schedule); kept apart, it is that kernel instruction for instruction.
				if constexpr (!CLIP)
				{
					const uint32_t t = tb + lane;
					RdTri tri;
					bool live = false, large = false;
					uint32_t ia = 0, ib = 0, ic = 0;
					if (t < te)
					{
						const uint32_t o = indexOffset * 4 + t * 3;
						ia = data8[o], ib = data8[o + 1], ic = data8[o + 2];
						live = rd_setup(vtx, ia, ib, ic, ve, bothFaces, W, H, tri);
					}
					if (live)
					{
						drawn += 1;
						if (tri.x0 <= tri.x1 && tri.y0 <= tri.y1)
						{
							const uint32_t n = (uint32_t)(tri.x1 - tri.x0 + 1) * (uint32_t)(tri.y1 - tri.y0 + 1);
							large = n > a.smallLimit;
							if (!large)
							{
								const auto id = rd_id<STABLE>(index, mvi, t);
								for (int32_t py = tri.y0; py <= tri.y1; ++py)
									for (int32_t px = tri.x0; px <= tri.x1; ++px)
										samples += rd_sample<STABLE>(tri, px, py, a.width, a.depth, STABLE ? vis : a.visibility, id) ? 1u : 0u;
							}
						}
					}
					const uint64_t q = __ballot(large);
					if (large)
					{
						// the raw index bytes: the wave reruns rd_setup on them (same inputs, same bits)
						const uint32_t at = queued + (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(q >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)q, 0u));
						queue[at] = t | ia << 8 | ib << 16 | ic << 24;
					}
					queued += (uint32_t)__builtin_popcountll(q);
				}
				else
				{
					const uint32_t t = tb + lane;
					uint32_t ia = 0, ib = 0, ic = 0, pieces = 0;
					int4 p0 = make_int4(0, 0, 0, 1), p1 = p0, p2 = p0, p3 = p0;
					if (t < te)
					{
						const uint32_t o = indexOffset * 4 + t * 3;
						ia = data8[o], ib = data8[o + 1], ic = data8[o + 2];
						if (ia < ve && ib < ve && ic < ve)
							pieces = rd_clip(a.globals, vtx[ia], vtx[ib], vtx[ic], cvx[ia], cvx[ib], cvx[ic], H, p0, p1, p2, p3);
					}
					for (uint32_t p = 0; p < 2u; ++p)
					{
						if (!__ballot(p < pieces)) // (wave-uniform)
							break;
						RdTri tri;
						bool large = false;
						const bool live = p < pieces && rd_setup_corners(p0, rd_sel(p != 0u, p2, p1), rd_sel(p != 0u, p3, p2), bothFaces, W, H, tri);
						if (live)
						{
							drawn += 1;
							if (tri.x0 <= tri.x1 && tri.y0 <= tri.y1)
							{
								const uint32_t n = (uint32_t)(tri.x1 - tri.x0 + 1) * (uint32_t)(tri.y1 - tri.y0 + 1);
								large = n > a.smallLimit;
								if (!large)
								{
									const auto id = rd_id<STABLE>(index, mvi, t);
									for (int32_t py = tri.y0; py <= tri.y1; ++py)
										for (int32_t px = tri.x0; px <= tri.x1; ++px)
											samples += rd_sample<STABLE>(tri, px, py, a.width, a.depth, STABLE ? vis : a.visibility, id) ? 1u : 0u;
								}
							}
						}
						const uint64_t q = __ballot(large);
						if (large)
						{
							// the raw index bytes: the wave reruns the setup on them (same inputs, same bits)
							const uint32_t at = queued + (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(q >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)q, 0u));
							queue[at] = t | p << 7 | ia << 8 | ib << 16 | ic << 24; // (t < 96; at < 96 * PIECES: each (t, p) once)
						}
						queued += (uint32_t)__builtin_popcountll(q);
					}
				}
			}
			rd_lds_order();

			// ---- large triangles, the whole wave: lane = pixel of an 8 x 8 stamp
			for (uint32_t k = 0; k < queued; ++k)
			{
				const uint32_t e = queue[k];
				RdTri tri;
				decltype(rd_id<STABLE>(0u, 0u, 0u)) id;
				if constexpr (CLIP)
				{
					const uint32_t ia = e >> 8 & 0xffu, ib = e >> 16 & 0xffu, ic = e >> 24; // (< ve: it was queued)
					const bool second = (e & 0x80u) != 0u;
					int4 p0, p1, p2, p3;
					rd_clip(a.globals, vtx[ia], vtx[ib], vtx[ic], cvx[ia], cvx[ib], cvx[ic], H, p0, p1, p2, p3);
					rd_setup_corners(p0, rd_sel(second, p2, p1), rd_sel(second, p3, p2), bothFaces, W, H, tri); // (true: it was queued)
					id = rd_id<STABLE>(index, mvi, e & 0x7fu);
				}
				else
				{
					rd_setup(vtx, e >> 8 & 0xffu, e >> 16 & 0xffu, e >> 24, ve, bothFaces, W, H, tri); // (true: it was queued)
					id = rd_id<STABLE>(index, mvi, e & 0xffu);
				}
				const uint32_t sw = (uint32_t)(tri.x1 - tri.x0) / 8u + 1u, sh = (uint32_t)(tri.y1 - tri.y0) / 8u + 1u;
				const int32_t lx = (int32_t)(lane & 7u), ly = (int32_t)(lane >> 3);
				for (uint32_t sy = 0; sy < sh; ++sy)
				{
					const int32_t py = tri.y0 + (int32_t)sy * 8 + ly;
					for (uint32_t sx = 0; sx < sw; ++sx)
					{
						const int32_t px = tri.x0 + (int32_t)sx * 8 + lx;
						if (px <= tri.x1 && py <= tri.y1)
							samples += rd_sample<STABLE>(tri, px, py, a.width, a.depth, STABLE ? vis : a.visibility, id) ? 1u : 0u;
					}
				}
			}
		}
	}

	// totals: per-workgroup partial sums, plain stores; rasterdepth_totals_kernel adds them up
	__shared__ unsigned long long s_tot[RD_WAVES][4];
	unsigned long long d = drawn, smp = samples;
	for (int o = 32; o > 0; o >>= 1)
	{
		d += __shfl_xor(d, o, 64);
		smp += __shfl_xor(smp, o, 64);
	}
	if (lane == 0)
	{
		s_tot[wave][0] = clusters;
		s_tot[wave][1] = triangles;
		s_tot[wave][2] = d;
		s_tot[wave][3] = smp;
	}
	__syncthreads();
	if (threadIdx.x < 4)
	{
		unsigned long long t = 0;
#pragma unroll
		for (int k = 0; k < RD_WAVES; ++k)
			t += s_tot[k][threadIdx.x];
		a.partials[(size_t)blockIdx.x * 4 + threadIdx.x] = t;
	}
}

// adds the per-workgroup partial sums of a launch to the caller's four totals (one workgroup)
__global__ __launch_bounds__(256) void rasterdepth_totals_kernel(const unsigned long long* __restrict__ partials, uint32_t blocks,
                                                                 unsigned long long* __restrict__ totals)
{
	__shared__ unsigned long long s_part[4][4];
	unsigned long long t[4] = { 0, 0, 0, 0 };
	for (uint32_t i = threadIdx.x; i < blocks; i += 256)
#pragma unroll
		for (int k = 0; k < 4; ++k)
			t[k] += partials[(size_t)i * 4 + k];
#pragma unroll
	for (int k = 0; k < 4; ++k)
		for (int o = 32; o > 0; o >>= 1)
			t[k] += __shfl_xor(t[k], o, 64);
	if ((threadIdx.x & 63u) == 0)
		for (int k = 0; k < 4; ++k)
			s_part[threadIdx.x >> 6][k] = t[k];
	__syncthreads();
	if (threadIdx.x < 4)
		totals[threadIdx.x] += s_part[0][threadIdx.x] + s_part[1][threadIdx.x] + s_part[2][threadIdx.x] + s_part[3][threadIdx.x];
}

int launch_raster_totals(hipStream_t stream, const unsigned long long* partials, uint32_t blocks, unsigned long long* totals)
{
	hipLaunchKernelGGL(rasterdepth_totals_kernel, dim3(1), dim3(256), 0, stream, partials, blocks, totals);
	return (int)hipGetLastError();
}

int launch_rasterdepth(hipStream_t stream, const RasterArgs& a, uint32_t gridBlocks, bool nearClip, bool stableIds)
{
	gridBlocks = gridBlocks / 8 * RD_BLOCKS_PER_CU; // the caller passes 8 workgroups per CU, the size of `partials`
	// (the stable form differs only in the visibility word: without a visibility target the launch is the default kernel)
	if (stableIds && a.visibility)
	{
		if (nearClip)
			hipLaunchKernelGGL((rasterdepth_kernel<true, true>), dim3(gridBlocks), dim3(RD_THREADS), 0, stream, a);
		else
			hipLaunchKernelGGL((rasterdepth_kernel<false, true>), dim3(gridBlocks), dim3(RD_THREADS), 0, stream, a);
	}
	else if (nearClip)
		hipLaunchKernelGGL((rasterdepth_kernel<true, false>), dim3(gridBlocks), dim3(RD_THREADS), 0, stream, a);
	else
		hipLaunchKernelGGL((rasterdepth_kernel<false, false>), dim3(gridBlocks), dim3(RD_THREADS), 0, stream, a);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess || !a.totals)
		return (int)e;
	return launch_raster_totals(stream, a.partials, gridBlocks, a.totals);
}

} // namespace nv
