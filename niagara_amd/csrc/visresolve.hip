// visresolve.hip — nv_visibility_resolve: the stable-ID visibility buffer back to {draw, meshlet, triangle} for gfx950.
//
// nv_rasterdepth with NV_OPT_RASTER_VISIBILITY_ID 1 leaves, per pixel, word = bits(z) << 34 | id34 with id34 = ((mvi << 7) | triangle) + 1
// and mvi the cluster's meshlet-visibility bit index (command.meshletVisibilityOffset + lane): a name that depends on the draw and its LOD
// only.  This kernel inverts it: the draw is the last one whose meshletVisibilityOffset is <= mvi (the offsets are the non-decreasing
// prefix nv_assign_visibility_offsets writes), the LOD is what drawcull.comp.glsl:106-118 selects for that draw under the frame's CullData
// (cullmath.h lod_distance / lod_pick: the statements drawcull.hip's decide_post runs), the meshlet is the LOD's meshletOffset + (mvi - offset).
//
// Shape.  Memory-bound: 8 B in, 16 B out per pixel.  One lane per pixel of a persistent grid, the words read once (non-temporal 8-byte
// loads, a wave reads 512 contiguous bytes), the records written with one 16-byte store per lane.  Neighbouring pixels mostly show the
// same cluster, so the prefix search (log2(drawCount) dependent loads) and the LOD select run once per RUN of equal mvi in a wave: a lane
// starts a run when its mvi differs from lane - 1's (one DPP move, one ballot), the starting lanes do the work, and every lane fetches the
// result from the start of its run (ds_bpermute).  The atomics are aggregated the same way: one add to d_drawPixels and one OR into
// d_meshletSeen per run instead of per pixel — a 1920 x 1080 frame of a few thousand clusters would otherwise send two million atomics
// to a few thousand lines.  The totals are summed per lane, per wave (DPP), per workgroup (LDS) and added once per workgroup.
// No workgroup waits on another, nothing is allocated, no scratch memory: the entry point only enqueues and can be captured.
//
// RUNS = false (experiments build, NV_RESOLVE_PER_PIXEL=1) is the kernel without the runs — every named pixel searches and adds for itself —
// kept for the measurement that justifies the runs (profiles/r10_visibility.md).
#include "cullmath.h"
#include "launch.h"

namespace nv
{

constexpr int VR_THREADS = 256;
constexpr uint32_t VR_ID_BITS = 34;

// {drawId or ~0 when mvi names no meshlet, meshletIndex} of the cluster with meshlet-visibility index mvi
NV_DEV uint2 vr_lookup(const VisResolveArgs& a, uint32_t mvi)
{
	// draws [0, lo) have meshletVisibilityOffset <= mvi, draws [hi, drawCount) have a larger one
	uint32_t lo = 0, hi = a.drawCount;
	while (lo < hi)
	{
		const uint32_t mid = (lo + hi) >> 1;
		if (a.draws[mid].meshletVisibilityOffset <= mvi)
			lo = mid + 1u;
		else
			hi = mid;
	}
	if (lo == 0u)
		return make_uint2(~0u, 0u);
	const uint32_t d = lo - 1u;
	const float4* p = reinterpret_cast<const float4*>(a.draws + d);
	const float4 d0 = p[0], d1 = p[1]; // position.xyz, scale | orientation
	const uint4 d2 = *reinterpret_cast<const uint4*>(p + 2); // meshIndex, meshletVisibilityOffset, postPass, materialIndex
	if (d2.x >= a.meshCount)
		return make_uint2(~0u, 0u);
	const char* mesh = reinterpret_cast<const char*>(a.meshes + d2.x);
	uint32_t lod = 0;
	if (a.cd.lodEnabled == 1)
	{
		// drawcull.comp.glsl:73-75 and :104-112, the statements of drawcull.hip's decide_pre (records in place) and decide_post
		const float4 cr = *reinterpret_cast<const float4*>(mesh); // center.xyz, radius
		const f3 c = sphere_center(a.cd, f3{ cr.x, cr.y, cr.z }, f3{ d1.x, d1.y, d1.z }, d1.w, d0.w, f3{ d0.x, d0.y, d0.z });
		const float distance = lod_distance(c, cr.w * d0.w);
		const float threshold = distance * a.cd.lodTarget / d0.w;
		const uint32_t lodCount = *reinterpret_cast<const uint32_t*>(mesh + 32);
		float err[NV_MAX_LODS];
#pragma unroll
		for (uint32_t i = 1; i < NV_MAX_LODS; ++i)
			err[i] = *reinterpret_cast<const float*>(mesh + 48 + 20 * i + 16);
		lod = lod_pick(lodCount, err, threshold);
	}
	const uint32_t meshletOffset = *reinterpret_cast<const uint32_t*>(mesh + 48 + 20 * lod + 8);
	const uint32_t meshletCount = *reinterpret_cast<const uint32_t*>(mesh + 48 + 20 * lod + 12);
	const uint32_t local = mvi - d2.y; // (>= 0: the search)
	if (local >= meshletCount)
		return make_uint2(~0u, 0u);
	return make_uint2(d, meshletOffset + local);
}

template <bool RUNS>
__global__ __launch_bounds__(VR_THREADS) void visibility_resolve_kernel(VisResolveArgs a)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t stride = gridDim.x * VR_THREADS;
	uint32_t covered = 0, unresolved = 0; // per lane

	// `base` is the wave's first pixel: the loop is uniform over the wave, so the DPP move, the ballots and the permutes below see all 64 lanes
	for (uint32_t base = blockIdx.x * VR_THREADS + wave * 64u; base < a.n; base += stride)
	{
		const uint32_t i = base + lane;
		const bool in = i < a.n;
		const unsigned long long word = __builtin_nontemporal_load(a.visibility + (in ? i : base));
		const unsigned long long id = word & ((1ull << VR_ID_BITS) - 1ull);
		const bool has = in && word != 0ull;
		const bool named = has && id != 0ull; // (a word without an id is not the rasteriser's: unresolved)
		const uint32_t mvi = named ? (uint32_t)((id - 1ull) >> 7) : ~0u; // (< 2^27: never ~0)
		const uint32_t triangle = (uint32_t)((id - 1ull) & 127ull);

		uint2 found = make_uint2(~0u, 0u);
		uint64_t starts = ~0ull;
		if (RUNS)
		{
			// (the move is a statement of its own: as the right operand of `lane == 0u || ...` it would run with lane 0 switched off, and lane 1
			// would read its own value instead of lane 0's)
			const uint32_t previous = wave_shift_up1_u32(mvi);
			const bool start = lane == 0u || previous != mvi;
			starts = __ballot(start);
			if (start && named)
				found = vr_lookup(a, mvi);
			// the start of this lane's run: the highest starting lane at or below it (lane 0 always starts one)
			const uint32_t from = 63u - (uint32_t)__builtin_clzll(starts & (~0ull >> (63u - lane)));
			found.x = (uint32_t)__shfl((int)found.x, (int)from, 64);
			found.y = (uint32_t)__shfl((int)found.y, (int)from, 64);
		}
		else if (named)
			found = vr_lookup(a, mvi);

		const bool resolved = named && found.x != ~0u && triangle < 96u;
		covered += has ? 1u : 0u;
		unresolved += has && !resolved ? 1u : 0u;
		if (a.records && in)
		{
			uint4 r = make_uint4(~0u, 0u, 0u, 0u); // no sample
			if (has)
				r = resolved ? make_uint4(found.x, found.y, triangle, (uint32_t)(word >> VR_ID_BITS)) : make_uint4(~0u, ~0u, ~0u, ~0u);
			a.records[i] = r;
		}

		// one add and one OR per run: the run's resolved pixels counted from the ballot by its starting lane
		const uint64_t res = __ballot(resolved);
		uint32_t count = resolved ? 1u : 0u;
		bool adds = resolved;
		if (RUNS)
		{
			const uint64_t above = starts & ~(~0ull >> (63u - lane)); // the starting lanes after this one
			const uint64_t upto = above ? (1ull << __builtin_ctzll(above)) - 1ull : ~0ull;
			count = (uint32_t)__builtin_popcountll(res & upto & ~((1ull << lane) - 1ull));
			adds = (starts >> lane & 1ull) != 0ull && count != 0u; // (count != 0: a lane of the run is resolved, so found.x is a draw)
		}
		if (adds)
		{
			if (a.drawPixels)
				atomicAdd(a.drawPixels + found.x, count);
			if (a.meshletSeen)
				atomicOr(a.meshletSeen + (mvi >> 5), 1u << (mvi & 31u));
		}
	}

	if (!a.totals)
		return;
	__shared__ uint32_t s_tot[VR_THREADS / 64][2];
	const uint32_t wc = wave_sum_u32(covered), wu = wave_sum_u32(unresolved);
	if (lane == 0u)
	{
		s_tot[wave][0] = wc;
		s_tot[wave][1] = wu;
	}
	__syncthreads();
	if (threadIdx.x < 2u)
	{
		unsigned long long t = 0;
#pragma unroll
		for (int k = 0; k < VR_THREADS / 64; ++k)
			t += s_tot[k][threadIdx.x];
		if (t)
			atomicAdd(a.totals + threadIdx.x, t);
	}
}

int launch_visibility_resolve(hipStream_t stream, VisResolveArgs a, uint32_t maxBlocks, bool perPixel)
{
	const uint32_t grid = capped_grid(a.n, VR_THREADS, maxBlocks);
	if (perPixel)
		hipLaunchKernelGGL(visibility_resolve_kernel<false>, dim3(grid), dim3(VR_THREADS), 0, stream, a);
	else
		hipLaunchKernelGGL(visibility_resolve_kernel<true>, dim3(grid), dim3(VR_THREADS), 0, stream, a);
	return (int)hipGetLastError();
}

} // namespace nv
