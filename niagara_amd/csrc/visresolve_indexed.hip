// visresolve_indexed.hip — nv_visibility_resolve_indexed: the visibility target of nv_rasterdepth_indexed_visibility back to {draw, index
// position, vertex offset, depth bits} for gfx950.
//
// The word is bits(z) << 34 | (tri34 + 1), tri34 = triangleOffsets[draw] + t: the draw is the last one whose offset is <= tri34 (the offsets
// are the non-decreasing prefix nv_assign_triangle_offsets writes), the LOD is what drawcull.comp.glsl:104-112 selects for that draw under the
// frame's CullData (cullmath.h lod_distance / lod_pick, the statements nv_visibility_resolve runs), and the record names what
// drawcull.comp.glsl:145-150 put into the draw's command: indexPosition = lods[lod].indexOffset + 3 t and the mesh's vertexOffset.
//
// Shape, as visresolve.hip: one lane per pixel of a persistent grid stepping by whole waves, the words read once (non-temporal), one 16-byte
// store per lane.  The search and the LOD select run once per DRAW a wave sees, never per triangle: the first lane that is still open names
// a triangle, the whole wave searches for its draw with wave-uniform (scalar) loads, and every open lane whose tri34 lies in that draw's span
// [offsets[d], offsets[d + 1]) takes the result and closes — a run of equal draw closes in one trip, and so do its other runs in the wave.
// d_drawPixels gets one add per trip.  The trips are serial, so they are bounded: after VRI_TRIPS of them (a wave that shows more draws than
// that: an image of many small draws) the lanes still open search for themselves, all at once, as visresolve.hip's starting lanes do.
// Totals per lane, per wave, per workgroup.  No workgroup waits on another, nothing is allocated, no scratch memory: the entry point only
// enqueues and can be captured.
#include "cullmath.h"
#include "launch.h"

namespace nv
{

constexpr int VRI_THREADS = 256;
constexpr uint32_t VRI_ID_BITS = 34;

constexpr uint32_t VRI_TRIPS = 4; // wave-uniform trips before the lanes that are still open search for themselves

NV_DEV unsigned long long vri_uniform_u64(unsigned long long v, uint32_t lane)
{
	const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)lane);
	const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)lane);
	return (unsigned long long)hi << 32 | lo;
}

// the number of draws whose offset is <= want: draws [0, lo) have one, draws [lo, drawCount) a larger one (wave-uniform for a uniform `want`)
NV_DEV uint32_t vri_search(const VisResolveIndexedArgs& a, unsigned long long want)
{
	uint32_t lo = 0, hi = a.drawCount;
	while (lo < hi)
	{
		const uint32_t mid = (lo + hi) >> 1;
		if (a.triangleOffsets[mid] <= want)
			lo = mid + 1u;
		else
			hi = mid;
	}
	return lo;
}

// The record of triangle tri34 of draw d, whose span starts at `first` (offsets[d] <= tri34: the caller's).  false: unresolved.
NV_DEV bool vri_record(const VisResolveIndexedArgs& a, uint32_t d, unsigned long long first, unsigned long long tri34, unsigned long long total,
                       uint32_t& position, uint32_t& vertexOffset)
{
	const float4* p = reinterpret_cast<const float4*>(a.draws + d);
	const float4 d0 = p[0], d1 = p[1]; // position.xyz, scale | orientation
	const uint32_t meshIndex = *reinterpret_cast<const uint32_t*>(p + 2);
	if (meshIndex >= a.meshCount)
		return false;
	const char* mesh = reinterpret_cast<const char*>(a.meshes + meshIndex);
	uint32_t lod = 0;
	if (a.cd.lodEnabled == 1)
	{
		// drawcull.comp.glsl:73-75 and :104-112, the statements of visresolve.hip's vr_lookup
		const float4 cr = *reinterpret_cast<const float4*>(mesh); // center.xyz, radius
		const f3 c = sphere_center(a.cd, f3{ cr.x, cr.y, cr.z }, f3{ d1.x, d1.y, d1.z }, d1.w, d0.w, f3{ d0.x, d0.y, d0.z });
		const float distance = lod_distance(c, cr.w * d0.w);
		const float threshold = distance * a.cd.lodTarget / d0.w;
		const uint32_t lodCount = *reinterpret_cast<const uint32_t*>(mesh + 32);
		float err[NV_MAX_LODS];
#pragma unroll
		for (uint32_t k = 1; k < NV_MAX_LODS; ++k)
			err[k] = *reinterpret_cast<const float*>(mesh + 48 + 20 * k + 16);
		lod = lod_pick(lodCount, err, threshold);
	}
	const uint32_t indexOffset = *reinterpret_cast<const uint32_t*>(mesh + 48 + 20 * lod);
	const uint32_t indexCount = *reinterpret_cast<const uint32_t*>(mesh + 48 + 20 * lod + 4);
	vertexOffset = *reinterpret_cast<const uint32_t*>(mesh + 16);
	const unsigned long long t = tri34 - first;
	const unsigned long long at = (unsigned long long)indexOffset + 3ull * t;
	position = (uint32_t)at;
	return tri34 < total && t < (unsigned long long)(indexCount / 3u) && at + 2ull <= 0xffffffffull;
}

__global__ __launch_bounds__(VRI_THREADS) void visibility_resolve_indexed_kernel(VisResolveIndexedArgs a)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t stride = gridDim.x * VRI_THREADS;
	const unsigned long long total = a.triangleOffsets[a.drawCount]; // (wave-uniform; the array holds drawCount + 1 entries)
	uint32_t covered = 0, unresolved = 0; // per lane

	// `base` is the wave's first pixel: the loop is uniform over the wave, so the ballots below see all 64 lanes
	for (uint32_t base = blockIdx.x * VRI_THREADS + wave * 64u; base < a.n; base += stride)
	{
		const uint32_t i = base + lane;
		const bool in = i < a.n;
		const unsigned long long word = __builtin_nontemporal_load(a.visibility + (in ? i : base));
		const unsigned long long id = word & ((1ull << VRI_ID_BITS) - 1ull);
		const bool has = in && word != 0ull;
		const bool named = has && id != 0ull; // (a word without an id is not the rasteriser's: unresolved)
		const unsigned long long tri34 = id - 1ull;

		uint32_t drawId = ~0u, indexPosition = 0u, vertexOffset = 0u;
		bool resolved = false;
		uint64_t open = __ballot(named);
		for (uint32_t trip = 0; open != 0ull && trip < VRI_TRIPS; ++trip) // (wave-uniform)
		{
			const uint32_t leader = (uint32_t)__builtin_ctzll(open);
			const unsigned long long want = vri_uniform_u64(tri34, leader);
			const uint32_t lo = vri_search(a, want);
			// the span this trip closes: tri34 in [first, end); the leader's lies in it
			const unsigned long long first = lo ? a.triangleOffsets[lo - 1u] : 0ull;
			const unsigned long long end = lo < a.drawCount ? a.triangleOffsets[lo] : ~0ull;
			const bool mine = (open >> lane & 1ull) != 0ull && tri34 >= first && tri34 < end;
			if (lo != 0u) // (else: no draw has an offset <= tri34)
			{
				const uint32_t d = lo - 1u;
				uint32_t position = 0u, vo = 0u;
				const bool ok = vri_record(a, d, first, tri34, total, position, vo) && mine;
				if (ok)
					drawId = d, indexPosition = position, vertexOffset = vo, resolved = true;
				// one add per trip: the span's resolved pixels, by the leader
				const uint32_t count = (uint32_t)__builtin_popcountll(__ballot(ok));
				if (a.drawPixels && lane == leader && count != 0u)
					atomicAdd(a.drawPixels + d, count);
			}
			open &= ~(__ballot(mine) | 1ull << leader);
		}
		// more draws in this wave than trips (an image of many small draws): every lane that is still open searches for itself, all at once
		if (open >> lane & 1ull)
		{
			const uint32_t lo = vri_search(a, tri34);
			if (lo != 0u)
			{
				const uint32_t d = lo - 1u;
				uint32_t position = 0u, vo = 0u;
				if (vri_record(a, d, a.triangleOffsets[d], tri34, total, position, vo))
				{
					drawId = d, indexPosition = position, vertexOffset = vo, resolved = true;
					if (a.drawPixels)
						atomicAdd(a.drawPixels + d, 1u);
				}
			}
		}

		covered += has ? 1u : 0u;
		unresolved += has && !resolved ? 1u : 0u;
		if (a.records && in)
		{
			uint4 r = make_uint4(~0u, 0u, 0u, 0u); // no sample
			if (has)
				r = resolved ? make_uint4(drawId, indexPosition, vertexOffset, (uint32_t)(word >> VRI_ID_BITS)) : make_uint4(~0u, ~0u, ~0u, ~0u);
			a.records[i] = r;
		}
	}

	if (!a.totals)
		return;
	__shared__ uint32_t s_tot[VRI_THREADS / 64][2];
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
		for (int k = 0; k < VRI_THREADS / 64; ++k)
			t += s_tot[k][threadIdx.x];
		if (t)
			atomicAdd(a.totals + threadIdx.x, t);
	}
}

int launch_visibility_resolve_indexed(hipStream_t stream, VisResolveIndexedArgs a, uint32_t maxBlocks)
{
	const uint32_t grid = capped_grid(a.n, VRI_THREADS, maxBlocks);
	hipLaunchKernelGGL(visibility_resolve_indexed_kernel, dim3(grid), dim3(VRI_THREADS), 0, stream, a);
	return (int)hipGetLastError();
}

} // namespace nv
