// depthmerge.hip — the composites of a sharded frame for gfx950: nv_depth_merge and nv_visibility_merge, ONE kernel text for the
// two word types.
//
// Every shard of a frame rasterises its own draws into its own depth target; the frame's target is the element-wise maximum of the
// shards' (reverse-Z in [0, 1]: the maximum of the floats is the unsigned maximum of their bits, the rule the rasterisers' atomics
// use).  dst[i] = max(dst[i], src_0[i], ..., src_{K-1}[i]) on the BIT PATTERNS, as unsigned integers: an exact, commutative and
// associative operation, so the composite does not depend on how the draws were split or in which order the targets are folded.
// NaN and negative patterns are not special: they order by their bits (a set sign bit is above every positive float).
//
// Memory-bound: (K + 2) x 4 bytes per texel and one v_max_u32 per source.  One thread owns an element, so there are no atomics; 16-B
// loads and stores, every source's load of an iteration issued before the first max (K is a template parameter), a grid bounded by the
// device (grid-stride loop) and a scalar tail for the last n % 4 texels.  The sources are read once: non-temporal loads, like the
// pyramid build's read of the target (depthreduce.hip); the destination is stored cacheable, the pyramid build reads it next.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch.h"

namespace nv
{

// nv_visibility_merge is the same composite for the stable-ID visibility buffer: dst[i] = max(dst[i], src_0[i], ...,
// src_{K-1}[i]) on unsigned 64-bit words.  Every shard writes the same word for the same sample (NV_OPT_RASTER_VISIBILITY_ID 1), so the maximum
// over the shards is the word one pass over all draws leaves.  Twice the bytes per element: a thread owns a PAIR of words per 16-B group.

constexpr int MERGE_MAX = 8; // sources per launch: the host folds longer lists in groups (the destination accumulates)

// W = uint32_t (depth bits) or unsigned long long (visibility words)
template <typename W>
struct MergeArgs
{
	W* dst;
	const W* src[MERGE_MAX];
	uint32_t nv; // whole 16-B groups (0 when a pointer is not 16-B aligned: everything goes through the scalar loop)
	uint32_t n;  // words, <= 16384 * 16384
};

template <typename W, int K>
__global__ __launch_bounds__(256) void merge_kernel(MergeArgs<W> a)
{
	constexpr uint32_t PER = 16u / sizeof(W); // words of a 16-B group
	typedef W vec __attribute__((ext_vector_type(PER)));
	const uint32_t stride = gridDim.x * 256u;
	const uint32_t first = blockIdx.x * 256u + threadIdx.x;
	for (uint32_t i = first; i < a.nv; i += stride)
	{
		vec s[K];
#pragma unroll
		for (int k = 0; k < K; ++k)
			s[k] = __builtin_nontemporal_load(reinterpret_cast<const vec*>(a.src[k]) + i);
		vec d = reinterpret_cast<const vec*>(a.dst)[i];
#pragma unroll
		for (int k = 0; k < K; ++k)
#pragma unroll
			for (uint32_t j = 0; j < PER; ++j)
				d[j] = d[j] > s[k][j] ? d[j] : s[k][j];
		reinterpret_cast<vec*>(a.dst)[i] = d;
	}
	// the ragged end (fewer words than a group), or the whole buffer when a pointer is not 16-B aligned
	for (uint32_t i = a.nv * PER + first; i < a.n; i += stride)
	{
		W d = a.dst[i];
#pragma unroll
		for (int k = 0; k < K; ++k)
			d = d > a.src[k][i] ? d : a.src[k][i];
		a.dst[i] = d;
	}
}

template <typename W, int K>
static void launch_k(hipStream_t stream, const MergeArgs<W>& a, uint32_t grid)
{
	hipLaunchKernelGGL((merge_kernel<W, K>), dim3(grid), dim3(256), 0, stream, a);
}

template <typename W>
static int launch_merge(hipStream_t stream, W* dst, const W* const* srcs, uint32_t sources, uint32_t n, uint32_t maxBlocks)
{
	constexpr uint32_t PER = 16u / sizeof(W);
	for (uint32_t at = 0; at < sources; at += MERGE_MAX)
	{
		const uint32_t k = sources - at < (uint32_t)MERGE_MAX ? sources - at : (uint32_t)MERGE_MAX;
		MergeArgs<W> a;
		a.dst = dst;
		uintptr_t bits = reinterpret_cast<uintptr_t>(dst);
		for (uint32_t i = 0; i < (uint32_t)MERGE_MAX; ++i)
		{
			a.src[i] = srcs[at + (i < k ? i : 0)];
			bits |= reinterpret_cast<uintptr_t>(a.src[i]);
		}
		a.n = n;
		a.nv = (bits & 15u) ? 0u : n / PER;
		const uint32_t work = a.nv ? a.nv + (PER - 1u) : n; // threads that have something to do
		const uint32_t grid = capped_grid(work, 256u, maxBlocks);
		switch (k)
		{
		case 1: launch_k<W, 1>(stream, a, grid); break;
		case 2: launch_k<W, 2>(stream, a, grid); break;
		case 3: launch_k<W, 3>(stream, a, grid); break;
		case 4: launch_k<W, 4>(stream, a, grid); break;
		case 5: launch_k<W, 5>(stream, a, grid); break;
		case 6: launch_k<W, 6>(stream, a, grid); break;
		case 7: launch_k<W, 7>(stream, a, grid); break;
		default: launch_k<W, 8>(stream, a, grid); break;
		}
	}
	return (int)hipGetLastError();
}

int launch_depth_merge(hipStream_t stream, float* dst, const float* const* srcs, uint32_t sources, uint32_t n, uint32_t maxBlocks)
{
	return launch_merge(stream, reinterpret_cast<uint32_t*>(dst), reinterpret_cast<const uint32_t* const*>(srcs), sources, n, maxBlocks);
}

int launch_visibility_merge(hipStream_t stream, unsigned long long* dst, const unsigned long long* const* srcs, uint32_t sources, uint32_t n, uint32_t maxBlocks)
{
	return launch_merge(stream, dst, srcs, sources, n, maxBlocks);
}

} // namespace nv
