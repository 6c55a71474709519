// depthmerge.hip — the depth composite of a sharded frame for gfx950.
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

namespace nv
{

constexpr int DEPTH_MERGE_MAX = 8; // sources per launch: the host folds longer lists in groups (the destination accumulates)

struct DepthMergeArgs
{
	uint32_t* dst;
	const uint32_t* src[DEPTH_MERGE_MAX];
	uint32_t n4; // whole 16-B groups (0 when a pointer is not 16-B aligned: everything goes through the scalar loop)
	uint32_t n;  // texels, <= 16384 * 16384
};

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

template <int K>
__global__ __launch_bounds__(256) void depth_merge_kernel(DepthMergeArgs a)
{
	const uint32_t stride = gridDim.x * 256u;
	const uint32_t first = blockIdx.x * 256u + threadIdx.x;
	for (uint32_t i = first; i < a.n4; i += stride)
	{
		v4u s[K];
#pragma unroll
		for (int k = 0; k < K; ++k)
			s[k] = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(a.src[k]) + i);
		v4u d = reinterpret_cast<const v4u*>(a.dst)[i];
#pragma unroll
		for (int k = 0; k < K; ++k)
		{
			d.x = umax(d.x, s[k].x);
			d.y = umax(d.y, s[k].y);
			d.z = umax(d.z, s[k].z);
			d.w = umax(d.w, s[k].w);
		}
		reinterpret_cast<v4u*>(a.dst)[i] = d;
	}
	// the ragged end (at most 3 texels), or the whole buffer when a pointer is not 16-B aligned
	for (uint32_t i = a.n4 * 4u + first; i < a.n; i += stride)
	{
		uint32_t d = a.dst[i];
#pragma unroll
		for (int k = 0; k < K; ++k)
			d = umax(d, a.src[k][i]);
		a.dst[i] = d;
	}
}

template <int K>
static void launch_k(hipStream_t stream, const DepthMergeArgs& a, uint32_t grid)
{
	hipLaunchKernelGGL(depth_merge_kernel<K>, dim3(grid), dim3(256), 0, stream, a);
}

int launch_depth_merge(hipStream_t stream, float* dst, const float* const* srcs, uint32_t sources, uint32_t n, uint32_t maxBlocks)
{
	for (uint32_t at = 0; at < sources; at += DEPTH_MERGE_MAX)
	{
		const uint32_t k = sources - at < (uint32_t)DEPTH_MERGE_MAX ? sources - at : (uint32_t)DEPTH_MERGE_MAX;
		DepthMergeArgs a;
		a.dst = reinterpret_cast<uint32_t*>(dst);
		uintptr_t bits = reinterpret_cast<uintptr_t>(dst);
		for (uint32_t i = 0; i < (uint32_t)DEPTH_MERGE_MAX; ++i)
		{
			a.src[i] = reinterpret_cast<const uint32_t*>(srcs[at + (i < k ? i : 0)]);
			bits |= reinterpret_cast<uintptr_t>(a.src[i]);
		}
		a.n = n;
		a.n4 = (bits & 15u) ? 0u : n / 4u;
		const uint32_t work = a.n4 ? a.n4 + 3u : n; // threads that have something to do
		uint32_t grid = (work + 255u) / 256u;
		grid = grid < maxBlocks ? grid : maxBlocks;
		switch (k)
		{
		case 1: launch_k<1>(stream, a, grid); break;
		case 2: launch_k<2>(stream, a, grid); break;
		case 3: launch_k<3>(stream, a, grid); break;
		case 4: launch_k<4>(stream, a, grid); break;
		case 5: launch_k<5>(stream, a, grid); break;
		case 6: launch_k<6>(stream, a, grid); break;
		case 7: launch_k<7>(stream, a, grid); break;
		default: launch_k<8>(stream, a, grid); break;
		}
	}
	return (int)hipGetLastError();
}

// ---- nv_visibility_merge: the same composite for the stable-ID visibility buffer
//
// dst[i] = max(dst[i], src_0[i], ..., src_{K-1}[i]) on unsigned 64-bit words.  Every shard writes the same word for the same sample
// (NV_OPT_RASTER_VISIBILITY_ID 1), so the maximum over the shards is the word one pass over all draws leaves.  The shape of the depth merge
// with twice the bytes per element: one thread owns a PAIR of words (16-B loads and stores), no atomics, a scalar tail for an odd count.

struct VisMergeArgs
{
	unsigned long long* dst;
	const unsigned long long* src[DEPTH_MERGE_MAX];
	uint32_t n2; // whole 16-B pairs (0 when a pointer is not 16-B aligned)
	uint32_t n;  // words, <= 16384 * 16384
};

typedef unsigned long long v2ull __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned long long umax64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

template <int K>
__global__ __launch_bounds__(256) void visibility_merge_kernel(VisMergeArgs a)
{
	const uint32_t stride = gridDim.x * 256u;
	const uint32_t first = blockIdx.x * 256u + threadIdx.x;
	for (uint32_t i = first; i < a.n2; i += stride)
	{
		v2ull s[K];
#pragma unroll
		for (int k = 0; k < K; ++k)
			s[k] = __builtin_nontemporal_load(reinterpret_cast<const v2ull*>(a.src[k]) + i);
		v2ull d = reinterpret_cast<const v2ull*>(a.dst)[i];
#pragma unroll
		for (int k = 0; k < K; ++k)
		{
			d.x = umax64(d.x, s[k].x);
			d.y = umax64(d.y, s[k].y);
		}
		reinterpret_cast<v2ull*>(a.dst)[i] = d;
	}
	// the odd last word, or the whole buffer when a pointer is not 16-B aligned
	for (uint32_t i = a.n2 * 2u + first; i < a.n; i += stride)
	{
		unsigned long long d = a.dst[i];
#pragma unroll
		for (int k = 0; k < K; ++k)
			d = umax64(d, a.src[k][i]);
		a.dst[i] = d;
	}
}

template <int K>
static void launch_vk(hipStream_t stream, const VisMergeArgs& a, uint32_t grid)
{
	hipLaunchKernelGGL(visibility_merge_kernel<K>, dim3(grid), dim3(256), 0, stream, a);
}

int launch_visibility_merge(hipStream_t stream, unsigned long long* dst, const unsigned long long* const* srcs, uint32_t sources, uint32_t n, uint32_t maxBlocks)
{
	for (uint32_t at = 0; at < sources; at += DEPTH_MERGE_MAX)
	{
		const uint32_t k = sources - at < (uint32_t)DEPTH_MERGE_MAX ? sources - at : (uint32_t)DEPTH_MERGE_MAX;
		VisMergeArgs a;
		a.dst = dst;
		uintptr_t bits = reinterpret_cast<uintptr_t>(dst);
		for (uint32_t i = 0; i < (uint32_t)DEPTH_MERGE_MAX; ++i)
		{
			a.src[i] = srcs[at + (i < k ? i : 0)];
			bits |= reinterpret_cast<uintptr_t>(a.src[i]);
		}
		a.n = n;
		a.n2 = (bits & 15u) ? 0u : n / 2u;
		const uint32_t work = a.n2 ? a.n2 + 1u : n; // threads that have something to do
		uint32_t grid = (work + 255u) / 256u;
		grid = grid < maxBlocks ? grid : maxBlocks;
		switch (k)
		{
		case 1: launch_vk<1>(stream, a, grid); break;
		case 2: launch_vk<2>(stream, a, grid); break;
		case 3: launch_vk<3>(stream, a, grid); break;
		case 4: launch_vk<4>(stream, a, grid); break;
		case 5: launch_vk<5>(stream, a, grid); break;
		case 6: launch_vk<6>(stream, a, grid); break;
		case 7: launch_vk<7>(stream, a, grid); break;
		default: launch_vk<8>(stream, a, grid); break;
		}
	}
	return (int)hipGetLastError();
}

} // namespace nv
