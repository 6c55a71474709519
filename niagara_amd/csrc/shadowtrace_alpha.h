// shadowtrace_alpha.h — the alpha-tested shadow trace over either residency of the texture set: shadowtrace.h's tile walk
// with rtalpha.h's rt_occluded_alpha as its ray query, and its launch.  shadowtrace_alpha.hip instantiates it over the decoded set,
// shadowtrace_blocks.hip over the block-resident one.
#pragma once
#include "shadowtrace.h"
#include "rtalpha.h"

namespace nv
{

struct AlphaQuery
{
	template <typename ARGS>
	static NV_DEV bool occluded(const ARGS& a, rt3 origin, rt3 dir) { return rt_occluded_alpha(a.scene, a.in, origin, dir, 1e-2f, 1e3f); } // :86-123
};

template <typename ARGS>
int launch_shadow_trace_set(hipStream_t stream, ARGS a, uint32_t maxBlocks)
{
	const uint32_t grid = shadow_trace_complete(a, maxBlocks);
	hipLaunchKernelGGL((shadow_trace_kernel<AlphaQuery, ARGS>), dim3(grid), dim3(ST_THREADS), 0, stream, a);
	return (int)hipGetLastError();
}

} // namespace nv
