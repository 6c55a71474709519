// shadowtrace.hip — nv_shadow_trace for gfx950: shadow.comp.glsl's ray-traced sun shadow mask on the software BVH that
// rtbuild.cpp builds.  gfx950 has no ray accelerator: the ray query of the shader is rtmath.h's rt_occluded, the same text
// nv_rt_scene_trace_host runs on the CPU, and the RESULT is defined without the BVH (tests/shadow_ref.c tests every triangle).
//
// The kernel is shadowtrace.h's tile walk.  QUALITY is a template parameter (the reference has two pipelines, src/niagara.cpp:1803), not a
// per-lane branch.
#include "shadowtrace.h"

namespace nv
{

template <int QUALITY>
struct OpaqueQuery
{
	static NV_DEV bool occluded(const ShadowTraceArgs& a, rt3 origin, rt3 dir) { return rt_occluded(a.scene, origin, dir, 1e-2f, 1e3f, (uint32_t)QUALITY); }
};

int launch_shadow_trace(hipStream_t stream, ShadowTraceArgs a, int quality, uint32_t maxBlocks)
{
	const uint32_t grid = shadow_trace_complete(a, maxBlocks);
	if (quality == 0)
		hipLaunchKernelGGL((shadow_trace_kernel<OpaqueQuery<0>, ShadowTraceArgs>), dim3(grid), dim3(ST_THREADS), 0, stream, a);
	else
		hipLaunchKernelGGL((shadow_trace_kernel<OpaqueQuery<1>, ShadowTraceArgs>), dim3(grid), dim3(ST_THREADS), 0, stream, a);
	return (int)hipGetLastError();
}

} // namespace nv
