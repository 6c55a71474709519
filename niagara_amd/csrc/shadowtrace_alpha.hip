// shadowtrace_alpha.hip — nv_shadow_trace_textured at quality 1 for gfx950: shadowTraceTransparent of shadow.comp.glsl:86-123,
// the ray query whose candidates are confirmed by the alpha of their albedo texture.  The traversal is rtalpha.h's rt_occluded_alpha, the text
// nv_rt_scene_trace_host_textured_rays runs on the CPU; the RESULT is defined without the BVH (tests/shadow_alpha_ref.c).
//
// The kernel is shadowtrace.h's tile walk, shared with nv_shadow_trace, not copied.  The lanes of a wave walk the same nodes until the alpha
// test, where they part: a lane whose candidate is transparent goes on while its neighbour has left.  A candidate's four alpha taps are issued
// together and waited for once (TxDecoded::alpha_lod0).  Quality 0 has no alpha test: the entry point dispatches shadowtrace.hip's kernel.
#include "shadowtrace_alpha.h"

namespace nv
{

int launch_shadow_trace_alpha(hipStream_t stream, ShadowTraceAlphaArgs a, uint32_t maxBlocks) { return launch_shadow_trace_set(stream, a, maxBlocks); }

} // namespace nv
