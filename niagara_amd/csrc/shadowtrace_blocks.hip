// shadowtrace_blocks.hip — nv_shadow_trace_blocks at quality 1 for gfx950: nv_shadow_trace_textured's alpha-tested ray query
// over a block-resident texture set.  The kernel is shadowtrace.h's tile walk and the traversal rtalpha.h's rt_occluded_alpha, the texts
// shadowtrace_alpha.hip runs, over TxBlocks: the descriptor is checked by tx_block_desc_ok and the four alpha taps of level 0 are each decoded
// from their block — alpha alone (tx_decode_alpha), a block loaded once per distinct block of the four taps.  The alpha codes are the decoded
// chain's top bytes and the blend is the same, so the mask is nv_shadow_trace_textured's byte for byte.
#include "texmath.h" // in full, ahead of rtalpha.h's sampler-only inclusion: this translation unit decodes
#include "shadowtrace_alpha.h"

namespace nv
{

int launch_shadow_trace_blocks(hipStream_t stream, ShadowTraceBlockArgs a, uint32_t maxBlocks) { return launch_shadow_trace_set(stream, a, maxBlocks); }

} // namespace nv
