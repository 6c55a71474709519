// visattr_blocks.hip — nv_visibility_attributes_blocks: the textured attribute pass over a block-resident texture set.
//
// The pass is visattr.h's kernel with TEX, the text nv_visibility_attributes_textured runs, over TxBlocks.  The sampler is texmath.h's over a texel
// source; the block source loads a tap's block — 8 bytes for BC1, otherwise 16 in one load — once per distinct block of a level's four taps and
// decodes the tap's texel from it.  The codes are the decoded chain's and every operation after the fetch is the decoded sampler's, so the outputs
// are nv_visibility_attributes_textured's bit for bit.  Format and BC7 mode differ between the lanes of a wave; nothing here is wave-uniform by
// assumption.  One launch, no scratch memory, only enqueued work.
#include "texmath.h" // in full, ahead of fragalpha.h's sampler-only inclusion: this translation unit decodes
#include "visattr.h"

namespace nv
{

int launch_visibility_attributes_blocks(hipStream_t stream, VisAttrBlockArgs a, uint32_t height, uint32_t maxBlocks)
{
	return launch_visibility_attributes_set(stream, a, height, maxBlocks);
}

} // namespace nv
