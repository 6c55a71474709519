// visattr_indexed_blocks.hip — nv_visibility_attributes_indexed_blocks: the textured attribute pass over indexed records and a
// block-resident texture set.
//
// visattr_indexed_tex.hip's pair — visattr.h's kernel with TEX, visattr_indexed.h's set-up — over TxBlocks: a tap's texel is decoded from
// its BC block, to the decoded chain's codes, so the outputs are nv_visibility_attributes_indexed_textured's bit for bit.  One launch, no
// scratch memory, only enqueued work.
#include "texmath.h" // in full, ahead of fragalpha.h's sampler-only inclusion: this translation unit decodes
#include "visattr_indexed.h"

namespace nv
{

template __device__ void va_indexed_dispatch_check(const VisAttrIndexedBlockArgs&, uint4, VaSetup&);

int launch_visibility_attributes_indexed_blocks(hipStream_t stream, VisAttrIndexedBlockArgs a, uint32_t height, uint32_t maxBlocks)
{
	return launch_visibility_attributes_set(stream, a, height, maxBlocks);
}

} // namespace nv
