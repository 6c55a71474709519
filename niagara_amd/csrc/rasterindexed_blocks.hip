// rasterindexed_blocks.hip — nv_rasterdepth_indexed_blocks: nv_rasterdepth_indexed_textured's POST alpha discard over a block-resident
// texture set.
//
// rasterindexed.h's kernel with ALPHA over TxBlocks: a tap's texel is decoded from its BC block, to the decoded chain's codes, so targets
// and counters are nv_rasterdepth_indexed_textured's bit for bit.
#include "texmath.h" // in full, ahead of fragalpha.h's sampler-only inclusion: this translation unit decodes
#include "rasterindexed.h"

namespace nv
{

int launch_rasterindexed_blocks(hipStream_t stream, RasterIndexedBlockArgs a, void* scratch, uint32_t gridBlocks, bool nearClip)
{
	return launch_rasterindexed_as(stream, a, scratch, gridBlocks, nearClip);
}

} // namespace nv
