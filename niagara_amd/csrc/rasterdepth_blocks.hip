// rasterdepth_blocks.hip — nv_rasterdepth_blocks: nv_rasterdepth_textured's POST alpha discard over a block-resident texture set (DESIGN.md
// §4.21).  The pass is rasterdepth.h's kernel with ALPHA, the text rasterdepth_alpha.hip instantiates, over TxBlocks: the slot's descriptor is
// checked by tx_block_desc_ok and a tap is decoded from its block to the decoded chain's code, so depth, visibility and every counter are
// nv_rasterdepth_textured's bit for bit.
#include "texmath.h" // in full, ahead of fragalpha.h's sampler-only inclusion: this translation unit decodes
#include "rasterdepth.h"

namespace nv
{

int launch_rasterdepth_blocks(hipStream_t stream, const RasterBlockArgs& a, uint32_t gridBlocks, bool nearClip, bool stableIds)
{
	return launch_rasterdepth_as<true>(stream, a, gridBlocks, nearClip, stableIds);
}

} // namespace nv
