// visattr_blocks.hip — nv_visibility_attributes_blocks: the textured attribute pass over a block-resident texture set.
//
// The pass is visattr.h's kernel with TEX, the text nv_visibility_attributes_textured runs, instantiated with VisAttrBlockArgs: its a.tx is the
// block set, and the va_texture below is the one the kernel's calls resolve to.  The sampler is texmath.h's over a texel source; the block
// source loads a tap's block — 8 bytes for BC1, otherwise 16 in one load — once per distinct block of a level's four taps and decodes the
// tap's texel from it.  The codes are the decoded chain's and every operation after the fetch is the decoded sampler's, so the outputs are
// nv_visibility_attributes_textured's bit for bit.  Format and BC7 mode differ between the lanes of a wave; nothing here is wave-uniform by
// assumption.  One launch, no scratch memory, only enqueued work.
#include "texmath.h" // in full, ahead of fragalpha.h's sampler-only inclusion: this translation unit decodes
#include "visattr.h"

namespace nv
{

// texture(SAMP(id), uv) from the block set.  false: id is past the table or tx_block_desc_ok refused the descriptor — nothing was loaded from
// the block buffer; the caller shades from the factors and counts the pixel.
NV_DEV bool va_texture(const VaBlockTextures& tx, uint32_t id, float u, float v, float dudx, float dvdx, float dudy, float dvdy, TxF4& c)
{
	if (id >= tx.count)
		return false;
	const uint4 w = tx.descs[id];
	const TxBlockDesc d = { w.x, w.y, w.z, w.w };
	if (!tx_block_desc_ok(d, tx.units16))
		return false;
	c = tx_sample(tx_block_source(tx.blocks, d), u, v, dudx, dvdx, dudy, dvdy);
	return true;
}

int launch_visibility_attributes_blocks(hipStream_t stream, VisAttrBlockArgs a, uint32_t height, uint32_t maxBlocks)
{
	const uint32_t grid = va_complete(a, height, maxBlocks);
	hipLaunchKernelGGL((visibility_attributes_kernel<true, true, VisAttrBlockArgs>), dim3(grid), dim3(VA_THREADS), 0, stream, a);
	return (int)hipGetLastError();
}

} // namespace nv
