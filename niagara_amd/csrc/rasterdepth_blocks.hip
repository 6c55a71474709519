// rasterdepth_blocks.hip — nv_rasterdepth_blocks: nv_rasterdepth_textured's POST alpha discard over a block-resident texture set (DESIGN.md
// §4.21).  The pass is rasterdepth.h's kernel with ALPHA, the text rasterdepth_alpha.hip instantiates, with RasterBlockArgs; what differs is
// below: the slot's descriptor check (tx_block_desc_ok) and the guarded read, which samples texmath.h's sampler over the block source.  The
// codes are the decoded chain's, so depth, visibility and every counter are nv_rasterdepth_textured's bit for bit.
#include "texmath.h" // in full, ahead of fragalpha.h's sampler-only inclusion: this translation unit decodes
#include "rasterdepth.h"

namespace nv
{

// the block descriptor of a slot's albedo texture, its four words in the slot record's TxDesc (levels = levelsFormat).  false: id is past the
// table or tx_block_desc_ok refused it; nothing is ever loaded from the block buffer through a descriptor this refused.
NV_DEV bool rd_slot_desc(const VaBlockTextures& tx, uint32_t id, TxDesc& d)
{
	if (id >= tx.count)
		return false;
	const uint4 w = tx.descs[id];
	d = TxDesc{ w.x, w.y, w.z, w.w };
	return tx_block_desc_ok(TxBlockDesc{ w.x, w.y, w.z, w.w }, tx.units16);
}

// the slot's albedo texture at (u, v) from the block set: `desc` carries TxBlockDesc's four words (levels = levelsFormat)
NV_DEV TxF4 rd_texture(const unsigned char* blocks, const TxDesc& desc, float u, float v, float dudx, float dvdx, float dudy, float dvdy)
{
	return tx_sample(tx_block_source(blocks, TxBlockDesc{ desc.offset, desc.width, desc.height, desc.levels }), u, v, dudx, dvdx, dudy, dvdy);
}

template <>
struct RdTexels<RasterBlockArgs>
{
	typedef unsigned char type;
	static NV_DEV const type* of(const RasterBlockArgs& a) { return static_cast<const unsigned char*>(a.tx.blocks); }
};

int launch_rasterdepth_blocks(hipStream_t stream, const RasterBlockArgs& a, uint32_t gridBlocks, bool nearClip, bool stableIds)
{
	gridBlocks = gridBlocks / 8 * RD_BLOCKS_PER_CU; // (as launch_rasterdepth_alpha)
	if (stableIds && a.visibility)
	{
		if (nearClip)
			hipLaunchKernelGGL((rasterdepth_kernel<true, true, true, RasterBlockArgs>), dim3(gridBlocks), dim3(RD_THREADS), 0, stream, a);
		else
			hipLaunchKernelGGL((rasterdepth_kernel<false, true, true, RasterBlockArgs>), dim3(gridBlocks), dim3(RD_THREADS), 0, stream, a);
	}
	else if (nearClip)
		hipLaunchKernelGGL((rasterdepth_kernel<true, false, true, RasterBlockArgs>), dim3(gridBlocks), dim3(RD_THREADS), 0, stream, a);
	else
		hipLaunchKernelGGL((rasterdepth_kernel<false, false, true, RasterBlockArgs>), dim3(gridBlocks), dim3(RD_THREADS), 0, stream, a);
	hipError_t e = hipGetLastError();
	if (e == hipSuccess && a.totals)
		e = (hipError_t)launch_raster_totals(stream, a.partials, gridBlocks, a.totals);
	if (e == hipSuccess && a.alphaTotals)
		e = (hipError_t)launch_raster_alpha_totals(stream, a.alphaPartials, gridBlocks, a.alphaTotals);
	return (int)e;
}

} // namespace nv
