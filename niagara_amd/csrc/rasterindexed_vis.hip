// rasterindexed_vis.hip — nv_rasterdepth_indexed_visibility: the indexed-draw raster with a stable-form visibility word.
//
// nv_rasterdepth_indexed's three launches and rule set (rasterindexed.hip, rasterindexed.h), and per covered sample also the atomic maximum of
// bits(z) << 34 | (tri34 + 1) into the visibility target, tri34 = triangleOffsets[command.drawId] + t: the name nv_assign_triangle_offsets
// gives triangle t of a draw, whatever pass, LOD, command slot or rank draws it.  The current command's {offsets[drawId], offsets[drawId + 1]}
// are loaded where its transform is (wave-uniform, four SGPRs); a queued piece's id rides in LDS next to its corners.  A triangle outside its
// draw's span, or with tri34 >= 2^34 - 1, writes depth and no word.  The kernel is rasterindexed.h's, instantiated on RasterIndexedVisArgs.
#include "rasterindexed.h"

namespace nv
{

int launch_rasterindexed_vis(hipStream_t stream, RasterIndexedVisArgs a, void* scratch, uint32_t gridBlocks, bool nearClip)
{
	return launch_rasterindexed_as(stream, a, scratch, gridBlocks, nearClip);
}

} // namespace nv
