// rasterindexed_alpha.hip — nv_rasterdepth_indexed_textured: the indexed-draw raster with the POST alpha discard as coverage (DESIGN.md §4.24;
// mesh.frag.glsl:88).
//
// The pass is rasterindexed.h's kernel — chunk search, per-lane set-up, clipping, both raster paths: shared with nv_rasterdepth_indexed and
// nv_rasterdepth_indexed_visibility, not copied — instantiated on RasterIndexedSetArgs<SET>.  Where a wave loads its current command's
// transform it also loads, wave-uniform, the draw's materialIndex, the material's albedoTexture and diffuseFactor.a and the texture's
// descriptor (rasterdepth.h's rd_alpha_slot: each load behind the check that keeps it inside its table).  A lane of an alpha-tested command
// keeps the three corners of its ORIGINAL triangle (clip x, y, w, packed texcoord) in registers; a queued piece carries them in an LDS array
// of its own.  A covered sample is §4.20's rd_sample_alpha: the attribute pass's arithmetic (fragalpha.h), the albedo texture through the
// set's sampler, and no load or atomic on either target when albedo.a < 0.5.  Alpha is evaluated for EVERY covered sample of a tested command,
// so the kept and dropped counts do not depend on the order of the GPU's work.
// This file instantiates the kernel over the decoded set, rasterindexed_blocks.hip over the block-resident one.
#include "rasterindexed.h"

namespace nv
{

int launch_rasterindexed_alpha(hipStream_t stream, RasterIndexedAlphaArgs a, void* scratch, uint32_t gridBlocks, bool nearClip)
{
	return launch_rasterindexed_as(stream, a, scratch, gridBlocks, nearClip);
}

} // namespace nv
