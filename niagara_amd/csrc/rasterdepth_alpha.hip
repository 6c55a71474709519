// rasterdepth_alpha.hip — nv_rasterdepth_textured: the depth rasteriser of the visible clusters with the POST alpha discard as coverage
// (mesh.frag.glsl:88).
//
// The pass is rasterdepth.h's kernel — slot headers, vertex stage, set-up, clipping, both raster paths: shared with nv_rasterdepth, not copied —
// instantiated with ALPHA.  With the slot's header a lane also fetches the draw's materialIndex, the material's albedoTexture and
// diffuseFactor.a and the texture's descriptor, each load behind the check that keeps it inside its table; the slot's road is wave-uniform.  The
// vertex stage of an alpha-tested slot keeps one more float4 per vertex in LDS (clip x, y, w and the packed texcoord); a covered sample sets up
// the ORIGINAL triangle from them as the attribute pass does (fragalpha.h), samples the albedo texture through texmath.h's `textureSampler`
// (8 taps) and is dropped, before any load or atomic on the targets, when albedo.a < 0.5.  Alpha is evaluated for EVERY covered sample of an
// alpha-tested slot, so the kept and dropped counts do not depend on the order of the GPU's work.  smallLimit picks the path of every slot's
// triangles, alpha-tested or not: a lane that walks its own small triangle issues its own taps.
// The kernel takes the set's residency as a type (RasterSetArgs<SET>::Set, texmath.h) and asks it for the slot's descriptor check and for the
// sample: this file instantiates it over the decoded set, rasterdepth_blocks.hip over the block-resident one.
#include "rasterdepth.h"

namespace nv
{

int launch_rasterdepth_alpha(hipStream_t stream, const RasterAlphaArgs& a, uint32_t gridBlocks, bool nearClip, bool stableIds)
{
	return launch_rasterdepth_as<true>(stream, a, gridBlocks, nearClip, stableIds);
}

} // namespace nv
