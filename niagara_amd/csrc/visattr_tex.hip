// visattr_tex.hip — nv_visibility_attributes_textured: the attribute pass with the complete fragment stage.
//
// The pass is visattr.h's kernel — run detection, set-up, barycentrics and varyings of §4.13, shared with nv_visibility_attributes, not
// copied — instantiated with TEX: per pixel the triangle's barycentrics are taken twice more, at the centres of (px + 1, py) and (px, py + 1),
// from the run's set-up that is already in registers; uv there minus the pixel's own uv are the derivatives the level of detail needs (a
// visibility buffer has no quads).  Then up to four textures are sampled through texmath.h's software `textureSampler` (REPEAT, trilinear:
// 8 taps each), one texture after the other so that only one texture's taps are live at a time, and enter mesh.frag.glsl:62-80.  Before any
// texel load the index is checked against the table and the descriptor's whole chain against the texel buffer.  One launch, no scratch
// memory, only enqueued work.
// The kernel takes the set's residency as a type (VisAttrSetArgs<SET>::Set, texmath.h): this file instantiates it over the decoded set,
// visattr_blocks.hip over the block-resident one.
#include "visattr.h"

namespace nv
{

int launch_visibility_attributes_textured(hipStream_t stream, VisAttrTexArgs a, uint32_t height, uint32_t maxBlocks)
{
	return launch_visibility_attributes_set(stream, a, height, maxBlocks);
}

} // namespace nv
