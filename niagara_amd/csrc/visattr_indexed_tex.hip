// visattr_indexed_tex.hip — nv_visibility_attributes_indexed_textured: the attribute pass over indexed records with the complete fragment
// stage.
//
// Nothing here is new text: the kernel is visattr.h's with TEX (the statements nv_visibility_attributes_textured runs: uv's steps from the
// run's set-up, up to four textures through texmath.h's sampler, the guarded descriptor look-up of TxTable), the set-up is
// visattr_indexed.h's (the statements nv_visibility_attributes_indexed runs), and the argument type VisAttrIndexedSetArgs<SET> is
// VisAttrIndexedArgs plus the set.  This file instantiates the pair over the decoded set, visattr_indexed_blocks.hip over the
// block-resident one.  One launch, no scratch memory, only enqueued work.
#include "visattr_indexed.h"

namespace nv
{

template __device__ void va_indexed_dispatch_check(const VisAttrIndexedTexArgs&, uint4, VaSetup&);

int launch_visibility_attributes_indexed_textured(hipStream_t stream, VisAttrIndexedTexArgs a, uint32_t height, uint32_t maxBlocks)
{
	return launch_visibility_attributes_set(stream, a, height, maxBlocks);
}

} // namespace nv
