// visattr_indexed.hip — nv_visibility_attributes_indexed: the attribute pass over nv_visibility_resolve_indexed's records.
//
// A record names a triangle of the classic path: {drawId, indexPosition, vertexOffset}.  Its three corners are
// vertices[indices[indexPosition + k] + vertexOffset] (mod 2^32: mesh.vert.glsl:41-62 reads gl_VertexIndex), and from the three fetched
// vertices on the pass IS nv_visibility_attributes: visattr.h's kernel, instantiated on VisAttrIndexedArgs, with its run detection (the
// kernel compares the first three words of neighbouring records: here the draw, the index position and the vertex offset), its corner,
// barycentric and fragment statements and its totals in one copy.  Only the set-up differs: visattr_indexed.h's overload of va_setup, the
// one the kernel's call resolves to for these arguments (shared with the textured forms, visattr_indexed_tex.hip).
#include "visattr_indexed.h"

namespace nv
{

// visattr.h's kernel finds the overload by argument-dependent lookup where it is instantiated (below).  Were it not found, the call
// would bind to the meshlet set-up through the conversion to VisAttrArgs and every record would be invalid: refuse to compile instead.
__device__ void va_setup_dispatch_check(const VisAttrIndexedArgs& a, uint4 r, VaSetup& s)
{
	static_assert(__is_same(decltype(va_setup(a, r, s)), VaIndexedSetup), "the indexed records must reach the indexed va_setup");
}

int launch_visibility_attributes_indexed(hipStream_t stream, VisAttrIndexedArgs a, uint32_t height, uint32_t maxBlocks)
{
	const uint32_t grid = va_complete(a, height, maxBlocks);
	hipLaunchKernelGGL((visibility_attributes_kernel<true, false, VisAttrIndexedArgs>), dim3(grid), dim3(VA_THREADS), 0, stream, a);
	return (int)hipGetLastError();
}

} // namespace nv
