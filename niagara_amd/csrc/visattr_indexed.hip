// visattr_indexed.hip — nv_visibility_attributes_indexed: the attribute pass over nv_visibility_resolve_indexed's records.
//
// A record names a triangle of the classic path: {drawId, indexPosition, vertexOffset}.  Its three corners are
// vertices[indices[indexPosition + k] + vertexOffset] (mod 2^32: mesh.vert.glsl:41-62 reads gl_VertexIndex), and from the three fetched
// vertices on the pass IS nv_visibility_attributes: visattr.h's kernel, instantiated on VisAttrIndexedArgs, with its run detection (the
// kernel compares the first three words of neighbouring records: here the draw, the index position and the vertex offset), its corner,
// barycentric and fragment statements and its totals in one copy.  Only the set-up below differs: the overload of va_setup the kernel's
// call resolves to for these arguments.
#include "visattr.h"

namespace nv
{

// The validation and the set-up of the triangle an indexed record names (drawId != ~0).  Every load is behind the check that keeps it
// inside the caller's buffers; s.ok = 0 when a check fails.
struct VaIndexedSetup // (what this overload returns and the meshlet one does not: the static_assert below tells them apart)
{
};
NV_DEV VaIndexedSetup va_setup(const VisAttrIndexedArgs& a, uint4 r, VaSetup& s)
{
	s.ok = 0u;
	if (r.x >= a.drawCount)
		return {};
	if ((unsigned long long)r.y + 2ull >= (unsigned long long)a.indexCapacity)
		return {};
	const uint32_t va = a.indices[r.y] + r.z, vb = a.indices[r.y + 1u] + r.z, vc = a.indices[r.y + 2u] + r.z; // (mod 2^32)
	if (va >= a.vertexCount || vb >= a.vertexCount || vc >= a.vertexCount)
		return {};
	const float4* dp = reinterpret_cast<const float4*>(a.draws + r.x);
	const float4 d0 = dp[0], d1 = dp[1];
	const uint32_t materialIndex = reinterpret_cast<const uint32_t*>(dp + 2)[3];
	if (a.materials && materialIndex >= a.materialCount)
		return {};
	const uint4* vp = reinterpret_cast<const uint4*>(a.vertices);
	const uint4 v0 = vp[va], v1 = vp[vb], v2 = vp[vc];
	s.a = va_vertex(a.globals, v0, d0, d1);
	s.b = va_vertex(a.globals, v1, d0, d1);
	s.c = va_vertex(a.globals, v2, d0, d1);
	s.materialIndex = materialIndex;
	s.ok = 1u;
	return {};
}

// visattr.h's kernel finds the overload above by argument-dependent lookup where it is instantiated (below).  Were it not found, the call
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
