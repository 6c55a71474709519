// visattr_indexed.h — the set-up of the attribute pass over indexed records in ONE text for its entry points:
// visattr_indexed.hip (nv_visibility_attributes_indexed: the fragment stage from the material's factors) and visattr_indexed_tex.hip and
// visattr_indexed_blocks.hip (nv_visibility_attributes_indexed_textured, nv_visibility_attributes_indexed_blocks: the complete fragment stage).
//
// A record names a triangle of the classic path: {drawId, indexPosition, vertexOffset}.  Its three corners are
// vertices[indices[indexPosition + k] + vertexOffset] (mod 2^32: mesh.vert.glsl:41-62 reads gl_VertexIndex), and from the three fetched
// vertices on the pass IS visattr.h's kernel.  Only the set-up below differs: the overload of va_setup the kernel's call resolves to for
// VisAttrIndexedArgs and for every argument type derived from it (the nearer base wins over the meshlet set-up's VisAttrArgs).
#pragma once
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

// visattr.h's kernel finds the overload above by argument-dependent lookup where it is instantiated.  Were it not found — or did the
// conversion of a derived argument type prefer VisAttrArgs — the call would bind to the meshlet set-up and every record would be invalid:
// refuse to compile instead.  Each translation unit that instantiates the kernel over indexed records states this for its ARGS.
template <typename ARGS>
__device__ void va_indexed_dispatch_check(const ARGS& a, uint4 r, VaSetup& s)
{
	static_assert(__is_same(decltype(va_setup(a, r, s)), VaIndexedSetup), "the indexed records must reach the indexed va_setup");
}

} // namespace nv
