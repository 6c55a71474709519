// drawmirror.h — one entry of the cull mirror of the draws (nv_upload_draws / nv_update_draws / nv_animate_draws): the world-space sphere —
// drawcull.comp.glsl:73-75 up to the view transform, in the reference's operation order — and {scale, meshIndex}.  drawcull.hip's
// draw_split_kernel and animate.hip's kernel run this text, so an entry is the same bits whichever of them wrote it.
#pragma once

#include "cullmath.h"

namespace nv
{

struct DrawMirrorEntry
{
	float4 world;    // the world-space sphere
	uint2 scaleMesh; // {scale bits, meshIndex}
};

// d0 = {position, scale}, d1 = orientation, meshIndex = the draw's word 8; meshCount = the registered table's size, or 0
NV_DEV DrawMirrorEntry draw_mirror_entry(float4 d0, float4 d1, uint32_t meshIndex, const NvMesh* meshes, uint32_t meshCount)
{
	// A draw the passes always skip (postPass mismatch, never visible) may carry any meshIndex: the decide kernel never reads
	// its Mesh, so the mirror must not either.  With a registered table the index is clamped — the entry of such a
	// draw is never used; a valid index is untouched.
	const uint32_t mi = meshCount && meshIndex >= meshCount ? 0u : meshIndex;
	const float4 cr = *reinterpret_cast<const float4*>(meshes + mi); // center.xyz, radius
	const f3 r = rotate_quat(f3{ cr.x, cr.y, cr.z }, f3{ d1.x, d1.y, d1.z }, d1.w);
	// the same three statements as sphere_center() (cullmath.h) before view_point()
	return DrawMirrorEntry{ make_float4(r.x * d0.w + d0.x, r.y * d0.w + d0.y, r.z * d0.w + d0.z, cr.w * d0.w), make_uint2(__float_as_uint(d0.w), meshIndex) };
}

} // namespace nv
