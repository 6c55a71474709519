// visattr.hip — nv_visibility_attributes: the attribute pass of the visibility buffer for gfx950.
//
// nv_visibility_resolve names {draw, meshlet, triangle} per pixel; this kernel says what that triangle looks like AT the pixel: the varyings
// niagara's mesh.frag.glsl receives (uv, normal, tangent, wpos, drawId) and the two G-buffer words it writes (texture terms left out).  Per
// pixel: the triangle's three vertices are fetched and taken through the mesh shader's vertex stage (meshlet.mesh.glsl:125-147; the
// position through raster.h's rd_clip_position, so the clip-space bits are the ones the rasteriser saw), homogeneous barycentrics are
// taken at the pixel centre, every varying is interpolated as (l0 a0 + l1 a1) + l2 a2, and the fragment stage (mesh.frag.glsl:57-89) is
// evaluated from the material's factors.  Every fp32 operation is one IEEE operation in a fixed order (-ffp-contract=off): tests/visattr_ref.c
// restates the rule set one pixel at a time and the attribute records and the gbuffer1 words must equal it bit for bit (gbuffer0 goes
// through pow and log2, which are correctly rounded on neither side: within one code).
//
// Shape.  One lane per pixel of a persistent grid stepping by whole waves, the records read once (non-temporal 16-byte loads), the attribute
// record written as four 16-byte stores per lane.  Neighbouring pixels mostly show the same triangle, so everything that depends on the
// triangle only — the validation, the meshlet header, the three index bytes, the three vertex references, the three vertex records, the draw
// and the three vertex transforms — runs once per RUN of equal (meshletIndex, triangle, drawId) in a wave: a lane starts a run when its key
// differs from lane - 1's (three DPP moves, one ballot), the starting lanes do the set-up, and every lane fetches the 44 words of it from
// the start of its run (ds_bpermute).  What is left per pixel is the barycentrics, the interpolation and the fragment stage.  The three
// corners are named members, selected never indexed: nothing lives in scratch memory.  No workgroup waits on another, nothing is
// allocated: the entry point only enqueues and can be captured.
//
// RUNS = false (experiments build, NV_ATTRIBUTES_PER_PIXEL=1) is the kernel without the runs — every pixel sets its own triangle up — kept for
// the measurement that justifies the runs (profiles/r12_visattr.md).
#include "visattr.h"

namespace nv
{

int launch_visibility_attributes(hipStream_t stream, VisAttrArgs a, uint32_t height, uint32_t maxBlocks, bool perPixel)
{
	const uint32_t grid = va_complete(a, height, maxBlocks);
	if (perPixel)
		hipLaunchKernelGGL(visibility_attributes_kernel<false>, dim3(grid), dim3(VA_THREADS), 0, stream, a);
	else
		hipLaunchKernelGGL(visibility_attributes_kernel<true>, dim3(grid), dim3(VA_THREADS), 0, stream, a);
	return (int)hipGetLastError();
}

} // namespace nv
