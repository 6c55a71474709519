// shadowtrace_blocks.hip — nv_shadow_trace_blocks at quality 1 for gfx950: nv_shadow_trace_textured's alpha-tested ray query
// over a block-resident texture set.  The kernel is shadowtrace.h's tile walk and the traversal rtalpha.h's rt_occluded_alpha, the texts
// shadowtrace_alpha.hip runs, instantiated with RtAlphaBlockInputs; what differs is below: the descriptor check and the four alpha taps of
// level 0, each decoded from its block — alpha alone (tx_decode_alpha), a block loaded once per distinct block of the four taps.  The alpha
// codes are the decoded chain's top bytes and the blend is rt_alpha_lod0's, so the mask is nv_shadow_trace_textured's byte for byte.
#include "texmath.h" // in full, ahead of rtalpha.h's sampler-only inclusion: this translation unit decodes
#include "shadowtrace.h"
#include "rtalpha.h"

namespace nv
{

NV_RT TxBlockDesc rt_alpha_none(const RtAlphaBlockInputs&) { return TxBlockDesc{ 0u, 1u, 1u, 1u | TX_BC1 << 8 }; }

// rt_alpha_texture over the block set: the same index checks, then tx_block_desc_ok against units16
NV_RT bool rt_alpha_texture(const RtAlphaBlockInputs& in, uint32_t drawId, TxBlockDesc* desc)
{
	if (drawId >= in.drawCount)
		return false;
	const uint32_t material = in.draws[drawId].materialIndex;
	if (material >= in.materialCount)
		return false;
	const uint32_t tex = in.materials[material].albedoTexture;
	if (tex == 0u || tex >= in.textureCount)
		return false;
	*desc = in.textures[tex];
	return tx_block_desc_ok(*desc, in.units16);
}

// rt_alpha_lod0 with the four taps' alpha decoded from their blocks (level 0 starts at the texture's first byte)
NV_RT float rt_alpha_lod0(const TxBlockSource& src, float u, float v)
{
	uint32_t x0, x1, y0, y1;
	float ax, ay;
	tx_axis(u, src.width, x0, x1, ax);
	tx_axis(v, src.height, y0, y1, ay);
	uint32_t c00, c01, c10, c11;
	src.walk<true>(src.byteBase, src.width, x0, x1, y0, y1, c00, c01, c10, c11);
	const float a00 = (float)(c00 >> 24) / 255.0f, a01 = (float)(c01 >> 24) / 255.0f, a10 = (float)(c10 >> 24) / 255.0f, a11 = (float)(c11 >> 24) / 255.0f;
	return tx_lerp(tx_lerp(a00, a01, ax), tx_lerp(a10, a11, ax), ay);
}

NV_RT float rt_hit_alpha(const RtAlphaBlockInputs& in, const TxBlockDesc& t, const RtHit& hit, uint32_t w0, uint32_t w1, uint32_t w2)
{
	const RtUv at = rt_hit_uv(hit, w0, w1, w2);
	return rt_alpha_lod0(tx_block_source(in.blocks, t), at.u, at.v);
}

struct BlockAlphaQuery
{
	static NV_DEV bool occluded(const ShadowTraceBlockArgs& a, rt3 origin, rt3 dir) { return rt_occluded_alpha(a.scene, a.in, origin, dir, 1e-2f, 1e3f); } // :86-123
};

int launch_shadow_trace_blocks(hipStream_t stream, ShadowTraceBlockArgs a, uint32_t maxBlocks)
{
	const uint32_t grid = shadow_trace_complete(a, maxBlocks);
	hipLaunchKernelGGL((shadow_trace_kernel<BlockAlphaQuery, ShadowTraceBlockArgs>), dim3(grid), dim3(ST_THREADS), 0, stream, a);
	return (int)hipGetLastError();
}

} // namespace nv
