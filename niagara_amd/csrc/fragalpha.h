// fragalpha.h — what the fragment's albedo.a needs (mesh.frag.glsl:62-64, :88), in ONE text for its two users: the attribute pass (visattr.h,
// DESIGN.md §4.13, §4.18) and the alpha-tested depth raster (rasterdepth.h with ALPHA, §4.20).  A corner as clip x, y, w plus its packed
// texcoord, the homogeneous barycentrics with their degenerate rule, uv's steps to the two neighbouring pixel centres and the alpha of a
// material.  Both stages feed it rd_clip_position's bits, so the same triangle at the same pixel gives the same alpha.  The texture itself is
// read through the set's residency type (texmath.h; args.h TxTable::desc is the guarded look-up).
#pragma once
#include "cullmath.h"
#include "args.h"
#define NV_TX_SAMPLER_ONLY // (a block translation unit has included texmath.h in full ahead of this; the others keep the BC tables out of their code objects)
#include "texmath.h"

namespace nv
{

// one corner of the triangle after the vertex stage, as far as uv needs it
struct FaCorner
{
	float cx, cy, cw; // clip x, y, w
	uint32_t uv;      // tu | tv << 16, fp16 bits (the conversion is exact: done after the hand-over)
};

NV_DEV float va_mix(float l0, float l1, float l2, float a0, float a1, float a2) { return (l0 * a0 + l1 * a1) + l2 * a2; }
NV_DEV bool va_finite(float x) { return __builtin_fabsf(x) < __builtin_inff(); }

// homogeneous barycentrics of the triangle (a, b, c) at the point (fx, fy) in pixels (row 0 at the top); returns §4.13's `degen`
NV_DEV bool fa_bary(const FaCorner& a, const FaCorner& b, const FaCorner& c, float fx, float fy, float fw, float fh, float& l0, float& l1, float& l2)
{
	const float nx = (fx / fw) * 2.0f - 1.0f, ny = 1.0f - (fy / fh) * 2.0f;
	const float d0x = a.cx - nx * a.cw, d0y = a.cy - ny * a.cw;
	const float d1x = b.cx - nx * b.cw, d1y = b.cy - ny * b.cw;
	const float d2x = c.cx - nx * c.cw, d2y = c.cy - ny * c.cw;
	const float b0 = d1x * d2y - d1y * d2x, b1 = d2x * d0y - d2y * d0x, b2 = d0x * d1y - d0y * d1x;
	const float sum = (b0 + b1) + b2;
	l0 = b0 / sum, l1 = b1 / sum, l2 = b2 / sum;
	const bool degen = sum == 0.0f || !va_finite(l0) || !va_finite(l1) || !va_finite(l2);
	l0 = degen ? 1.0f : l0, l1 = degen ? 0.0f : l1, l2 = degen ? 0.0f : l2;
	return degen;
}

// uv's steps per pixel (§4.18): the same triangle at the centres of (px + 1, py) and (px, py + 1) minus the pixel's own (u, v); a degenerate
// neighbour contributes zero.  fx, fy: the pixel's own centre.  Nothing is loaded.
NV_DEV void fa_uv_steps(const FaCorner& a, const FaCorner& b, const FaCorner& c, uint32_t px, uint32_t py, float fx, float fy, float fw, float fh, float u, float v,
                        float& dudx, float& dvdx, float& dudy, float& dvdy)
{
	const float ua = half_bits_to_float(a.uv & 0xffffu), ub = half_bits_to_float(b.uv & 0xffffu), uc = half_bits_to_float(c.uv & 0xffffu);
	const float va = half_bits_to_float(a.uv >> 16), vb = half_bits_to_float(b.uv >> 16), vc = half_bits_to_float(c.uv >> 16);
	float m0, m1, m2;
	const bool degenX = fa_bary(a, b, c, (float)(px + 1u) + 0.5f, fy, fw, fh, m0, m1, m2);
	dudx = degenX ? 0.0f : va_mix(m0, m1, m2, ua, ub, uc) - u, dvdx = degenX ? 0.0f : va_mix(m0, m1, m2, va, vb, vc) - v;
	const bool degenY = fa_bary(a, b, c, fx, (float)(py + 1u) + 0.5f, fw, fh, m0, m1, m2);
	dudy = degenY ? 0.0f : va_mix(m0, m1, m2, ua, ub, uc) - u, dvdy = degenY ? 0.0f : va_mix(m0, m1, m2, va, vb, vc) - v;
}

// albedo.a (:62-64): diffuseFactor.a, times the albedo texel's .a where the texture is sampled (fromsrgb leaves .a as it is)
NV_DEV float fa_alpha(float factorA, float texelA) { return factorA * texelA; }

// the discard test of a POST fragment (:88); a NaN alpha keeps the fragment, as the shader's comparison does
NV_DEV bool fa_discard(float alpha) { return alpha < 0.5f; }

} // namespace nv
