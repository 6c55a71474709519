// bloommath.h — VK_FORMAT_B10G11R11_UFLOAT_PACK32 decode and store and the bilinear footprint of DESIGN.md §4.15, as the bloom kernels
// (bloom.hip) and the BLOOM instantiations of shade_final_kernel (shade.hip) use them.  Integer arithmetic on the float's bits throughout:
// the result does not depend on a denormal mode or a rounding mode.  The header stands alone (no HIP include) so that
// tests/test_bloom_cpu.py can compile it for the host and compare it with tests/bloom_ref.c over every code and a sweep of floats.
#ifndef NV_BLOOMMATH_H
#define NV_BLOOMMATH_H

#include <stdint.h>

#ifndef NV_DEV
#define NV_DEV static inline
#endif

namespace nv
{

// passes 1 and 2 (bloom.hip): a workgroup owns BL_TILE x BL_TILE texels of the level it writes and stages the source texels they can sample
constexpr int BL_TILE = 16;
// pass 1: staged texels per axis.  The tile's coordinates span 15 + 2 (the taps at -1 and +1) output steps of at most 2 + 1 / 16 source texels:
// at most ceil(35.07) + 2 = 38 columns between the first i0 and the last i1; a level narrower than a tile reads at most 2 * 15 + 1 = 31
constexpr int BL_DOWN_SIDE = 40;
// pass 2 up to BL_UP_STAGED_RADIUS: 15 + 2 * 4 output steps of at most half a source texel, at most ceil(11.5) + 2 = 14 columns
constexpr int BL_UP_SIDE = 16;
constexpr float BL_UP_STAGED_RADIUS = 4.0f;
// the fused tail: the texels of all levels it holds, three fp32 planes in one workgroup's 64 KB of static LDS (63 KB)
constexpr int BL_TAIL_TEXELS = 5376;
// (tests/test_bloom_cpu.py walks every tile of every level width with these functions and checks both bounds)

NV_DEV float bl_from_bits(uint32_t b) { return __builtin_bit_cast(float, b); }
NV_DEV uint32_t bl_to_bits(float f) { return __builtin_bit_cast(uint32_t, f); }

// one unsigned small float, MBITS of mantissa (6: R and G, 5: B), 5 bits of exponent with bias 15.  Exact: denormals decode to their values
// (code * 2^(-14 - MBITS), an integer below 2^MBITS times a power of two), exponent 31 is +inf with a zero mantissa and NaN otherwise
template <int MBITS>
NV_DEV float bl_decode(uint32_t code)
{
	const uint32_t e = code >> MBITS, m = code & ((1u << MBITS) - 1u);
	if (e == 0u)
		return (float)m * bl_from_bits((uint32_t)(127 - 14 - MBITS) << 23);
	if (e == 31u)
		return bl_from_bits(m ? 0x7fc00000u : 0x7f800000u);
	return bl_from_bits((e + (127u - 15u)) << 23 | m << (23 - MBITS));
}

// the store (§4.15, D3D's rule): NaN -> exponent 31 with the top mantissa bit; anything else with the sign bit -> 0 (-0 and -inf too);
// +inf -> inf; a finite value above the largest finite code -> that code; everything else rounds toward zero, below the smallest denormal to 0
template <int MBITS>
NV_DEV uint32_t bl_encode(float f)
{
	const uint32_t b = bl_to_bits(f);
	if ((b & 0x7fffffffu) > 0x7f800000u)
		return 31u << MBITS | 1u << (MBITS - 1);
	if (b >> 31)
		return 0u;
	if (b == 0x7f800000u)
		return 31u << MBITS;
	if (b >= 0x47800000u) // 65536 and above: past every finite code
		return (31u << MBITS) - 1u;
	if (b >= 0x38800000u) // 2^-14 and above: rebias the exponent, drop the low mantissa bits
		return (b - ((127u - 15u) << 23)) >> (23 - MBITS);
	// below 2^-14: floor(f * 2^(14 + MBITS)) from the 24-bit significand (an fp32 denormal is far below the smallest code)
	const uint32_t e = b >> 23;
	if (e < 127u - 14u - (uint32_t)MBITS - 1u)
		return 0u;
	return ((b & 0x7fffffu) | 0x800000u) >> ((23 - MBITS) + (127 - 14) - (int)e);
}

NV_DEV uint32_t bl_pack(float r, float g, float b) { return bl_encode<6>(r) | bl_encode<6>(g) << 11 | bl_encode<5>(b) << 22; }

// texture() with filterSampler along one axis (§4.15): u = uv * size - 0.5, i0 = floor(u), alpha = u - i0, i1 = i0 + 1, both clamped to
// [0, size - 1] as floats before the conversion (an overflowed uv clamps like any other)
struct BlAxis
{
	int i0, i1;
	float alpha;
};

NV_DEV BlAxis bl_axis(float uv, float size)
{
	const float u = uv * size - 0.5f;
	const float f0 = __builtin_floorf(u), f1 = f0 + 1.0f, top = size - 1.0f;
	BlAxis a;
	a.alpha = u - f0;
	a.i0 = (int)(f0 < 0.0f ? 0.0f : f0 > top ? top : f0);
	a.i1 = (int)(f1 < 0.0f ? 0.0f : f1 > top ? top : f1);
	return a;
}

// the coordinate of one tap along one axis: uv + step * o with uv = (x + 0.5) / size (bloom.comp.glsl:26); step is texelSize in passes 0 and 1 and
// texelSize * radius in pass 2.  o == 0 gives uv itself (step is finite and positive or zero)
NV_DEV float bl_coord(uint32_t x, float size, float step, float o) { return ((float)x + 0.5f) / size + step * o; }

// (t00 (1 - a) + t10 a) (1 - b) + (t01 (1 - a) + t11 a) b, in that order; a weight of exactly 0 still multiplies
NV_DEV float bl_lerp2(float t00, float t10, float t01, float t11, float a, float b)
{
	return (t00 * (1.0f - a) + t10 * a) * (1.0f - b) + (t01 * (1.0f - a) + t11 * a) * b;
}

} // namespace nv

#endif
