// shade.hip — the shading end of the frame for gfx950: nv_shadow_fill (shadowfill.comp.glsl), nv_shadow_blur
// (shadowblur.comp.glsl, BLUR 1), nv_shade_final (final.comp.glsl, the bloom term left out) and nv_shade_final_bloom (final.comp.glsl complete:
// the bloom term is §4.15's texture() of level 0 of the bloom target).
//
// Images are linear buffers, row 0 at the top: depth fp32 (reverse-Z, 0 = no sample), gbuffer0 R8G8B8A8 / gbuffer1 A2B10G10R10 as
// nv_visibility_attributes packs them, shadow images u8 (R8_UNORM, row pitch = width), the colour R8G8B8A8 with R in the low byte.
//
// The rule set is §4.14's: every fp32 operation is one IEEE operation in the shader's order (-ffp-contract=off); max(a, b) = a < b ? b : a
// and min(a, b) = b < a ? b : a with the shader's argument order (a NaN in `view` of a sky pixel survives max(dot, 0) and dies in tonemap's
// max(0, c - 0.004)); pow and exp2 are the two functions that are not single operations.  A texel fetched outside the image is 0, a store
// outside it is dropped: every load stays inside the caller's buffers, which need no padding.  tests/shade_ref.c restates the three passes one
// pixel at a time.
//
// None of the kernels waits on another workgroup, nothing is allocated: the entry points only enqueue and can be captured.
#include "cullmath.h"
#include "bloommath.h"
#include "rtmath.h"
#include "launch.h"

namespace nv
{

constexpr int SH_THREADS = 256;

// UNORM store of one 8-bit channel: clamp to [0, 1] with NaN -> 0, scale, round half to even (§4.13)
NV_DEV uint32_t sh_unorm8(float x)
{
	float v = x > 0.0f ? x : 0.0f;
	v = v < 1.0f ? v : 1.0f;
	return (uint32_t)__builtin_rintf(v * 255.0f);
}

// ---------------------------------------------------------------------------------------------------------------- shadow fill

// shadowfill.comp.glsl:17-46, in place.  Invocation (gx, gy) owns the texel x = 2 gx + (~(gy ^ checkerboard) & 1), y = gy: every texel a launch
// writes has the same parity of x + y, and the four neighbours an invocation reads have the other one.  Nothing that is read is written by
// the same launch, so the in-place update has no race and needs no second image.
__global__ __launch_bounds__(SH_THREADS) void shadow_fill_kernel(uint8_t* shadow, const float* __restrict__ depthImage, uint32_t width, uint32_t height,
                                                                  uint32_t halfWidth, uint32_t n, uint32_t checkerboard)
{
	const uint32_t stride = gridDim.x * SH_THREADS;
	for (uint32_t i = blockIdx.x * SH_THREADS + threadIdx.x; i < n; i += stride)
	{
		const uint32_t gy = i / halfWidth, gx = i - gy * halfWidth;
		const uint32_t px = gx * 2u + (~(gy ^ checkerboard) & 1u);
		if (px >= width) // odd width: the store would be dropped
			continue;
		const size_t at = (size_t)gy * width + px;
		const bool l = px > 0u, r = px + 1u < width, u = gy > 0u, d = gy + 1u < height;
		// the address of a neighbour outside the image is the centre's: the load is in range, the value is replaced by 0
		const size_t al = l ? at - 1u : at, ar = r ? at + 1u : at, au = u ? at - width : at, ad = d ? at + width : at;
		const float depth = depthImage[at];
		const float d0 = depthImage[al], d1 = depthImage[ar], d2 = depthImage[au], d3 = depthImage[ad];
		const uint32_t c0 = shadow[al], c1 = shadow[ar], c2 = shadow[au], c3 = shadow[ad];
		const float z0 = l ? d0 : 0.0f, z1 = r ? d1 : 0.0f, z2 = u ? d2 : 0.0f, z3 = d ? d3 : 0.0f;
		const float s0 = l ? (float)c0 / 255.0f : 0.0f, s1 = r ? (float)c1 / 255.0f : 0.0f;
		const float s2 = u ? (float)c2 / 255.0f : 0.0f, s3 = d ? (float)c3 / 255.0f : 0.0f;
		// :41 weights = exp2(-abs(depths / depth - 1) * 20)
		const float w0 = __builtin_exp2f(-__builtin_fabsf(z0 / depth - 1.0f) * 20.0f);
		const float w1 = __builtin_exp2f(-__builtin_fabsf(z1 / depth - 1.0f) * 20.0f);
		const float w2 = __builtin_exp2f(-__builtin_fabsf(z2 / depth - 1.0f) * 20.0f);
		const float w3 = __builtin_exp2f(-__builtin_fabsf(z3 / depth - 1.0f) * 20.0f);
		// :43
		const float num = ((w0 * s0 + w1 * s1) + w2 * s2) + w3 * s3;
		const float den = ((w0 * 1.0f + w1 * 1.0f) + w2 * 1.0f) + w3 * 1.0f;
		shadow[at] = (uint8_t)sh_unorm8(num / (den + 1e-2f));
	}
}

// ---------------------------------------------------------------------------------------------------------------- shadow blur

constexpr int SB_KERNEL = 10; // shadowblur.comp.glsl:36
constexpr int SB_TILE_X = 64; // both forms: a wave reads 64 texels along x
constexpr int SB_TILE_Y_H = 4;  // horizontal: 64 x 4 outputs, (64 + 20) x 4 staged texels
constexpr int SB_TILE_Y_V = 16; // vertical: 64 x 16 outputs, 64 x (16 + 20) staged texels, four outputs per lane

// :48 exp2(-i * i / 50) is integer arithmetic, ((-i) * i) / 50 truncating toward zero: 0 for i <= 7, -1 for 8 and 9, -2 for 10
constexpr float sb_gw(int i) { return i <= 7 ? 1.0f : i <= 9 ? 0.5f : 0.25f; }

// shadowblur.comp.glsl:24-64.  A workgroup stages its tile and the 10-texel aprons along the filter axis in LDS: per staged texel the
// quotient znear / depth (one IEEE division: the bits do not depend on how often it is computed) and the UNORM fetch of the shadow byte; a
// texel outside the image is depth 0 -> +inf (its weight is exp2(-inf) = 0) and shadow 0.  Global loads run along x in both forms; the
// vertical form walks the taps down the rows of LDS (lane = column: no bank conflicts either way).  The tap loops are unrolled over
// compile-time offsets and sb_gw: no indexed array, no scratch.
template <bool HORIZONTAL>
__global__ __launch_bounds__(SH_THREADS) void shadow_blur_kernel(uint8_t* __restrict__ out, const uint8_t* __restrict__ shadowImage,
                                                                  const float* __restrict__ depthImage, uint32_t width, uint32_t height, float znear)
{
	constexpr int TY = HORIZONTAL ? SB_TILE_Y_H : SB_TILE_Y_V;
	constexpr int SW = HORIZONTAL ? SB_TILE_X + 2 * SB_KERNEL : SB_TILE_X; // staged width
	constexpr int SH = HORIZONTAL ? TY : TY + 2 * SB_KERNEL;               // staged height
	__shared__ float s_q[SH * SW]; // znear / depth
	__shared__ float s_s[SH * SW]; // shadow
	const int x0 = (int)blockIdx.x * SB_TILE_X - (HORIZONTAL ? SB_KERNEL : 0);
	const int y0 = (int)blockIdx.y * TY - (HORIZONTAL ? 0 : SB_KERNEL);
	for (int k = (int)threadIdx.x; k < SH * SW; k += SH_THREADS)
	{
		const int sy = k / SW, sx = k - sy * SW;
		const int x = x0 + sx, y = y0 + sy;
		const bool in = x >= 0 && y >= 0 && x < (int)width && y < (int)height;
		const size_t at = in ? (size_t)y * width + (uint32_t)x : 0u;
		const float dz = depthImage[at];
		const uint32_t code = shadowImage[at];
		s_q[k] = znear / (in ? dz : 0.0f);
		s_s[k] = in ? (float)code / 255.0f : 0.0f;
	}
	__syncthreads();

	const int lx = (int)(threadIdx.x & 63u), wy = (int)(threadIdx.x >> 6);
	const uint32_t px = blockIdx.x * SB_TILE_X + (uint32_t)lx;
	constexpr int STEP = HORIZONTAL ? 1 : SW; // LDS distance of one tap
#pragma unroll
	for (int oy = 0; oy < TY; oy += SH_THREADS / 64)
	{
		const int ty = oy + wy;
		const uint32_t py = blockIdx.y * TY + (uint32_t)ty;
		const int c = HORIZONTAL ? ty * SW + lx + SB_KERNEL : (ty + SB_KERNEL) * SW + lx; // the centre texel in LDS
		float shadow = s_s[c], accumw = 1.0f; // :29-30
		const float depth = s_q[c];           // :32
#pragma unroll
		for (int sign = -1; sign <= 1; sign += 2)
		{
			const float dnext = s_q[c + sign * STEP];                                                 // :41
			const float dgrad = __builtin_fabsf(depth - dnext) < 0.1f ? dnext - depth : 0.0f;        // :42
#pragma unroll
			for (int i = 1; i <= SB_KERNEL; ++i)
			{
				const float dv = s_q[c + i * sign * STEP];                                            // :49
				const float dw = __builtin_exp2f(-__builtin_fabsf(dv - (depth + dgrad * (float)i)) * 100.0f); // :50
				const float fw = sb_gw(i) * dw;                                                       // :51
				shadow = shadow + s_s[c + i * sign * STEP] * fw;                                      // :53
				accumw = accumw + fw;                                                                 // :54
			}
		}
		shadow = shadow / accumw; // :58
		if (px < width && py < height)
			out[(size_t)py * width + px] = (uint8_t)sh_unorm8(shadow);
	}
}

// ---------------------------------------------------------------------------------------------------------------- final shade

// the kernel argument by instantiation (args.h): BLOOM = false keeps ShadeFinalArgs, and with it its code
template <bool BLOOM>
struct ShadeFinalArgsOf
{
	typedef ShadeFinalArgs type;
};
template <>
struct ShadeFinalArgsOf<true>
{
	typedef ShadeFinalBloomArgs type;
};

NV_DEV f3 sh_normalize(f3 v)
{
	const float l = __builtin_sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z);
	return f3{ v.x / l, v.y / l, v.z / l };
}

// math.h:91-95 for one component
NV_DEV float sh_tonemap(float c)
{
	const float x = gl_max(0.0f, c - 0.004f);
	return (x * (6.2f * x + 0.5f)) / (x * (6.2f * x + 1.7f) + 0.06f);
}

// final.comp.glsl:37-80.  One lane per pixel of a persistent grid, straight-line: the loads of a pixel are issued together, the shadow load
// exists only in the SHADOW instantiation (shadeData.shadowsEnabled == 1 is uniform per launch), one 4-byte store per pixel.  BLOOM adds
// :76's texture(bloomImage, uv): four packed texels of the half-resolution level 0 (cached: neighbouring pixels share them), blended by §4.15.
template <bool SHADOW, bool BLOOM>
__global__ __launch_bounds__(SH_THREADS) void shade_final_kernel(typename ShadeFinalArgsOf<BLOOM>::type a)
{
	const uint32_t stride = gridDim.x * SH_THREADS;
	const float* m = a.sd.inverseViewProjection;
	const f3 sun = { a.sd.sunDirection[0], a.sd.sunDirection[1], a.sd.sunDirection[2] };
	for (uint32_t i = blockIdx.x * SH_THREADS + threadIdx.x; i < a.n; i += stride)
	{
		const uint32_t g0 = __builtin_nontemporal_load(a.gbuffer0 + i), g1 = __builtin_nontemporal_load(a.gbuffer1 + i);
		const float depth = __builtin_nontemporal_load(a.depth + i);
		const uint32_t sc = SHADOW ? a.shadow[i] : 0u;
		const uint32_t py = i / a.width, px = i - py * a.width;
		// :40
		const float uvx = ((float)px + 0.5f) / a.sd.imageSize[0], uvy = ((float)py + 0.5f) / a.sd.imageSize[1];
		// :42-43 UNORM fetch
		const float g0r = (float)(g0 & 255u) / 255.0f, g0g = (float)(g0 >> 8 & 255u) / 255.0f, g0b = (float)(g0 >> 16 & 255u) / 255.0f;
		const float g0a = (float)(g0 >> 24) / 255.0f;
		const float g1r = (float)(g1 & 1023u) / 1023.0f, g1g = (float)(g1 >> 10 & 1023u) / 1023.0f, g1b = (float)(g1 >> 20 & 1023u) / 1023.0f;
		// :46-47
		const f3 albedo = { __builtin_powf(g0r, 2.2f), __builtin_powf(g0g, 2.2f), __builtin_powf(g0b, 2.2f) };
		const float e = __builtin_exp2f(g0a * 5.0f) - 1.0f;
		const f3 emissive = { albedo.x * e, albedo.y * e, albedo.z * e };
		// :48 decodeOct (math.h:60-67)
		f3 nv = { g1r * 2.0f - 1.0f, g1g * 2.0f - 1.0f, 0.0f };
		nv.z = (1.0f - __builtin_fabsf(nv.x)) - __builtin_fabsf(nv.y);
		const float t = gl_max(-nv.z, 0.0f);
		nv.x = nv.x + (nv.x >= 0.0f ? -t : t);
		nv.y = nv.y + (nv.y >= 0.0f ? -t : t);
		const f3 normal = sh_normalize(nv);
		// :50
		const float ndotl = gl_max(dot3(normal, sun), 0.0f);
		// :52-54
		const float cx = uvx * 2.0f - 1.0f, cy = 1.0f - uvy * 2.0f;
		const rt3 wpos = rt_unproject(m, cx, cy, depth); // (rtmath.h: the shadow trace's ray origin is the same arithmetic)
		// :56-59
		const f3 view = sh_normalize(f3{ a.sd.cameraPosition[0] - wpos.x, a.sd.cameraPosition[1] - wpos.y, a.sd.cameraPosition[2] - wpos.z });
		const f3 halfv = sh_normalize(f3{ view.x + sun.x, view.y + sun.y, view.z + sun.z });
		const float ndoth = gl_max(dot3(normal, halfv), 0.0f);
		const float gloss = g1b;
		// :62 mix(1, 64, gloss) = 1 (1 - gloss) + 64 gloss
		const float specular = __builtin_powf(ndoth, 1.0f * (1.0f - gloss) + 64.0f * gloss) * gloss;
		// :64-66
		const float shadow = SHADOW ? (float)sc / 255.0f : 1.0f;
		// :73-76 (without BLOOM: an all-zero image)
		const float lit = (ndotl * gl_min(shadow + 0.05f, 1.0f)) * 2.5f + 0.07f;
		const float spec = (specular * shadow) * 2.5f;
		float bloomx, bloomy, bloomz;
		if constexpr (BLOOM)
		{
			const BlAxis ax = bl_axis(uvx, (float)a.bloomWidth), ay = bl_axis(uvy, (float)a.bloomHeight);
			const uint32_t row0 = (uint32_t)ay.i0 * a.bloomWidth, row1 = (uint32_t)ay.i1 * a.bloomWidth;
			const uint32_t b00 = a.bloom[row0 + (uint32_t)ax.i0], b10 = a.bloom[row0 + (uint32_t)ax.i1];
			const uint32_t b01 = a.bloom[row1 + (uint32_t)ax.i0], b11 = a.bloom[row1 + (uint32_t)ax.i1];
			bloomx = bl_lerp2(bl_decode<6>(b00 & 2047u), bl_decode<6>(b10 & 2047u), bl_decode<6>(b01 & 2047u), bl_decode<6>(b11 & 2047u), ax.alpha, ay.alpha) * 0.1f;
			bloomy = bl_lerp2(bl_decode<6>(b00 >> 11 & 2047u), bl_decode<6>(b10 >> 11 & 2047u), bl_decode<6>(b01 >> 11 & 2047u), bl_decode<6>(b11 >> 11 & 2047u),
			                  ax.alpha, ay.alpha) * 0.1f;
			bloomz = bl_lerp2(bl_decode<5>(b00 >> 22), bl_decode<5>(b10 >> 22), bl_decode<5>(b01 >> 22), bl_decode<5>(b11 >> 22), ax.alpha, ay.alpha) * 0.1f;
		}
		else
			bloomx = bloomy = bloomz = 0.0f * 0.1f;
		const float ox = ((albedo.x * lit + spec) + emissive.x) + bloomx;
		const float oy = ((albedo.y * lit + spec) + emissive.y) + bloomy;
		const float oz = ((albedo.z * lit + spec) + emissive.z) + bloomz;
		// :78 gradientNoise(vec2(pos)): no half-pixel offset (math.h:99-102)
		const float inner = (float)px * 0.06711056f + (float)py * 0.00583715f;
		const float f0 = inner - __builtin_floorf(inner);
		const float n1 = 52.9829189f * f0;
		const float noise = n1 - __builtin_floorf(n1);
		const float band = (noise * 2.0f - 1.0f) * (0.5f / 255.0f);
		// :79
		a.color[i] = sh_unorm8(sh_tonemap(ox) + band) | sh_unorm8(sh_tonemap(oy) + band) << 8 | sh_unorm8(sh_tonemap(oz) + band) << 16 | 255u << 24;
	}
}

// ---------------------------------------------------------------------------------------------------------------- launches

int launch_shadow_fill(hipStream_t stream, uint8_t* shadow, const float* depth, uint32_t width, uint32_t height, int checkerboard, uint32_t maxBlocks)
{
	const uint32_t halfWidth = (width + 1u) / 2u; // src/niagara.cpp:1797,1833
	const uint32_t n = halfWidth * height;
	hipLaunchKernelGGL(shadow_fill_kernel, dim3(capped_grid(n, SH_THREADS, maxBlocks)), dim3(SH_THREADS), 0, stream, shadow, depth, width, height, halfWidth, n, (uint32_t)checkerboard);
	return (int)hipGetLastError();
}

int launch_shadow_blur(hipStream_t stream, uint8_t* out, const uint8_t* shadow, const float* depth, uint32_t width, uint32_t height, bool horizontal,
                       float znear)
{
	const uint32_t tx = (width + SB_TILE_X - 1u) / SB_TILE_X;
	if (horizontal)
		hipLaunchKernelGGL(shadow_blur_kernel<true>, dim3(tx, (height + SB_TILE_Y_H - 1u) / SB_TILE_Y_H), dim3(SH_THREADS), 0, stream, out, shadow, depth,
		                   width, height, znear);
	else
		hipLaunchKernelGGL(shadow_blur_kernel<false>, dim3(tx, (height + SB_TILE_Y_V - 1u) / SB_TILE_Y_V), dim3(SH_THREADS), 0, stream, out, shadow, depth,
		                   width, height, znear);
	return (int)hipGetLastError();
}

int launch_shade_final(hipStream_t stream, ShadeFinalBloomArgs a, uint32_t height, uint32_t maxBlocks)
{
	a.n = a.width * height;
	const uint32_t grid = capped_grid(a.n, SH_THREADS, maxBlocks);
	if (a.bloom)
	{
		if (a.sd.shadowsEnabled == 1)
			hipLaunchKernelGGL((shade_final_kernel<true, true>), dim3(grid), dim3(SH_THREADS), 0, stream, a);
		else
			hipLaunchKernelGGL((shade_final_kernel<false, true>), dim3(grid), dim3(SH_THREADS), 0, stream, a);
	}
	else if (a.sd.shadowsEnabled == 1)
		hipLaunchKernelGGL((shade_final_kernel<true, false>), dim3(grid), dim3(SH_THREADS), 0, stream, static_cast<const ShadeFinalArgs&>(a));
	else
		hipLaunchKernelGGL((shade_final_kernel<false, false>), dim3(grid), dim3(SH_THREADS), 0, stream, static_cast<const ShadeFinalArgs&>(a));
	return (int)hipGetLastError();
}

} // namespace nv
