// bloom.hip — the bloom passes for gfx950: nv_bloom_extract (bloom.comp.glsl pass 0), nv_bloom_downsample (pass 1, QUALITY 1)
// and nv_bloom_upsample (pass 2, QUALITY 1); nv_bloom chains them as src/niagara.cpp:1873-1901 does.
//
// The bloom target is one linear buffer of B10G11R11_UFLOAT_PACK32 words, the levels concatenated, row 0 at the top.  The rule set is §4.15's:
// exact decode, a store that rounds toward zero (bloommath.h), texture() as a bilinear blend with fp32 weights and clamp to edge, one IEEE
// operation per shader operation in the shader's order (-ffp-contract=off); pow and exp2 in pass 0 are the two functions that are not single
// operations.  The clamp keeps every sample inside the level it reads; a thread outside the level it writes stores nothing.
// tests/bloom_ref.c restates the passes one texel at a time; passes 1 and 2 are additions and multiplications only and match it bit for bit.
//
// None of the kernels waits on another workgroup, nothing is allocated: the entry points only enqueue and can be captured.
#include "cullmath.h"
#include "bloommath.h"
#include "launch.h"

namespace nv
{

constexpr int BL_THREADS = 256;

struct BlTexel
{
	float r, g, b;
};

NV_DEV BlTexel bl_unpack(uint32_t word) { return BlTexel{ bl_decode<6>(word & 2047u), bl_decode<6>(word >> 11 & 2047u), bl_decode<5>(word >> 22) }; }

// one texture() of a decoded image, weighted and added: result += texture(...).rgb * weight, per channel (bloom.comp.glsl:54-66,85-93)
template <class Fetch>
NV_DEV void bl_tap(const Fetch& fetch, BlAxis ax, BlAxis ay, float weight, float& r, float& g, float& b)
{
	const BlTexel t00 = fetch(ax.i0, ay.i0), t10 = fetch(ax.i1, ay.i0), t01 = fetch(ax.i0, ay.i1), t11 = fetch(ax.i1, ay.i1);
	r = r + bl_lerp2(t00.r, t10.r, t01.r, t11.r, ax.alpha, ay.alpha) * weight;
	g = g + bl_lerp2(t00.g, t10.g, t01.g, t11.g, ax.alpha, ay.alpha) * weight;
	b = b + bl_lerp2(t00.b, t10.b, t01.b, t11.b, ax.alpha, ay.alpha) * weight;
}

// ---------------------------------------------------------------------------------------------------------------- pass 0

// one sample of gbuffer0 (filtered on the stored codes) through fromsrgb and the emissive decode, bloom.comp.glsl:33,38
NV_DEV f3 bl_emissive(const uint32_t* __restrict__ g0, uint32_t srcW, float fW, float fH, float u, float v)
{
	const BlAxis ax = bl_axis(u, fW), ay = bl_axis(v, fH);
	const uint32_t row0 = (uint32_t)ay.i0 * srcW, row1 = (uint32_t)ay.i1 * srcW;
	const uint32_t w00 = g0[row0 + (uint32_t)ax.i0], w10 = g0[row0 + (uint32_t)ax.i1], w01 = g0[row1 + (uint32_t)ax.i0], w11 = g0[row1 + (uint32_t)ax.i1];
	const float sr = bl_lerp2((float)(w00 & 255u) / 255.0f, (float)(w10 & 255u) / 255.0f, (float)(w01 & 255u) / 255.0f, (float)(w11 & 255u) / 255.0f, ax.alpha, ay.alpha);
	const float sg = bl_lerp2((float)(w00 >> 8 & 255u) / 255.0f, (float)(w10 >> 8 & 255u) / 255.0f, (float)(w01 >> 8 & 255u) / 255.0f,
	                          (float)(w11 >> 8 & 255u) / 255.0f, ax.alpha, ay.alpha);
	const float sb = bl_lerp2((float)(w00 >> 16 & 255u) / 255.0f, (float)(w10 >> 16 & 255u) / 255.0f, (float)(w01 >> 16 & 255u) / 255.0f,
	                          (float)(w11 >> 16 & 255u) / 255.0f, ax.alpha, ay.alpha);
	const float sa = bl_lerp2((float)(w00 >> 24) / 255.0f, (float)(w10 >> 24) / 255.0f, (float)(w01 >> 24) / 255.0f, (float)(w11 >> 24) / 255.0f, ax.alpha, ay.alpha);
	const float e = __builtin_exp2f(sa * 5.0f) - 1.0f;
	return f3{ __builtin_powf(sr, 2.2f) * e, __builtin_powf(sg, 2.2f) * e, __builtin_powf(sb, 2.2f) * e };
}

// bloom.comp.glsl:29-46.  One lane per level-0 texel of a persistent grid: 16 loads of gbuffer0 (the four footprints of an even-sized image
// are the four source texels under the output, each fetched with weight 1 up to the rounding of the coordinate; the rule decides), one store.
__global__ __launch_bounds__(BL_THREADS) void bloom_extract_kernel(const uint32_t* __restrict__ g0, uint32_t* __restrict__ out, uint32_t srcW, uint32_t srcH,
                                                                    uint32_t w, uint32_t h, uint32_t n)
{
	const uint32_t stride = gridDim.x * BL_THREADS;
	const float fw = (float)w, fh = (float)h, fW = (float)srcW, fH = (float)srcH;
	const float tx = 1.0f / fw, ty = 1.0f / fh; // :27
	for (uint32_t i = blockIdx.x * BL_THREADS + threadIdx.x; i < n; i += stride)
	{
		const uint32_t y = i / w, x = i - y * w;
		const float uvx = ((float)x + 0.5f) / fw, uvy = ((float)y + 0.5f) / fh; // :26
		const float xm = uvx + tx * -0.25f, xp = uvx + tx * 0.25f, ym = uvy + ty * -0.25f, yp = uvy + ty * 0.25f;
		const f3 e0 = bl_emissive(g0, srcW, fW, fH, xm, ym); // :33-41
		const f3 e1 = bl_emissive(g0, srcW, fW, fH, xp, ym);
		const f3 e2 = bl_emissive(g0, srcW, fW, fH, xm, yp);
		const f3 e3 = bl_emissive(g0, srcW, fW, fH, xp, yp);
		// :43
		out[i] = bl_pack((((e0.x + e1.x) + e2.x) + e3.x) * 0.25f, (((e0.y + e1.y) + e2.y) + e3.y) * 0.25f, (((e0.z + e1.z) + e2.z) + e3.z) * 0.25f);
	}
}

// ---------------------------------------------------------------------------------------------------------------- passes 1 and 2

// The source texels a tile of outputs can sample, decoded once into three fp32 planes of SIDE x SIDE.  (x0, y0) is the first texel: the i0 of
// the leftmost tap of the tile's first output.  Every coordinate is fl(fl((x + 0.5) / w) + fl(step * o)), non-decreasing in x and in o, and
// floor and the clamp keep the order: no tap of the tile lies left of or above it, and bloommath.h's constants bound how far right and down
// the last one lies.  Texels past the level's edge are never sampled (the clamp) and are staged as zeros without a load.
template <int SIDE>
NV_DEV void bl_stage(float* s_r, float* s_g, float* s_b, const uint32_t* src, int x0, int y0, uint32_t W, uint32_t H)
{
	for (int k = (int)threadIdx.x; k < SIDE * SIDE; k += BL_THREADS)
	{
		const int sy = k / SIDE, sx = k - sy * SIDE;
		const uint32_t x = (uint32_t)(x0 + sx), y = (uint32_t)(y0 + sy);
		const bool in = x < W && y < H;
		const BlTexel t = bl_unpack(in ? src[y * W + x] : 0u);
		s_r[k] = t.r, s_g[k] = t.g, s_b[k] = t.b;
	}
}

// bloom.comp.glsl:50-76 for the texel (x, y) of a w x h level from its W x H source, whatever `fetch` reads the decoded source from: the word
// to store.  The 13 taps use five coordinates per axis (offsets -1, -0.5, 0, +0.5, +1 texels of dst): ten footprints, computed once
template <class Fetch>
NV_DEV uint32_t bl_down_texel(const Fetch& fetch, uint32_t x, uint32_t y, float fw, float fh, float fW, float fH)
{
	const float tx = 1.0f / fw, ty = 1.0f / fh; // :27
	const BlAxis xa = bl_axis(bl_coord(x, fw, tx, -1.0f), fW), xb = bl_axis(bl_coord(x, fw, tx, -0.5f), fW), xc = bl_axis(bl_coord(x, fw, tx, 0.0f), fW),
	             xd = bl_axis(bl_coord(x, fw, tx, 0.5f), fW), xe = bl_axis(bl_coord(x, fw, tx, 1.0f), fW);
	const BlAxis ya = bl_axis(bl_coord(y, fh, ty, -1.0f), fH), yb = bl_axis(bl_coord(y, fh, ty, -0.5f), fH), yc = bl_axis(bl_coord(y, fh, ty, 0.0f), fH),
	             yd = bl_axis(bl_coord(y, fh, ty, 0.5f), fH), ye = bl_axis(bl_coord(y, fh, ty, 1.0f), fH);
	float r = 0.0f, g = 0.0f, b = 0.0f; // :50
	bl_tap(fetch, xc, yc, 0.125f, r, g, b);        // :54
	bl_tap(fetch, xd, yd, 0.5f / 4.0f, r, g, b);   // :55-58
	bl_tap(fetch, xd, yb, 0.5f / 4.0f, r, g, b);
	bl_tap(fetch, xb, yd, 0.5f / 4.0f, r, g, b);
	bl_tap(fetch, xb, yb, 0.5f / 4.0f, r, g, b);
	bl_tap(fetch, xe, ye, 0.125f / 4.0f, r, g, b); // :59-62
	bl_tap(fetch, xe, ya, 0.125f / 4.0f, r, g, b);
	bl_tap(fetch, xa, ye, 0.125f / 4.0f, r, g, b);
	bl_tap(fetch, xa, ya, 0.125f / 4.0f, r, g, b);
	bl_tap(fetch, xe, yc, 0.125f / 2.0f, r, g, b); // :63-66
	bl_tap(fetch, xa, yc, 0.125f / 2.0f, r, g, b);
	bl_tap(fetch, xc, ye, 0.125f / 2.0f, r, g, b);
	bl_tap(fetch, xc, ya, 0.125f / 2.0f, r, g, b);
	return bl_pack(r, g, b); // :76
}

// bloom.comp.glsl:81-106 for the texel (x, y) of a w x h level holding `own`, from its W x H source: the word to store.  The offsets are
// texelSize * radius * (-1, 0, +1), evaluated left to right: three footprints per axis
template <class Fetch>
NV_DEV uint32_t bl_up_texel(const Fetch& fetch, BlTexel own, uint32_t x, uint32_t y, float fw, float fh, float fW, float fH, float radius)
{
	const float rx = (1.0f / fw) * radius, ry = (1.0f / fh) * radius; // :27, texelSize * radius
	const BlAxis xm = bl_axis(bl_coord(x, fw, rx, -1.0f), fW), xc = bl_axis(bl_coord(x, fw, rx, 0.0f), fW), xp = bl_axis(bl_coord(x, fw, rx, 1.0f), fW);
	const BlAxis ym = bl_axis(bl_coord(y, fh, ry, -1.0f), fH), yc = bl_axis(bl_coord(y, fh, ry, 0.0f), fH), yp = bl_axis(bl_coord(y, fh, ry, 1.0f), fH);
	float r = own.r, g = own.g, b = own.b;         // :81
	bl_tap(fetch, xc, yc, 4.0f / 16.0f, r, g, b); // :85
	bl_tap(fetch, xp, yc, 2.0f / 16.0f, r, g, b); // :86-89
	bl_tap(fetch, xm, yc, 2.0f / 16.0f, r, g, b);
	bl_tap(fetch, xc, yp, 2.0f / 16.0f, r, g, b);
	bl_tap(fetch, xc, ym, 2.0f / 16.0f, r, g, b);
	bl_tap(fetch, xp, yp, 1.0f / 16.0f, r, g, b); // :90-93
	bl_tap(fetch, xp, ym, 1.0f / 16.0f, r, g, b);
	bl_tap(fetch, xm, yp, 1.0f / 16.0f, r, g, b);
	bl_tap(fetch, xm, ym, 1.0f / 16.0f, r, g, b);
	return bl_pack(r, g, b); // :106
}

// bloom.comp.glsl:47-77 with QUALITY 1.  src is level - 1 (W x H), dst level (w x h), two disjoint ranges of one buffer.  The 13 taps use five
// coordinates per axis (offsets -1, -0.5, 0, +0.5, +1 texels of dst): five footprints per axis, computed once; the blend of every tap is
// the rule's, from LDS, in the shader's order.
__global__ __launch_bounds__(BL_THREADS) void bloom_downsample_kernel(const uint32_t* src, uint32_t* dst, uint32_t W, uint32_t H, uint32_t w, uint32_t h)
{
	__shared__ float s_r[BL_DOWN_SIDE * BL_DOWN_SIDE], s_g[BL_DOWN_SIDE * BL_DOWN_SIDE], s_b[BL_DOWN_SIDE * BL_DOWN_SIDE];
	const float fw = (float)w, fh = (float)h, fW = (float)W, fH = (float)H;
	const float tx = 1.0f / fw, ty = 1.0f / fh; // :27
	const uint32_t tileX = blockIdx.x * BL_TILE, tileY = blockIdx.y * BL_TILE;
	const int x0 = bl_axis(bl_coord(tileX, fw, tx, -1.0f), fW).i0;
	const int y0 = bl_axis(bl_coord(tileY, fh, ty, -1.0f), fH).i0;
	bl_stage<BL_DOWN_SIDE>(s_r, s_g, s_b, src, x0, y0, W, H);
	__syncthreads();

	const uint32_t x = tileX + (threadIdx.x & 15u), y = tileY + (threadIdx.x >> 4);
	if (x >= w || y >= h)
		return;
	const auto fetch = [&](int i, int j) {
		const int k = (j - y0) * BL_DOWN_SIDE + (i - x0);
		return BlTexel{ s_r[k], s_g[k], s_b[k] };
	};
	dst[y * w + x] = bl_down_texel(fetch, x, y, fw, fh, fW, fH);
}

// bloom.comp.glsl:78-107 with QUALITY 1.  src is level + 1 (W x H), dst level (w x h), read and written by its own invocation only.  The offsets
// are texelSize * radius * (-1, 0, +1), evaluated left to right: three footprints per axis.  STAGED (radius <= BL_UP_STAGED_RADIUS, the host's choice, uniform
// per launch): the source tile comes from LDS as in pass 1; otherwise every tap decodes its four texels from global memory (the source is a
// quarter of the destination and stays in cache).  The arithmetic of the two forms is the same statements.
template <bool STAGED>
__global__ __launch_bounds__(BL_THREADS) void bloom_upsample_kernel(const uint32_t* src, uint32_t* dst, uint32_t W, uint32_t H, uint32_t w, uint32_t h, float radius)
{
	constexpr int SIDE = STAGED ? BL_UP_SIDE : 1;
	__shared__ float s_r[SIDE * SIDE], s_g[SIDE * SIDE], s_b[SIDE * SIDE];
	const float fw = (float)w, fh = (float)h, fW = (float)W, fH = (float)H;
	const float rx = (1.0f / fw) * radius, ry = (1.0f / fh) * radius; // :27, texelSize * radius
	const uint32_t tileX = blockIdx.x * BL_TILE, tileY = blockIdx.y * BL_TILE;
	int x0 = 0, y0 = 0;
	if (STAGED)
	{
		x0 = bl_axis(bl_coord(tileX, fw, rx, -1.0f), fW).i0;
		y0 = bl_axis(bl_coord(tileY, fh, ry, -1.0f), fH).i0;
		bl_stage<SIDE>(s_r, s_g, s_b, src, x0, y0, W, H);
		__syncthreads();
	}

	const uint32_t x = tileX + (threadIdx.x & 15u), y = tileY + (threadIdx.x >> 4);
	if (x >= w || y >= h)
		return;
	const auto fetch = [&](int i, int j) {
		if (STAGED)
		{
			const int k = (j - y0) * SIDE + (i - x0);
			return BlTexel{ s_r[k], s_g[k], s_b[k] };
		}
		return bl_unpack(src[(uint32_t)j * W + (uint32_t)i]);
	};
	dst[y * w + x] = bl_up_texel(fetch, bl_unpack(dst[y * w + x]), x, y, fw, fh, fW, fH, radius);
}

// ---------------------------------------------------------------------------------------------------------------- the fused tail

NV_DEV uint32_t bl_level_side(uint32_t side, uint32_t level)
{
	const uint32_t s = side >> level;
	return s ? s : 1u;
}

// The small end of the chain in ONE launch of ONE workgroup (NV_OPT_BLOOM_FUSED_TAIL): levels first .. levels - 1 together hold at most
// BL_TAIL_TEXELS texels and live in LDS as three fp32 planes, the levels one behind the other as in the bloom target.  Level `first` is
// read (pass 1 has written it, or pass 0 when first == 0); then pass 1 into first + 1 .. levels - 1 and pass 2 into levels - 2 .. first,
// each texel by bl_down_texel / bl_up_texel — the statements of the per-level kernels — packed to its word, stored to the bloom target and
// put back into LDS DECODED FROM THAT WORD, which is what the next pass of the per-level chain would read: the same words at every level.
// A barrier separates the passes; within pass 2 a texel is read and written by its own lane only.  No other workgroup exists to wait for.
__global__ __launch_bounds__(BL_THREADS) void bloom_tail_kernel(uint32_t* bloom, uint32_t width0, uint32_t height0, uint32_t first, uint32_t levels,
                                                                 uint32_t firstOffset, float radius)
{
	__shared__ float s_r[BL_TAIL_TEXELS], s_g[BL_TAIL_TEXELS], s_b[BL_TAIL_TEXELS];
	uint32_t W = bl_level_side(width0, first), H = bl_level_side(height0, first);
	uint32_t srcL = 0u, srcG = firstOffset; // where the source level starts in LDS and in the bloom target
	for (uint32_t k = threadIdx.x; k < W * H; k += BL_THREADS)
	{
		const BlTexel t = bl_unpack(bloom[srcG + k]);
		s_r[k] = t.r, s_g[k] = t.g, s_b[k] = t.b;
	}
	__syncthreads();
	for (uint32_t level = first + 1u; level < levels; ++level)
	{
		const uint32_t w = bl_level_side(width0, level), h = bl_level_side(height0, level);
		const uint32_t dstL = srcL + W * H, dstG = srcG + W * H;
		const auto fetch = [&](int i, int j) {
			const uint32_t k = srcL + (uint32_t)j * W + (uint32_t)i;
			return BlTexel{ s_r[k], s_g[k], s_b[k] };
		};
		for (uint32_t k = threadIdx.x; k < w * h; k += BL_THREADS)
		{
			const uint32_t y = k / w, x = k - y * w;
			const uint32_t word = bl_down_texel(fetch, x, y, (float)w, (float)h, (float)W, (float)H);
			bloom[dstG + k] = word;
			const BlTexel t = bl_unpack(word);
			s_r[dstL + k] = t.r, s_g[dstL + k] = t.g, s_b[dstL + k] = t.b;
		}
		__syncthreads();
		srcL = dstL, srcG = dstG, W = w, H = h;
	}
	for (uint32_t level = levels - 1u; level-- > first;)
	{
		const uint32_t w = bl_level_side(width0, level), h = bl_level_side(height0, level);
		const uint32_t dstL = srcL - w * h, dstG = srcG - w * h;
		const auto fetch = [&](int i, int j) {
			const uint32_t k = srcL + (uint32_t)j * W + (uint32_t)i;
			return BlTexel{ s_r[k], s_g[k], s_b[k] };
		};
		for (uint32_t k = threadIdx.x; k < w * h; k += BL_THREADS)
		{
			const uint32_t y = k / w, x = k - y * w;
			const uint32_t word = bl_up_texel(fetch, BlTexel{ s_r[dstL + k], s_g[dstL + k], s_b[dstL + k] }, x, y, (float)w, (float)h, (float)W, (float)H, radius);
			bloom[dstG + k] = word;
			const BlTexel t = bl_unpack(word);
			s_r[dstL + k] = t.r, s_g[dstL + k] = t.g, s_b[dstL + k] = t.b;
		}
		__syncthreads();
		srcL = dstL, srcG = dstG, W = w, H = h;
	}
}

// ---------------------------------------------------------------------------------------------------------------- launches

static uint32_t level_side(uint32_t side, uint32_t level)
{
	const uint32_t s = side >> level;
	return s ? s : 1u;
}

// the first level from which the rest of the chain fits the fused tail's LDS (the last level is at most 64 x 64 = 4096 texels: it always fits, so the answer is below d.levels)
uint32_t bloom_tail_first(const NvBloomDesc& d)
{
	uint32_t first = d.levels, texels = 0;
	while (first > 0u)
	{
		const uint32_t n = level_side(d.width, first - 1u) * level_side(d.height, first - 1u);
		if (texels + n > (uint32_t)BL_TAIL_TEXELS)
			break;
		texels += n, --first;
	}
	return first;
}

int launch_bloom_tail(hipStream_t stream, uint32_t* bloom, const NvBloomDesc& d, uint32_t first, float radius)
{
	hipLaunchKernelGGL(bloom_tail_kernel, dim3(1), dim3(BL_THREADS), 0, stream, bloom, d.width, d.height, first, d.levels, d.levelOffset[first], radius);
	return (int)hipGetLastError();
}

int launch_bloom_extract(hipStream_t stream, const uint32_t* gbuffer0, uint32_t width, uint32_t height, uint32_t* bloom, const NvBloomDesc& d, uint32_t maxBlocks)
{
	const uint32_t n = d.width * d.height;
	hipLaunchKernelGGL(bloom_extract_kernel, dim3(capped_grid(n, BL_THREADS, maxBlocks)), dim3(BL_THREADS), 0, stream, gbuffer0, bloom + d.levelOffset[0], width, height, d.width, d.height, n);
	return (int)hipGetLastError();
}

int launch_bloom_downsample(hipStream_t stream, uint32_t* bloom, const NvBloomDesc& d, uint32_t level)
{
	const uint32_t W = level_side(d.width, level - 1u), H = level_side(d.height, level - 1u), w = level_side(d.width, level), h = level_side(d.height, level);
	hipLaunchKernelGGL(bloom_downsample_kernel, dim3((w + BL_TILE - 1u) / BL_TILE, (h + BL_TILE - 1u) / BL_TILE), dim3(BL_THREADS), 0, stream,
	                   bloom + d.levelOffset[level - 1u], bloom + d.levelOffset[level], W, H, w, h);
	return (int)hipGetLastError();
}

int launch_bloom_upsample(hipStream_t stream, uint32_t* bloom, const NvBloomDesc& d, uint32_t level, float radius)
{
	const uint32_t W = level_side(d.width, level + 1u), H = level_side(d.height, level + 1u), w = level_side(d.width, level), h = level_side(d.height, level);
	const dim3 grid((w + BL_TILE - 1u) / BL_TILE, (h + BL_TILE - 1u) / BL_TILE);
	if (radius <= BL_UP_STAGED_RADIUS)
		hipLaunchKernelGGL(bloom_upsample_kernel<true>, grid, dim3(BL_THREADS), 0, stream, bloom + d.levelOffset[level + 1u], bloom + d.levelOffset[level], W, H, w,
		                   h, radius);
	else
		hipLaunchKernelGGL(bloom_upsample_kernel<false>, grid, dim3(BL_THREADS), 0, stream, bloom + d.levelOffset[level + 1u], bloom + d.levelOffset[level], W, H, w,
		                   h, radius);
	return (int)hipGetLastError();
}

} // namespace nv
