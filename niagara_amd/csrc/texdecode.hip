// texdecode.hip — nv_texture_decode: BC1 / BC2 / BC3 / BC7 blocks in, the RGBA8 mip chain out, every level in one launch.
//
// Shape.  A work item is one ROW of one block: it finds its level by walking the chain's block counts (at most 15 levels, no table), loads
// the block (8 or 16 bytes), decodes the row's four texels through texmath.h — a texel is a pure function of (block, texel), addressed by bit
// position, so nothing is indexed dynamically and nothing lives in scratch memory — and stores them cropped at the level's right and bottom
// edges: a partial block and the 2 x 1 / 1 x 1 tail write nothing past the level's last texel.  The grid covers the rows once (no stride).
// This runs at load time: correctness and no scratch come first, the throughput is recorded (profiles/r17_textures.md), not targeted; a
// block per work item has not been timed against this form.
#include <hip/hip_runtime.h>

#include "../../include/niagara_vis.h"
#include "texmath.h"
#include "launch.h"

namespace nv
{

constexpr uint32_t TD_THREADS = 256;

struct TexDecodeArgs
{
	const uint64_t* __restrict__ blocks;
	uint32_t* __restrict__ texels; // at the texture's level 0
	uint32_t format, width, height, levels;
	uint64_t rows; // 4 * blocks of every level
};

__global__ __launch_bounds__(TD_THREADS) void texture_decode_kernel(TexDecodeArgs a)
{
	const uint64_t i = (uint64_t)blockIdx.x * TD_THREADS + threadIdx.x;
	if (i >= a.rows)
		return;
	// the level of row i: the last one whose first row is <= i
	uint64_t rowBase = 0, blockBase = 0, texelBase = 0, rows = 0, blocks = 0, words = 0;
	uint32_t w = a.width, h = a.height, bw = (w + 3u) / 4u;
	for (uint32_t l = 0; l < a.levels; ++l)
	{
		const uint32_t lw = tx_level_side(a.width, l), lh = tx_level_side(a.height, l), lbw = (lw + 3u) / 4u, lbh = (lh + 3u) / 4u;
		const bool here = rows <= i;
		rowBase = here ? rows : rowBase, blockBase = here ? blocks : blockBase, texelBase = here ? words : texelBase;
		w = here ? lw : w, h = here ? lh : h, bw = here ? lbw : bw;
		rows += (uint64_t)lbw * lbh * 4u, blocks += (uint64_t)lbw * lbh, words += (uint64_t)lw * lh;
	}
	const uint64_t local = i - rowBase;
	const uint32_t block = (uint32_t)(local >> 2), row = (uint32_t)local & 3u;
	const uint32_t by = block / bw, bx = block - by * bw;
	const uint32_t y = by * 4u + row;
	if (y >= h)
		return;
	uint64_t lo, hi = 0;
	if (a.format == TX_BC1)
		lo = a.blocks[blockBase + block];
	else
	{
		const uint64_t* p = a.blocks + (blockBase + block) * 2u;
		lo = p[0], hi = p[1];
	}
	uint32_t* out = a.texels + texelBase + (uint64_t)y * w + bx * 4u;
	const uint32_t n = w - bx * 4u; // texels left in the row: >= 1
	const uint32_t t0 = tx_decode_texel(a.format, lo, hi, row * 4u), t1 = tx_decode_texel(a.format, lo, hi, row * 4u + 1u);
	const uint32_t t2 = tx_decode_texel(a.format, lo, hi, row * 4u + 2u), t3 = tx_decode_texel(a.format, lo, hi, row * 4u + 3u);
	out[0] = t0;
	if (n > 1u)
		out[1] = t1;
	if (n > 2u)
		out[2] = t2;
	if (n > 3u)
		out[3] = t3;
}

int launch_texture_decode(hipStream_t stream, const void* blocks, uint32_t format, uint32_t width, uint32_t height, uint32_t levels, uint32_t* texels)
{
	TexDecodeArgs a;
	a.blocks = static_cast<const uint64_t*>(blocks);
	a.texels = texels;
	a.format = format, a.width = width, a.height = height, a.levels = levels;
	a.rows = 0;
	for (uint32_t l = 0; l < levels; ++l)
		a.rows += (uint64_t)((tx_level_side(width, l) + 3u) / 4u) * ((tx_level_side(height, l) + 3u) / 4u) * 4u;
	const uint64_t grid = (a.rows + TD_THREADS - 1u) / TD_THREADS; // <= 4096 * 4096 * 4 / 3 * 4 / 256 < 2^19
	hipLaunchKernelGGL(texture_decode_kernel, dim3((uint32_t)grid), dim3(TD_THREADS), 0, stream, a);
	return (int)hipGetLastError();
}

} // namespace nv
