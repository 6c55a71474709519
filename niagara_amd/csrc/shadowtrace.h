// shadowtrace.h — the tile walk of the two ray-traced shadow passes as ONE text: shadowtrace.hip instantiates it with
// rtmath.h's rt_occluded (nv_shadow_trace), shadowtrace_alpha.h with rtalpha.h's rt_occluded_alpha over either residency of the texture set
// (shadowtrace_alpha.hip: nv_shadow_trace_textured at quality 1; shadowtrace_blocks.hip: nv_shadow_trace_blocks, §4.21).  They stay separate
// translation units: the opaque trace does not see the alpha test's text.
//
// Shape: one lane per invocation, a wave covers an 8 x 8 tile of invocations (the shader's workgroup: the rays of a wave start next to each
// other and are parallel up to the jitter, so they walk the same nodes and their 16-byte node loads hit the same cache lines), four waves per
// workgroup, a persistent grid that strides over the tiles.  Each lane runs the skip-link loops on its own indices: no stack, no LDS, no
// wait on another workgroup.  A lane with a hit leaves the loops; the wave goes on to its next tile when its last lane is done.  Nothing is
// allocated: the entry points only enqueue and can be captured.
#pragma once
#include "cullmath.h"
#include "rtmath.h"
#include "launch.h"

namespace nv
{

constexpr int ST_THREADS = 256;
constexpr uint32_t ST_WAVES = ST_THREADS / 64;
constexpr uint32_t ST_TILE = 8; // 8 x 8 invocations per wave (shadow.comp.glsl's local size)

// ARGS = ShadowTraceArgs or ShadowTraceSetArgs<SET> (args.h); QUERY::occluded(a, origin, dir) is the ray query of shadow.comp.glsl:81
template <typename QUERY, typename ARGS>
__global__ __launch_bounds__(ST_THREADS) void shadow_trace_kernel(ARGS a)
{
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	const uint32_t stride = gridDim.x * ST_WAVES;
	const uint32_t cb = (uint32_t)a.sd.checkerboard;
	for (uint32_t tile = blockIdx.x * ST_WAVES + wave; tile < a.tiles; tile += stride)
	{
		const uint32_t ty = tile / a.tilesX, tx = tile - ty * a.tilesX;
		const uint32_t gx = tx * ST_TILE + (lane & 7u), gy = ty * ST_TILE + (lane >> 3);
		if (gx >= a.invocationsX || gy >= a.height)
			continue;
		const uint32_t px = a.sd.checkerboard > 0 ? gx * 2u + ((gy ^ cb) & 1u) : gx; // :129-134
		if (px >= a.width) // odd width: the depth fetch is outside, the store would be dropped
			continue;
		const size_t at = (size_t)gy * a.width + px;
		rt3 origin, dir;
		rt_pixel_ray(a.sd.sunDirection, a.sd.sunJitter, a.sd.inverseViewProjection, a.sd.imageSize, px, gy, a.depth[at], &origin, &dir);
		const bool hit = QUERY::occluded(a, origin, dir);
		a.shadow[at] = hit ? (uint8_t)0 : (uint8_t)255; // :158-160
	}
}

// the fields both launchers derive from the image size, and their grid
template <typename ARGS>
inline uint32_t shadow_trace_complete(ARGS& a, uint32_t maxBlocks)
{
	a.invocationsX = a.sd.checkerboard > 0 ? (a.width + 1u) / 2u : a.width; // src/niagara.cpp:1797
	a.tilesX = (a.invocationsX + ST_TILE - 1u) / ST_TILE;
	a.tiles = a.tilesX * ((a.height + ST_TILE - 1u) / ST_TILE);
	return capped_grid(a.tiles, ST_WAVES, maxBlocks);
}

} // namespace nv
