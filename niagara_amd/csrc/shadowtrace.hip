// shadowtrace.hip — nv_shadow_trace for gfx950: shadow.comp.glsl's ray-traced sun shadow mask on the software BVH that
// rtbuild.cpp builds.  gfx950 has no ray accelerator: the ray query of the shader is rtmath.h's rt_occluded, the same text
// nv_rt_scene_trace_host runs on the CPU, and the RESULT is defined without the BVH (tests/shadow_ref.c tests every triangle).
//
// Shape: one lane per invocation, a wave covers an 8 x 8 tile of invocations (the shader's workgroup: the rays of a wave start next to each
// other and are parallel up to the jitter, so they walk the same nodes and their 16-byte node loads hit the same cache lines), four waves per
// workgroup, a persistent grid that strides over the tiles.  Each lane runs the skip-link loops on its own indices: no stack, no LDS, no
// wait on another workgroup.  A lane with a hit leaves the loops; the wave goes on to its next tile when its last lane is done.  QUALITY is a
// template parameter (the reference has two pipelines, src/niagara.cpp:1803), not a per-lane branch.  Nothing is allocated: the entry point
// only enqueues and can be captured.
#include "cullmath.h"
#include "rtmath.h"

namespace nv
{

constexpr int ST_THREADS = 256;
constexpr uint32_t ST_WAVES = ST_THREADS / 64;
constexpr uint32_t ST_TILE = 8; // 8 x 8 invocations per wave (shadow.comp.glsl's local size)

struct ShadowTraceArgs
{
	NvShadowData sd;
	const unsigned char* __restrict__ scene;
	const float* __restrict__ depth;
	uint8_t* __restrict__ shadow;
	uint32_t width, height;
	uint32_t invocationsX; // checkerboard > 0 ? (width + 1) / 2 : width
	uint32_t tilesX, tiles;
};

template <int QUALITY>
__global__ __launch_bounds__(ST_THREADS) void shadow_trace_kernel(ShadowTraceArgs a)
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
		const bool hit = rt_occluded(a.scene, origin, dir, 1e-2f, 1e3f, (uint32_t)QUALITY); // :81
		a.shadow[at] = hit ? (uint8_t)0 : (uint8_t)255;                                       // :158-160
	}
}

int launch_shadow_trace(hipStream_t stream, const NvShadowData& sd, const void* scene, const float* depth, uint8_t* shadow, uint32_t width, uint32_t height,
                        int quality, uint32_t maxBlocks)
{
	ShadowTraceArgs a;
	a.sd = sd;
	a.scene = static_cast<const unsigned char*>(scene);
	a.depth = depth;
	a.shadow = shadow;
	a.width = width;
	a.height = height;
	a.invocationsX = sd.checkerboard > 0 ? (width + 1u) / 2u : width; // src/niagara.cpp:1797
	a.tilesX = (a.invocationsX + ST_TILE - 1u) / ST_TILE;
	a.tiles = a.tilesX * ((height + ST_TILE - 1u) / ST_TILE);
	uint32_t grid = (a.tiles + ST_WAVES - 1u) / ST_WAVES;
	grid = grid < maxBlocks ? grid : maxBlocks;
	if (quality == 0)
		hipLaunchKernelGGL(shadow_trace_kernel<0>, dim3(grid), dim3(ST_THREADS), 0, stream, a);
	else
		hipLaunchKernelGGL(shadow_trace_kernel<1>, dim3(grid), dim3(ST_THREADS), 0, stream, a);
	return (int)hipGetLastError();
}

} // namespace nv
