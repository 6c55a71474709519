// shadowtrace_alpha.hip — nv_shadow_trace_textured at quality 1 for gfx950: shadowTraceTransparent of shadow.comp.glsl:86-123,
// the ray query whose candidates are confirmed by the alpha of their albedo texture.  The traversal is rtalpha.h's rt_occluded_alpha, the text
// nv_rt_scene_trace_host_textured_rays runs on the CPU; the RESULT is defined without the BVH (tests/shadow_alpha_ref.c).
//
// Shape: shadowtrace.hip's — one lane per invocation, an 8 x 8 tile per wave, four waves per workgroup, a persistent grid over the tiles; no
// stack, no LDS, nothing allocated.  The lanes of a wave walk the same nodes until the alpha test, where they part: a lane whose candidate is
// transparent goes on while its neighbour has left.  A candidate's four alpha taps are issued together and waited for once (rt_alpha_lod0).
// Quality 0 has no alpha test: the entry point dispatches shadowtrace.hip's kernel.
#include "cullmath.h"
#include "rtalpha.h"

namespace nv
{

constexpr int STA_THREADS = 256;
constexpr uint32_t STA_WAVES = STA_THREADS / 64;
constexpr uint32_t STA_TILE = 8; // 8 x 8 invocations per wave (shadow.comp.glsl's local size)

struct ShadowTraceAlphaArgs
{
	NvShadowData sd;
	RtAlphaInputs in;
	const unsigned char* __restrict__ scene;
	const float* __restrict__ depth;
	uint8_t* __restrict__ shadow;
	uint32_t width, height;
	uint32_t invocationsX; // checkerboard > 0 ? (width + 1) / 2 : width
	uint32_t tilesX, tiles;
};

__global__ __launch_bounds__(STA_THREADS) void shadow_trace_alpha_kernel(ShadowTraceAlphaArgs a)
{
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	const uint32_t stride = gridDim.x * STA_WAVES;
	const uint32_t cb = (uint32_t)a.sd.checkerboard;
	for (uint32_t tile = blockIdx.x * STA_WAVES + wave; tile < a.tiles; tile += stride)
	{
		const uint32_t ty = tile / a.tilesX, tx = tile - ty * a.tilesX;
		const uint32_t gx = tx * STA_TILE + (lane & 7u), gy = ty * STA_TILE + (lane >> 3);
		if (gx >= a.invocationsX || gy >= a.height)
			continue;
		const uint32_t px = a.sd.checkerboard > 0 ? gx * 2u + ((gy ^ cb) & 1u) : gx; // :129-134
		if (px >= a.width) // odd width: the depth fetch is outside, the store would be dropped
			continue;
		const size_t at = (size_t)gy * a.width + px;
		rt3 origin, dir;
		rt_pixel_ray(a.sd.sunDirection, a.sd.sunJitter, a.sd.inverseViewProjection, a.sd.imageSize, px, gy, a.depth[at], &origin, &dir);
		const bool hit = rt_occluded_alpha(a.scene, a.in, origin, dir, 1e-2f, 1e3f); // :81, :86-123
		a.shadow[at] = hit ? (uint8_t)0 : (uint8_t)255;                              // :158-160
	}
}

int launch_shadow_trace_alpha(hipStream_t stream, const NvShadowData& sd, const void* scene, const float* depth, uint8_t* shadow, uint32_t width,
                              uint32_t height, const NvMeshDraw* draws, uint32_t drawCount, const NvMaterial* materials, uint32_t materialCount,
                              const NvTextureDesc* textures, uint32_t textureCount, const uint32_t* texels, unsigned long long texelWords, uint32_t maxBlocks)
{
	ShadowTraceAlphaArgs a;
	a.sd = sd;
	a.in.draws = draws, a.in.materials = materials, a.in.textures = reinterpret_cast<const TxDesc*>(textures), a.in.texels = texels;
	a.in.texelWords = texelWords, a.in.drawCount = drawCount, a.in.materialCount = materialCount, a.in.textureCount = textureCount;
	a.scene = static_cast<const unsigned char*>(scene);
	a.depth = depth;
	a.shadow = shadow;
	a.width = width;
	a.height = height;
	a.invocationsX = sd.checkerboard > 0 ? (width + 1u) / 2u : width; // src/niagara.cpp:1797
	a.tilesX = (a.invocationsX + STA_TILE - 1u) / STA_TILE;
	a.tiles = a.tilesX * ((height + STA_TILE - 1u) / STA_TILE);
	uint32_t grid = (a.tiles + STA_WAVES - 1u) / STA_WAVES;
	grid = grid < maxBlocks ? grid : maxBlocks;
	hipLaunchKernelGGL(shadow_trace_alpha_kernel, dim3(grid), dim3(STA_THREADS), 0, stream, a);
	return (int)hipGetLastError();
}

} // namespace nv
