// launch.h — what the entry points (context.hip) call in the other translation units, declared ONCE: every nv::launch_*, the scratch sizes
// (*_bytes, *_stride), tlas_plan, rt_pack_blob and bloom_tail_first.  context.hip includes it and so does every file that defines one of them, so
// a definition that drifts from its declaration does not compile (clustercull.hip and drawcull.hip predate the header and are declared here only).
//
// Convention.  A launch with more than a handful of arguments takes ONE args struct of args.h by value: the entry point fills the caller-facing
// fields by name, the launcher completes the fields derived from them (n, fw and fh, invocationsX, tilesX and tiles ...) and chooses the
// instantiation; what follows the struct is the launch shape (the image height where the struct holds only n, the grid or its cap, the kernel
// variant).  Launches with a short list whose arguments cannot be swapped silently keep the list.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/niagara_vis.h"
#include "rttlas.h"

namespace nv
{

// ---- host code (rtbuild.cpp and rttlas.hip; this part compiles as plain C++)
uint64_t tlas_plan(uint64_t staticBytes, uint32_t maxDraws, TlasPlan* plan);
int rt_pack_blob(const RtHeader& src, const RtBlas* table, const RtNode* tlas, uint32_t tlasNodes, const RtInstance* inst, uint32_t instances,
                 const RtNode* blas, const RtF4* tris, float padOrigin, uint32_t drawCount, void* out, uint64_t* bytes);

// grid of a streaming launch: a workgroup per `per` items of `work`, at most maxBlocks of them (the kernels stride over the rest)
inline uint32_t capped_grid(uint32_t work, uint32_t per, uint32_t maxBlocks)
{
	const uint32_t grid = (work + per - 1u) / per;
	return grid < maxBlocks ? grid : maxBlocks;
}

} // namespace nv

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "args.h"
#include "cullform.h"

namespace nv
{

// clustercull.hip
int launch_cluster_mask(hipStream_t, const ClusterArgs&, const CullForm&, uint32_t maskBlocks);
int launch_cluster_scatter(hipStream_t, const ClusterArgs&, uint32_t scatterBlocks, uint32_t waves);
int launch_cluster_hiz(hipStream_t, const ClusterArgs&, bool soa, uint32_t gridBlocks);
int launch_cluster_bits(hipStream_t, const ClusterArgs&, bool soa, uint32_t gridBlocks);
size_t clustercull_mask_bytes();
size_t clustercull_list_bytes();
uint32_t clustercull_list_stride();
int launch_taskcull(hipStream_t, const ClusterArgs&, int late, bool soa, uint32_t gridBlocks);
int launch_probe(hipStream_t, const ClusterArgs&, bool soa, uint32_t gridBlocks);
int launch_soa_split(hipStream_t, const NvMeshlet*, uint32_t count, uint32_t padded, uint2* bounds, uint32_t* cones, uint32_t* poolWords, uint4* blocks);
// drawcull.hip
int launch_drawcull(hipStream_t, const DrawArgs&, int late, int task);
int launch_draw_split(hipStream_t, const NvMeshDraw*, const NvMesh*, uint32_t meshCount, uint32_t first, uint32_t count, float4* world, uint2* scaleMesh, uint32_t* postPass);
size_t drawcull_result_bytes(uint32_t drawCount);
// submit.hip
int launch_tasksubmit(hipStream_t, uint32_t* count4, NvMeshTaskCommand* commands);
int launch_clustersubmit(hipStream_t, uint32_t* cc4, uint32_t* clusterIndices);
int launch_reset_count(hipStream_t, uint32_t* a, uint32_t* b);
int launch_pack_counts(hipStream_t, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint64_t* out3);
int launch_cluster_expand(hipStream_t, const ClusterExpandArgs&, uint32_t gridBlocks);
int launch_totals3(hipStream_t, const unsigned long long* partials, uint32_t blocks, unsigned long long* totals); // (trianglecull.hip's too)
// bounds.hip, depthreduce.hip, trianglecull.hip
int launch_meshlet_bounds(hipStream_t, const NvVertex* vertices, const uint32_t* data, NvMeshlet* meshlets, uint32_t count, float* out8, uint32_t gridBlocks);
int launch_depthreduce(hipStream_t, const float* depth, uint32_t w, uint32_t h, const NvPyramidDesc& pyr);
int launch_trianglecull(hipStream_t, const TriangleArgs& a, uint32_t gridBlocks);
// rasterdepth.hip, rasterindexed.hip
int launch_rasterdepth(hipStream_t, const RasterArgs& a, uint32_t gridBlocks, bool nearClip, bool stableIds);
int launch_rasterdepth_alpha(hipStream_t, const RasterAlphaArgs& a, uint32_t gridBlocks, bool nearClip, bool stableIds);
int launch_rasterdepth_blocks(hipStream_t, const RasterBlockArgs& a, uint32_t gridBlocks, bool nearClip, bool stableIds);
int launch_raster_totals(hipStream_t, const unsigned long long* partials, uint32_t blocks, unsigned long long* totals, uint32_t counters); // (rasterindexed.hip's too)
int launch_rasterindexed(hipStream_t, RasterIndexedArgs a, void* scratch, uint32_t gridBlocks, bool nearClip);
size_t rasterindexed_scratch_bytes(uint32_t drawCount);
// rasterindexed_vis.hip, visresolve_indexed.hip, visattr_indexed.hip (§4.23)
void launch_rasterindexed_prepare(hipStream_t, RasterIndexedArgs& a, void* scratch); // (rasterindexed.hip's count and scan launches)
int launch_rasterindexed_vis(hipStream_t, RasterIndexedVisArgs a, void* scratch, uint32_t gridBlocks, bool nearClip);
int launch_visibility_resolve_indexed(hipStream_t, VisResolveIndexedArgs a, uint32_t maxBlocks);
int launch_visibility_attributes_indexed(hipStream_t, VisAttrIndexedArgs a, uint32_t height, uint32_t maxBlocks);
// rasterindexed_alpha.hip, rasterindexed_blocks.hip, visattr_indexed_tex.hip, visattr_indexed_blocks.hip (§4.24)
int launch_rasterindexed_alpha(hipStream_t, RasterIndexedAlphaArgs a, void* scratch, uint32_t gridBlocks, bool nearClip);
int launch_rasterindexed_blocks(hipStream_t, RasterIndexedBlockArgs a, void* scratch, uint32_t gridBlocks, bool nearClip);
int launch_visibility_attributes_indexed_textured(hipStream_t, VisAttrIndexedTexArgs a, uint32_t height, uint32_t maxBlocks);
int launch_visibility_attributes_indexed_blocks(hipStream_t, VisAttrIndexedBlockArgs a, uint32_t height, uint32_t maxBlocks);
// depthmerge.hip
int launch_depth_merge(hipStream_t, float* dst, const float* const* srcs, uint32_t sources, uint32_t n, uint32_t maxBlocks);
int launch_visibility_merge(hipStream_t, unsigned long long* dst, const unsigned long long* const* srcs, uint32_t sources, uint32_t n, uint32_t maxBlocks);
// visresolve.hip, visattr.hip, visattr_tex.hip, texdecode.hip
int launch_visibility_resolve(hipStream_t, VisResolveArgs a, uint32_t maxBlocks, bool perPixel);
int launch_visibility_attributes(hipStream_t, VisAttrArgs a, uint32_t height, uint32_t maxBlocks, bool perPixel);
int launch_visibility_attributes_textured(hipStream_t, VisAttrTexArgs a, uint32_t height, uint32_t maxBlocks);
int launch_visibility_attributes_blocks(hipStream_t, VisAttrBlockArgs a, uint32_t height, uint32_t maxBlocks);
int launch_texture_decode(hipStream_t, const void* blocks, uint32_t format, uint32_t width, uint32_t height, uint32_t levels, uint32_t* texels);
// shade.hip
int launch_shadow_fill(hipStream_t, uint8_t* shadow, const float* depth, uint32_t width, uint32_t height, int checkerboard, uint32_t maxBlocks);
int launch_shadow_blur(hipStream_t, uint8_t* out, const uint8_t* shadow, const float* depth, uint32_t width, uint32_t height, bool horizontal, float znear);
int launch_shade_final(hipStream_t, ShadeFinalBloomArgs a, uint32_t height, uint32_t maxBlocks); // a.bloom == nullptr: the kernels without the bloom term
// shadowtrace.hip, shadowtrace_alpha.hip, rttlas.hip
int launch_shadow_trace(hipStream_t, ShadowTraceArgs a, int quality, uint32_t maxBlocks);
int launch_shadow_trace_alpha(hipStream_t, ShadowTraceAlphaArgs a, uint32_t maxBlocks);
int launch_shadow_trace_blocks(hipStream_t, ShadowTraceBlockArgs a, uint32_t maxBlocks);
int launch_tlas_build(hipStream_t, void* scene, const TlasPlan& plan, const NvMeshDraw* draws, uint32_t drawCount);
// animate.hip
int launch_animate(hipStream_t, const AnimateArgs& a, bool mirror);
// bloom.hip
int launch_bloom_extract(hipStream_t, const uint32_t* gbuffer0, uint32_t width, uint32_t height, uint32_t* bloom, const NvBloomDesc& desc, uint32_t maxBlocks);
int launch_bloom_downsample(hipStream_t, uint32_t* bloom, const NvBloomDesc& desc, uint32_t level);
int launch_bloom_upsample(hipStream_t, uint32_t* bloom, const NvBloomDesc& desc, uint32_t level, float radius);
uint32_t bloom_tail_first(const NvBloomDesc& desc);
int launch_bloom_tail(hipStream_t, uint32_t* bloom, const NvBloomDesc& desc, uint32_t first, float radius);

} // namespace nv
#endif
