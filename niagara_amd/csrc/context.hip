// context.hip — the extern "C" boundary declared in include/niagara_vis.h: context lifetime, argument checks and packing, kernel launches.
// No torch types, no exceptions across the ABI; every entry point only enqueues on the caller's stream (nv_status and scratch growth are the
// only synchronising calls).
//
// One convention for every pass: the entry point refuses what it can see is wrong BEFORE anything is enqueued, in the vocabulary defined once
// below (misaligned, image_size_ok, ...), fills the caller-facing fields of the launch's args struct (args.h) by name and hands it to the
// launcher declared in launch.h, which completes the derived fields.  Library-owned device memory goes through scratch_alloc / scratch_reset.
#include <hip/hip_runtime.h>

#include <atomic>
#include <new>
#include <algorithm>
#include <vector>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <float.h>

#include "../../include/niagara_vis.h"
#include "cullmath.h"
#include "filtermath.h"
#include "texmath.h" // TxDecoded, TxBlocks: the residencies the texture-set argument structs are instantiated with
#include "launch.h"

struct ProfRecord
{
	int slot;
	hipEvent_t begin, end;
};

// What the upload hooks build from the caller's scene buffers: the SoA mirrors and the Mesh-table registration.  One
// per context by default; nv_share_scene makes several contexts of one device (several streams, several views in
// flight) use ONE instance, so that three contexts do not hold three identical 480 MB mirrors.  Reference-counted.
struct nv_scene
{
	std::atomic<int> refs{ 1 };
	int device = 0;
	// SoA mirror of the meshlet cull bytes
	const NvMeshlet* mirroredFrom = nullptr;
	uint32_t mirroredCount = 0;
	uint2* soaBounds = nullptr;
	uint32_t* soaCones = nullptr;
	uint32_t* poolWords = nullptr; // 2 x u32 (largest |centre component| / |radius| as fp16 bits) + 2 x float {3 Vmax, Rmax}: clustercull.hip pool_bounds_kernel
	uint4* blockBounds = nullptr; // one 16-B record per 64 meshlets of the mirror (soaCapacity / 64): filtermath.h block_record, clustercull.hip block_bounds_kernel
	uint32_t soaCapacity = 0;
	// SoA mirror of the MeshDraw fields a draw decision reads (nv_upload_draws)
	const NvMeshDraw* drawsFrom = nullptr;
	const NvMesh* drawsMeshes = nullptr; // the Mesh table whose centres / radii are folded into the mirror
	uint32_t drawsCount = 0;
	float4* soaWorld = nullptr;
	uint2* soaScaleMesh = nullptr;
	uint32_t* soaPostPass = nullptr;
	uint32_t drawsCapacity = 0;
	// Mesh table registered by nv_upload_meshes (pointer identity + count): lets drawcull stage it in LDS
	const NvMesh* meshesFrom = nullptr;
	uint32_t meshCount = 0;
};

// nv_create value-initialises it: a field without an initialiser starts at zero
struct nv_context
{
	int device;
	int numCUs;
	uint64_t* masks = nullptr; // per-command ballots between the two clustercull launches
	nv::ClusterCounts* tileCounts = nullptr;
	uint4* candList = nullptr; // late pass with HiZ: the commands with survivors (cull kernel -> occlusion stage)
	uint32_t listStride; // room per sub-list (entries)
	uint32_t listSharers = 4, listMinPer = 8; // occlusion stage: blocks per sub-list, listed commands per block at least
	// drawcull: per-draw result bytes between its two launches, and its own per-tile counts
	uint8_t* drawResults = nullptr;
	size_t drawResultsCapacity;
	nv::ClusterCounts* drawTileCounts = nullptr;
	unsigned long long* alphaPartials = nullptr;  // nv_rasterdepth_textured: per-workgroup {dropped, unevaluated} (2 x u64 x grid)
	unsigned long long* totalsPartials = nullptr; // nv_trianglecull / nv_cluster_expand / nv_rasterdepth(_indexed): per-workgroup partial totals (up to 4 x u64 x grid)
	// nv_rasterdepth_indexed: per-command chunk prefixes + the count launch's per-workgroup sums (rasterindexed.hip), sized like drawResults
	void* rasterScratch = nullptr;
	uint32_t rasterScratchDraws;
	nv_scene* scene = nullptr; // mirrors + registrations (shared between contexts by nv_share_scene)
	// launch shape of the cull kernel (workgroups per CU) and the dealing's start-delay compensation in percent; constants
	// in the product, environment-tunable (with the NV_DEBUG_MODE bit mask) only in the NV_EXPERIMENTS build
	uint32_t debugMode;
	uint32_t ccBlocksPerCU = 6;
	uint32_t dealScale = 100;
	uint32_t scatterTilesPerCU = 1;
	uint32_t scatterWaves = 16; // NV_OPT_SCATTER_WAVES: waves per workgroup of the cluster scatter launch (16; 4 / 8)
	uint32_t scatterTilesAbs; // experiments: absolute number of scatter tiles (0 = per CU)
	uint32_t directPercent = 35; // share of commands passing the filter above which the next launch skips the filter pass (measured crossover, config 3A geometry at several densities: ~36 %)
	uint32_t bitsBlocksPerCU = 4; // cluster_bits_kernel: grid (blocks per CU)
	uint32_t taskcullOneLaunch; // experiments: nv_taskcull's early pass as the one-command-per-wave kernel (the round-1 form)
	int forceDirect = -1;   // NV_OPT_CULL_FORM: -1 = by the previous launch's statistic, 0 / 1 = always filter / always direct, 2 = direct and never the bit-expanding early form
	int forceVisFirst = -1; // NV_OPT_DRAW_RECORDS: -1 = by the statistic of the last TASK pass, 0 / 1 = records with / after the visibility words in drawcull's early pass
	int forceTaskList = -1; // NV_OPT_TASK_EMIT: -1 = by the statistic of earlier TASK passes, 0 / 1 = per-draw / list form of drawcull's TASK scatter
	int forceShallow = -1;  // NV_OPT_CULL_RING: -1 = by the previous launch's command count, 0 / 1 = always the 8-deep / the 4-deep ring
	// command count of the previous clustercull launch, written by its kernel into mapped host memory (tuning hint)
	volatile uint32_t* hintHost = nullptr;
	uint32_t* hintDevice = nullptr;
	// the command buffer the last nv_drawcull(task) of this context wrote: a cluster pass over it runs on the commands of draws the draw-level cull
	// already found visible — nothing for the conservative filter to remove — so, while no launch has left a filter statistic yet (a fresh
	// context's first frames: the hint words lag the launches that fill them), such a pass takes the direct / lane forms instead of the filter form
	const void* taskCommandsFrom;
	uint32_t fusedReset;
	uint32_t fusedSubmit;
	uint64_t* countsSink; // nv_set_counts_sink
	// nv_profile_*: event pairs recorded on the launch stream, drained by nv_profile_read
	int profiling;
	std::vector<ProfRecord>* prof = nullptr;
	float* timing = nullptr; // NV_DEBUG_MODE bit 3: 8 x u64 stamps per wave of the last clustercull
	size_t timingWaves; // its room, in waves
	uint32_t variants[NV_VARIANT_SLOTS]; // nv_profile_variants: launches per kernel variant since the last read
	uint32_t rasterSmallLimit = 16; // NV_OPT_RASTER_SMALL_LIMIT
	uint32_t rasterNearClip;   // NV_OPT_RASTER_NEAR_CLIP: 1 = the clipping instantiations of both depth rasterisers
	uint32_t rasterStableIds;  // NV_OPT_RASTER_VISIBILITY_ID: 1 = nv_rasterdepth writes the stable form of the visibility word
	uint32_t bloomFusedTail;   // NV_OPT_BLOOM_FUSED_TAIL: 1 = nv_bloom runs the levels that fit one workgroup's LDS as one launch
	uint32_t resolvePerPixel;  // experiments: nv_visibility_resolve without the per-run de-duplication
	uint32_t attributesPerPixel; // experiments: nv_visibility_attributes without the per-run set-up
	void* rtScene = nullptr;     // nv_rt_scene_upload: the device copy of the validated scene blob nv_shadow_trace walks
	uint64_t rtSceneBytes;       // of the static blob (a dynamic reservation's allocation is rtPlan.bytes)
	uint32_t rtSceneFlags;       // the uploaded blob's header flags (RT_FLAG_*): a rebuild and a re-housing keep them
	nv::TlasPlan rtPlan;         // nv_rt_scene_reserve_dynamic: where the dynamic sections and the rebuild's scratch lie; maxDraws == 0 = static
	// nv_upload_animations: the validated table as nv_animate_draws' kernel loads it (args.h AnimateArgs)
	uint4* animRecords = nullptr;
	float2* animTimes = nullptr;
	float4* animKeyframes = nullptr;
	uint32_t animCapacity, animKeyCapacity; // room, in animations / keyframes
	uint32_t animCount;
	uint32_t animDrawBound, animLightBound; // the counts the indices were validated against
	bool animUploaded;
};

namespace
{

struct DeviceGuard
{
	int prev;
	bool switched;
	explicit DeviceGuard(int dev) : prev(-1), switched(false)
	{
		if (hipGetDevice(&prev) == hipSuccess && prev != dev)
			switched = hipSetDevice(dev) == hipSuccess;
	}
	~DeviceGuard()
	{
		if (switched)
			(void)hipSetDevice(prev);
	}
};

uint32_t round_up(uint32_t v, uint32_t m) { return (v + m - 1) / m * m; }

// ---- what the entry points refuse, said one way
bool misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; } // (NULL is aligned: optional pointers pass)

// every image of the library: n = width * height fits 32 bits with room for the launchers' rounding
bool image_size_ok(uint32_t width, uint32_t height) { return width != 0 && height != 0 && width <= 16384 && height <= 16384; }

// Library-owned device memory goes through these two.  Product: hipMalloc / hipFree.  Experiments build (tests with
// NV_LIBRARY_PATH = libniagara_vis_exp.so, tools/): every block sits between two 4 KiB canary zones (0xC5) that
// nv_debug_check_scratch compares, and starts out as 0xAB bytes instead of whatever the driver hands out — an out-of-range store of a
// kernel into the library's own scratch, or a kernel that reads a scratch word nobody wrote, shows up in ANY process instead of only
// in a long one whose allocations are recycled.
#ifdef NV_EXPERIMENTS
constexpr size_t NV_GUARD_BYTES = 4096;
struct GuardedBlock
{
	char* base;
	size_t bytes; // payload
};
std::vector<GuardedBlock>& guarded_blocks()
{
	static std::vector<GuardedBlock> v;
	return v;
}
std::atomic_flag g_guardLock = ATOMIC_FLAG_INIT;
struct GuardLock
{
	GuardLock() { while (g_guardLock.test_and_set(std::memory_order_acquire)) { } }
	~GuardLock() { g_guardLock.clear(std::memory_order_release); }
};
#endif

template <class T>
hipError_t scratch_alloc(T** out, size_t bytes)
{
#ifdef NV_EXPERIMENTS
	char* base = nullptr;
	const size_t padded = (bytes + 255) / 256 * 256;
	hipError_t e = hipMalloc(&base, padded + 2 * NV_GUARD_BYTES);
	if (e != hipSuccess)
		return e;
	(void)hipMemset(base, 0xC5, NV_GUARD_BYTES);
	(void)hipMemset(base + NV_GUARD_BYTES, 0xAB, padded);
	(void)hipMemset(base + NV_GUARD_BYTES + padded, 0xC5, NV_GUARD_BYTES);
	{
		GuardLock lock;
		guarded_blocks().push_back(GuardedBlock{ base, padded });
	}
	*out = reinterpret_cast<T*>(base + NV_GUARD_BYTES);
	return hipSuccess;
#else
	return hipMalloc(out, bytes);
#endif
}

void scratch_free(void* p)
{
	if (!p)
		return;
#ifdef NV_EXPERIMENTS
	char* base = static_cast<char*>(p) - NV_GUARD_BYTES;
	{
		GuardLock lock;
		std::vector<GuardedBlock>& v = guarded_blocks();
		for (size_t i = 0; i < v.size(); ++i)
			if (v[i].base == base)
			{
				v[i] = v.back();
				v.pop_back();
				break;
			}
	}
	(void)hipFree(base);
#else
	(void)hipFree(p);
#endif
}

// frees a library-owned block and forgets it
template <class T>
void scratch_reset(T*& p)
{
	scratch_free(p);
	p = nullptr;
}

#ifdef NV_EXPERIMENTS
// an environment variable of the experiments build as atoi reads it, parsed once; `unset` when it is not there
uint32_t env_u32(const char* name, uint32_t unset)
{
	const char* v = getenv(name);
	return v ? (uint32_t)atoi(v) : unset;
}
#endif

// profiling: returns an event recorded on `stream` now, or nullptr when profiling is off
hipEvent_t prof_mark(nv_context* ctx, hipStream_t stream)
{
	if (!ctx->profiling)
		return nullptr;
	hipEvent_t e = nullptr;
	if (hipEventCreate(&e) != hipSuccess)
		return nullptr;
	(void)hipEventRecord(e, stream);
	return e;
}

void prof_push(nv_context* ctx, int slot, hipEvent_t b, hipEvent_t e)
{
	if (b && e && ctx->prof)
		ctx->prof->push_back(ProfRecord{ slot, b, e });
}

NvPyramidDesc null_pyramid()
{
	NvPyramidDesc p;
	memset(&p, 0, sizeof(p));
	return p;
}

// Per-draw result bytes between drawcull's two launches.  Sized by nv_create (1 M draws) and nv_reserve only: a pass entry
// point never allocates or synchronises (it would stall the device behind an "asynchronous enqueue" and break a stream
// capture); a pass over more draws than were reserved returns NV_ENOMEM.
int reserve_draw_results(nv_context* ctx, uint32_t drawCount)
{
	const size_t need = nv::drawcull_result_bytes(drawCount);
	if (need <= ctx->drawResultsCapacity)
		return NV_OK;
	hipError_t e = hipDeviceSynchronize(); // a drawcull still in flight on any stream may be reading the old scratch
	if (e != hipSuccess)
		return (int)e;
	scratch_reset(ctx->drawResults);
	ctx->drawResultsCapacity = 0;
	const size_t cap = need < (size_t(1) << 21) ? (size_t(1) << 21) : need;
	if (scratch_alloc(&ctx->drawResults, cap) != hipSuccess)
		return NV_ENOMEM;
	ctx->drawResultsCapacity = cap;
	return NV_OK;
}

// nv_rasterdepth_indexed's scratch: one word per command slot (maxDrawCount) and a fixed part; sized by nv_create and nv_reserve only, like
// the result bytes above
int reserve_raster_scratch(nv_context* ctx, uint32_t drawCount)
{
	if (ctx->rasterScratch && drawCount <= ctx->rasterScratchDraws)
		return NV_OK;
	hipError_t e = hipDeviceSynchronize(); // a raster still in flight on any stream may be reading the old scratch
	if (e != hipSuccess)
		return (int)e;
	scratch_reset(ctx->rasterScratch);
	ctx->rasterScratchDraws = 0;
	const uint32_t cap = drawCount < (1u << 20) ? (1u << 20) : drawCount;
	char* p = nullptr;
	if (scratch_alloc(&p, nv::rasterindexed_scratch_bytes(cap)) != hipSuccess)
		return NV_ENOMEM;
	ctx->rasterScratch = p;
	ctx->rasterScratchDraws = cap;
	return NV_OK;
}

nv_scene* scene_new(int device)
{
	nv_scene* sc = new (std::nothrow) nv_scene();
	if (sc)
		sc->device = device;
	return sc;
}

// the meshlet mirror (nv_upload_meshlets); the pool words are sized once and stay
void scene_drop_meshlet_mirror(nv_scene* sc)
{
	scratch_reset(sc->soaBounds);
	scratch_reset(sc->soaCones);
	scratch_reset(sc->blockBounds);
	sc->soaCapacity = 0;
	sc->mirroredFrom = nullptr;
}

// the draw mirror (nv_upload_draws)
void scene_drop_draw_mirror(nv_scene* sc)
{
	scratch_reset(sc->soaWorld);
	scratch_reset(sc->soaScaleMesh);
	scratch_reset(sc->soaPostPass);
	sc->drawsCapacity = 0;
	sc->drawsFrom = nullptr;
}

// drops one reference; the last one frees the mirrors (the caller has made the owning device current)
void scene_release(nv_scene* sc)
{
	if (!sc || sc->refs.fetch_sub(1) != 1)
		return;
	scene_drop_meshlet_mirror(sc);
	scratch_reset(sc->poolWords);
	scene_drop_draw_mirror(sc);
	delete sc;
}

// Whether [d_draws, d_draws + count) is a sub-range of the registered draw buffer that starts on a record, and at which record (a pass over a
// shard of the draws, an update of some of them).  On byte differences: a pointer between two records is no NvMeshDraw* to subtract.
bool registered_draw_range(const nv_scene* sc, const NvMeshDraw* d_draws, uint32_t count, size_t* offset)
{
	const uintptr_t from = reinterpret_cast<uintptr_t>(sc->drawsFrom), at = reinterpret_cast<uintptr_t>(d_draws);
	if (!sc->drawsFrom || at < from || (at - from) % sizeof(NvMeshDraw) != 0)
		return false;
	*offset = (at - from) / sizeof(NvMeshDraw);
	return *offset + count <= sc->drawsCount;
}

// one scatter workgroup per CU, capped by the per-tile count table
uint32_t scatter_grid(const nv_context* ctx)
{
	uint32_t g = ctx->scatterTilesAbs ? ctx->scatterTilesAbs : (uint32_t)ctx->numCUs * ctx->scatterTilesPerCU;
	return g > nv::CC_MAX_SCATTER_TILES ? nv::CC_MAX_SCATTER_TILES : g;
}

// grid of the streaming kernels: blocksPerCU workgroups of 256 threads per CU (tests/pixel_cases.py trip_items restates it to size the second-trip tests)
uint32_t persistent_grid(const nv_context* ctx, uint32_t blocksPerCU)
{
	return (uint32_t)ctx->numCUs * blocksPerCU;
}

// The cull launch of nv_clustercull / nv_taskcull's early pass, in the form cullform.h choose_cull_form answers for the context, the pass's arguments and the mapped
// hint words (each read once): the form's words into the arguments, the launch, nv_profile_variants' count.  The provenance of the command list is good for ONE
// launch: a later list at the same address — a freed and reused buffer, a caller-built list — is not this context's drawcull output unless another
// nv_drawcull(task) has written there since.
nv::CullForm launch_cull(nv_context* ctx, hipStream_t s, nv::ClusterArgs& a, bool taskPayload, int late, const void* d_commands, int* rc)
{
	nv::CullFormInputs in = {};
	in.taskPayload = taskPayload;
	in.late = late != 0;
	in.clusterOcclusionEnabled = a.cd.clusterOcclusionEnabled;
	in.postPass = a.cd.postPass;
	in.soa = a.soaBounds != nullptr;
	in.filterPositive = a.filterK > 0.0f;
	in.forceDirect = ctx->forceDirect;
	in.forceShallow = ctx->forceShallow;
	in.directPercent = ctx->directPercent;
	in.hints = ctx->hintHost != nullptr;
	for (int i = 0; in.hints && i < 5; ++i)
		in.hint[i] = ctx->hintHost[i];
	in.ownTaskCommands = d_commands == ctx->taskCommandsFrom;
	ctx->taskCommandsFrom = nullptr;
	in.mirroredCount = ctx->scene->mirroredCount;
	in.alwaysDeep = (ctx->debugMode & 65536u) != 0; // bit 16 (experiments)
	in.commandCountOverride = a.commandCountOverride;
	const nv::CullForm form = nv::choose_cull_form(in);
	a.deferHiz = form.deferHiz;
	a.packDirect = form.packDirect;
	a.packBits = form.packBits;
	ctx->variants[form.variant] += 1u;
	*rc = form.lanes ? nv::launch_cluster_bits(s, a, form.soa, persistent_grid(ctx, ctx->bitsBlocksPerCU))
	                 : nv::launch_cluster_mask(s, a, form, persistent_grid(ctx, ctx->ccBlocksPerCU));
	return form;
}

// ---- the argument checks and fills that the entry points of one pass share: every refusal here is made before anything is enqueued

// What the three raster entry points share (the parameters are their first fifteen without the stream, in their order): the refusals all three
// have, then the caller-facing fields of nv_rasterdepth's launch
static int fill_raster_args(nv::RasterArgs& a, nv_context* ctx, const NvGlobals* globals, const NvMeshTaskCommand* d_commands, const NvMeshDraw* d_draws,
                            const NvMeshlet* d_meshlets, const uint32_t* d_meshletData, const NvVertex* d_vertices, const uint32_t* d_clusterIndices,
                            const uint32_t* d_clusterCount4, float* d_depth, uint32_t width, uint32_t height, uint64_t* d_visibility, uint64_t* d_totals4)
{
	if (!ctx || !globals || !d_commands || !d_draws || !d_meshlets || !d_meshletData || !d_vertices || !d_clusterIndices || !d_clusterCount4 ||
	    !d_depth || !image_size_ok(width, height) || globals->screenWidth != (float)width || globals->screenHeight != (float)height)
		return NV_EINVAL;
	a.globals = *globals;
	a.commands = d_commands;
	a.draws = d_draws;
	a.meshlets = d_meshlets;
	a.meshletData = d_meshletData;
	a.vertices = d_vertices;
	a.clusterIndices = d_clusterIndices;
	a.cc4 = d_clusterCount4;
	a.depth = reinterpret_cast<uint32_t*>(d_depth);
	a.visibility = reinterpret_cast<unsigned long long*>(d_visibility);
	a.width = width;
	a.height = height;
	a.smallLimit = ctx->rasterSmallLimit;
	a.totals = reinterpret_cast<unsigned long long*>(d_totals4);
	a.partials = ctx->totalsPartials;
	return NV_OK;
}

// What nv_rasterdepth_textured and nv_rasterdepth_blocks add to fill_raster_args (rasterdepth_alpha.hip): the alignments
// their kernels' loads need, the rules for the material table and the texture set, then the fields of the set.  d_buffer is the set's buffer —
// the decoded texels, bufferMask 3, or the blocks, bufferMask 15 — and `extent` its size (texelWords or units16)
template <typename SET>
static int fill_raster_set_args(nv::RasterSetArgs<SET>& a, nv_context* ctx, const NvGlobals* globals, const NvMeshTaskCommand* d_commands,
                                const NvMeshDraw* d_draws, const NvMeshlet* d_meshlets, const uint32_t* d_meshletData, const NvVertex* d_vertices,
                                const uint32_t* d_clusterIndices, const uint32_t* d_clusterCount4, float* d_depth, uint32_t width, uint32_t height,
                                uint64_t* d_visibility, uint64_t* d_totals4, const NvMaterial* d_materials, uint32_t materialCount, const void* d_textures,
                                uint32_t textureCount, const void* d_buffer, uintptr_t bufferMask, uint64_t extent, uint64_t* d_alphaTotals2)
{
	if (fill_raster_args(a, ctx, globals, d_commands, d_draws, d_meshlets, d_meshletData, d_vertices, d_clusterIndices, d_clusterCount4, d_depth, width, height,
	                     d_visibility, d_totals4) != NV_OK ||
	    misaligned(d_commands, 3u) || misaligned(d_clusterIndices, 3u) || misaligned(d_clusterCount4, 3u) || misaligned(d_depth, 3u) ||
	    misaligned(d_meshlets, 3u) || misaligned(d_meshletData, 3u) || misaligned(d_buffer, bufferMask) || misaligned(d_visibility, 7u) ||
	    misaligned(d_totals4, 7u) || misaligned(d_alphaTotals2, 7u) || misaligned(d_draws, 15u) || misaligned(d_vertices, 15u) ||
	    misaligned(d_materials, 15u) || misaligned(d_textures, 15u) || (d_textures != nullptr) != (d_buffer != nullptr) || (textureCount && !d_textures) ||
	    (d_materials && materialCount == 0))
		return NV_EINVAL;
	if (d_alphaTotals2 && !ctx->alphaPartials)
		return NV_ENOMEM; // (nv_create reserves them: a pass never allocates)
	a.materials = d_materials;
	a.materialCount = d_materials ? materialCount : 0u;
	a.tx.descs = static_cast<const uint4*>(d_textures);
	a.tx.count = d_textures ? textureCount : 0u;
	a.tx.data = static_cast<const typename SET::Unit*>(d_buffer);
	a.tx.extent = d_buffer ? extent : 0u;
	a.alphaTotals = reinterpret_cast<unsigned long long*>(d_alphaTotals2);
	a.alphaPartials = d_alphaTotals2 ? ctx->alphaPartials : nullptr;
	return NV_OK;
}

// The part the three attribute entry points share (the parameters are the entry points' first twenty, in their
// order): the refusals all three have, then the caller-facing fields of the launch.  The plain pass and the textured pair each add their own rule
// for the material table.
static int fill_attribute_args(nv::VisAttrArgs& a, nv_context* ctx, const NvGlobals* globals, const NvVisRecord* d_records, uint32_t width, uint32_t height,
                               const NvMeshDraw* d_draws, uint32_t drawCount, const NvMeshlet* d_meshlets, uint32_t meshletCount, const uint32_t* d_meshletData,
                               uint32_t meshletDataWords, const NvVertex* d_vertices, uint32_t vertexCount, const NvMaterial* d_materials, uint32_t materialCount,
                               NvPixelAttributes* d_attributes, uint32_t* d_gbuffer0, uint32_t* d_gbuffer1, uint64_t* d_totals4)
{
	if (!ctx || !globals || !d_records || !image_size_ok(width, height) || globals->screenWidth != (float)width || globals->screenHeight != (float)height ||
	    (drawCount && !d_draws) || (meshletCount && !d_meshlets) || (meshletDataWords && !d_meshletData) || (vertexCount && !d_vertices) ||
	    misaligned(d_records, 15u) || misaligned(d_attributes, 15u) || misaligned(d_draws, 15u) || misaligned(d_vertices, 15u) || misaligned(d_materials, 15u) ||
	    misaligned(d_totals4, 7u) || misaligned(d_meshlets, 3u) || misaligned(d_meshletData, 3u) || misaligned(d_gbuffer0, 3u) || misaligned(d_gbuffer1, 3u))
		return NV_EINVAL;
	a.globals = *globals;
	a.records = reinterpret_cast<const nv::va_u4*>(d_records);
	a.width = width;
	a.draws = d_draws;
	a.drawCount = drawCount;
	a.meshlets = d_meshlets;
	a.meshletCount = meshletCount;
	a.meshletData = d_meshletData;
	a.dataWords = meshletDataWords;
	a.vertices = d_vertices;
	a.vertexCount = vertexCount;
	a.materials = d_materials;
	a.materialCount = materialCount;
	a.attributes = reinterpret_cast<uint4*>(d_attributes);
	a.gbuffer0 = d_gbuffer0;
	a.gbuffer1 = d_gbuffer1;
	a.totals = reinterpret_cast<unsigned long long*>(d_totals4);
	return NV_OK;
}

// What nv_visibility_attributes_textured and nv_visibility_attributes_blocks add to fill_attribute_args: their rule for the material table, the
// texture set's refusals and fields.  d_buffer, bufferMask and extent as fill_raster_set_args'
template <typename SET>
static int fill_attribute_set_args(nv::VisAttrSetArgs<SET>& a, nv_context* ctx, const NvGlobals* globals, const NvVisRecord* d_records, uint32_t width,
                                   uint32_t height, const NvMeshDraw* d_draws, uint32_t drawCount, const NvMeshlet* d_meshlets, uint32_t meshletCount,
                                   const uint32_t* d_meshletData, uint32_t meshletDataWords, const NvVertex* d_vertices, uint32_t vertexCount,
                                   const NvMaterial* d_materials, uint32_t materialCount, NvPixelAttributes* d_attributes, uint32_t* d_gbuffer0,
                                   uint32_t* d_gbuffer1, uint64_t* d_totals4, const void* d_textures, uint32_t textureCount, const void* d_buffer,
                                   uintptr_t bufferMask, uint64_t extent)
{
	if (fill_attribute_args(a, ctx, globals, d_records, width, height, d_draws, drawCount, d_meshlets, meshletCount, d_meshletData, meshletDataWords, d_vertices,
	                        vertexCount, d_materials, materialCount, d_attributes, d_gbuffer0, d_gbuffer1, d_totals4) != NV_OK ||
	    !d_materials || (textureCount && (!d_textures || !d_buffer)) || misaligned(d_textures, 15u) || misaligned(d_buffer, bufferMask))
		return NV_EINVAL;
	a.tx.descs = static_cast<const uint4*>(d_textures);
	a.tx.count = d_textures ? textureCount : 0u;
	a.tx.data = static_cast<const typename SET::Unit*>(d_buffer);
	a.tx.extent = extent;
	return NV_OK;
}

// the arguments nv_rasterdepth_indexed and nv_rasterdepth_indexed_visibility share, checked (NV_EINVAL / NV_ENOMEM) and filled
static int fill_rasterindexed_args(nv::RasterIndexedArgs& a, nv_context* ctx, const NvGlobals* globals, const NvMeshDrawCommand* d_commands,
                                   const uint32_t* d_count, const NvMeshDraw* d_draws, uint32_t drawCount, const uint32_t* d_indices, uint32_t indexCapacity,
                                   const NvVertex* d_vertices, uint32_t vertexCapacity, float* d_depth, uint32_t width, uint32_t height, uint64_t* d_totals4)
{
	if (!ctx || !globals || !d_commands || !d_count || !d_draws || !d_indices || !d_vertices || !d_depth || !image_size_ok(width, height) ||
	    globals->screenWidth != (float)width || globals->screenHeight != (float)height)
		return NV_EINVAL;
	if (drawCount > ctx->rasterScratchDraws)
		return NV_ENOMEM; // nv_reserve(ctx, maxDraws, ...) first: a pass never allocates
	memset(&a, 0, sizeof(a));
	a.globals = *globals;
	a.commands = d_commands;
	a.count = d_count;
	a.draws = d_draws;
	a.drawCount = drawCount;
	a.indices = d_indices;
	a.indexCapacity = indexCapacity;
	a.vertices = d_vertices;
	a.vertexCapacity = vertexCapacity;
	a.depth = reinterpret_cast<uint32_t*>(d_depth);
	a.width = width;
	a.height = height;
	a.smallLimit = ctx->rasterSmallLimit;
	a.totals = reinterpret_cast<unsigned long long*>(d_totals4);
	a.partials = ctx->totalsPartials;
	return NV_OK;
}

// What nv_rasterdepth_indexed_textured and nv_rasterdepth_indexed_blocks add to fill_rasterindexed_args (rasterindexed_alpha.hip, DESIGN.md
// §4.24): the visibility pair, optional here as a pair, then fill_raster_set_args' alignments and rules for the material table, the texture set
// and the alpha totals.  d_buffer, bufferMask and extent as fill_raster_set_args'
template <typename SET>
static int fill_rasterindexed_set_args(nv::RasterIndexedSetArgs<SET>& a, nv_context* ctx, const NvGlobals* globals, const NvMeshDrawCommand* d_commands,
                                       const uint32_t* d_count, const NvMeshDraw* d_draws, uint32_t drawCount, const uint32_t* d_indices,
                                       uint32_t indexCapacity, const NvVertex* d_vertices, uint32_t vertexCapacity, float* d_depth, uint32_t width,
                                       uint32_t height, uint64_t* d_totals4, const uint64_t* d_triangleOffsets, uint64_t* d_visibility,
                                       const NvMaterial* d_materials, uint32_t materialCount, const void* d_textures, uint32_t textureCount,
                                       const void* d_buffer, uintptr_t bufferMask, uint64_t extent, uint64_t* d_alphaTotals2)
{
	const int rc = fill_rasterindexed_args(a, ctx, globals, d_commands, d_count, d_draws, drawCount, d_indices, indexCapacity, d_vertices, vertexCapacity,
	                                       d_depth, width, height, d_totals4);
	if (rc != NV_OK)
		return rc;
	if ((d_triangleOffsets != nullptr) != (d_visibility != nullptr) || misaligned(d_triangleOffsets, 7u) || misaligned(d_visibility, 7u) ||
	    misaligned(d_commands, 3u) || misaligned(d_count, 3u) || misaligned(d_indices, 3u) || misaligned(d_depth, 3u) || misaligned(d_buffer, bufferMask) ||
	    misaligned(d_totals4, 7u) || misaligned(d_alphaTotals2, 7u) || misaligned(d_draws, 15u) || misaligned(d_vertices, 15u) ||
	    misaligned(d_materials, 15u) || misaligned(d_textures, 15u) || (d_textures != nullptr) != (d_buffer != nullptr) || (textureCount && !d_textures) ||
	    (d_materials && materialCount == 0))
		return NV_EINVAL;
	if (d_alphaTotals2 && !ctx->alphaPartials)
		return NV_ENOMEM; // (nv_create reserves them: a pass never allocates)
	a.triangleOffsets = reinterpret_cast<const unsigned long long*>(d_triangleOffsets);
	a.visibility = reinterpret_cast<unsigned long long*>(d_visibility);
	a.materials = d_materials;
	a.materialCount = d_materials ? materialCount : 0u;
	a.tx.descs = static_cast<const uint4*>(d_textures);
	a.tx.count = d_textures ? textureCount : 0u;
	a.tx.data = static_cast<const typename SET::Unit*>(d_buffer);
	a.tx.extent = d_buffer ? extent : 0u;
	a.alphaTotals = reinterpret_cast<unsigned long long*>(d_alphaTotals2);
	a.alphaPartials = d_alphaTotals2 ? ctx->alphaPartials : nullptr;
	return NV_OK;
}

// The indexed pair (visattr_indexed_tex.hip): nv_visibility_attributes_indexed's refusals and fields, then
// fill_attribute_set_args' rule for the material table and the texture set — the union of the two parents' refusals
template <typename SET>
static int fill_attribute_indexed_set_args(nv::VisAttrIndexedSetArgs<SET>& a, nv_context* ctx, const NvGlobals* globals, const NvVisIndexedRecord* d_records,
                                           uint32_t width, uint32_t height, const NvMeshDraw* d_draws, uint32_t drawCount, const uint32_t* d_indices,
                                           uint32_t indexCapacity, const NvVertex* d_vertices, uint32_t vertexCapacity, const NvMaterial* d_materials,
                                           uint32_t materialCount, NvPixelAttributes* d_attributes, uint32_t* d_gbuffer0, uint32_t* d_gbuffer1,
                                           uint64_t* d_totals4, const void* d_textures, uint32_t textureCount, const void* d_buffer, uintptr_t bufferMask,
                                           uint64_t extent)
{
	if (fill_attribute_args(a, ctx, globals, reinterpret_cast<const NvVisRecord*>(d_records), width, height, d_draws, drawCount, nullptr, 0u, nullptr, 0u,
	                        d_vertices, vertexCapacity, d_materials, materialCount, d_attributes, d_gbuffer0, d_gbuffer1, d_totals4) != NV_OK ||
	    (indexCapacity && !d_indices) || misaligned(d_indices, 3u) || !d_materials || (textureCount && (!d_textures || !d_buffer)) ||
	    misaligned(d_textures, 15u) || misaligned(d_buffer, bufferMask))
		return NV_EINVAL;
	a.indices = d_indices;
	a.indexCapacity = indexCapacity;
	a.tx.descs = static_cast<const uint4*>(d_textures);
	a.tx.count = d_textures ? textureCount : 0u;
	a.tx.data = static_cast<const typename SET::Unit*>(d_buffer);
	a.tx.extent = extent;
	return NV_OK;
}

// what the three trace entry points share: the refusals, then the caller-facing fields of the opaque launch
static int fill_trace_args(nv::ShadowTraceArgs& a, nv_context* ctx, const NvShadowData* shadow, const float* d_depth, uint8_t* d_shadow, uint32_t width,
                           uint32_t height, int quality)
{
	if (!ctx || !ctx->rtScene || !shadow || !d_depth || !d_shadow || !image_size_ok(width, height) || shadow->imageSize[0] != (float)width ||
	    shadow->imageSize[1] != (float)height || quality < 0 || quality > 1 || misaligned(d_depth, 3u))
		return NV_EINVAL;
	a.sd = *shadow;
	a.scene = static_cast<const unsigned char*>(ctx->rtScene);
	a.depth = d_depth;
	a.shadow = d_shadow;
	a.width = width;
	a.height = height;
	return NV_OK;
}

// What nv_shadow_trace_textured and nv_shadow_trace_blocks add to fill_trace_args (shadowtrace_alpha.hip): a scene with
// texcoords, every count with its table, the alignments; then the alpha trace's arguments from the opaque launch's.  d_buffer, bufferMask and
// extent as fill_raster_set_args'
template <typename SET>
static int fill_trace_alpha(nv::ShadowTraceSetArgs<SET>& a, nv::ShadowTraceArgs& opaque, nv_context* ctx, const NvShadowData* shadow, const float* d_depth,
                            uint8_t* d_shadow, uint32_t width, uint32_t height, int quality, const NvMeshDraw* d_draws, uint32_t drawCount,
                            const NvMaterial* d_materials, uint32_t materialCount, const void* d_textures, uint32_t textureCount, const void* d_buffer,
                            uintptr_t bufferMask, uint64_t extent)
{
	if (fill_trace_args(opaque, ctx, shadow, d_depth, d_shadow, width, height, quality) != NV_OK || !(ctx->rtSceneFlags & nv::RT_FLAG_TEXCOORDS) ||
	    (drawCount && !d_draws) || (materialCount && !d_materials) || (textureCount && !d_textures) || (extent && !d_buffer) || misaligned(d_draws, 15u) ||
	    misaligned(d_materials, 15u) || misaligned(d_textures, 15u) || misaligned(d_buffer, bufferMask))
		return NV_EINVAL;
	a.sd = opaque.sd;
	a.in.draws = d_draws;
	a.in.materials = d_materials;
	a.in.textures = static_cast<const typename SET::Desc*>(d_textures);
	a.in.data = static_cast<const typename SET::Unit*>(d_buffer);
	a.in.extent = extent;
	a.in.drawCount = drawCount;
	a.in.materialCount = materialCount;
	a.in.textureCount = textureCount;
	a.scene = opaque.scene;
	a.depth = d_depth;
	a.shadow = d_shadow;
	a.width = width;
	a.height = height;
	return NV_OK;
}

} // namespace

extern "C" {

const char* nv_version(void) { return "niagara_vis 0.4 (gfx950)"; } // 0.2: NV_PROF_SLOTS 4 -> 5; 0.3: nv_reserve, nv_share_scene; 0.4: NV_VARIANT_SLOTS 9 -> 10

int nv_create(nv_context** out_ctx, int device)
{
	if (!out_ctx)
		return NV_EINVAL;
	*out_ctx = nullptr;
	int count = 0;
	if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
		return NV_ENODEV;
	if (device < 0 || device >= count)
		return NV_EINVAL;
	DeviceGuard guard(device);

	nv_context* ctx = new (std::nothrow) nv_context();
	if (!ctx)
		return NV_ENOMEM;
	ctx->device = device;
	ctx->scene = scene_new(device);
	if (!ctx->scene)
	{
		delete ctx;
		return NV_ENOMEM;
	}

	hipDeviceProp_t prop;
	hipError_t e = hipGetDeviceProperties(&prop, device);
	if (e != hipSuccess)
	{
		scene_release(ctx->scene);
		delete ctx;
		return (int)e;
	}
	ctx->numCUs = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
	ctx->listStride = nv::clustercull_list_stride();
#ifdef NV_EXPERIMENTS
	// the experiments build only (tools/): the product library reads no environment variable
	ctx->resolvePerPixel = env_u32("NV_RESOLVE_PER_PIXEL", ctx->resolvePerPixel);
	ctx->attributesPerPixel = env_u32("NV_ATTRIBUTES_PER_PIXEL", ctx->attributesPerPixel);
	ctx->forceDirect = (int)env_u32("NV_DIRECT", (uint32_t)ctx->forceDirect);
	ctx->taskcullOneLaunch = env_u32("NV_TASKCULL_ONE_LAUNCH", ctx->taskcullOneLaunch);
	ctx->bitsBlocksPerCU = env_u32("NV_BITS_BLOCKS", ctx->bitsBlocksPerCU);
	ctx->directPercent = env_u32("NV_DIRECT_PERCENT", ctx->directPercent);
	ctx->scatterTilesPerCU = std::max(env_u32("NV_SCATTER_TILES_PER_CU", 1), 1u);
	ctx->scatterTilesAbs = env_u32("NV_SCATTER_TILES", ctx->scatterTilesAbs);
	ctx->debugMode = env_u32("NV_DEBUG_MODE", ctx->debugMode);
	ctx->listStride = std::min(env_u32("NV_HIZ_LIST_STRIDE", ctx->listStride), ctx->listStride); // a small value forces the occlusion stage's scan fallback (tests)
	if (const uint32_t v = env_u32("NV_HIZ_SHARERS", 0))
		ctx->listSharers = v;
	if (const uint32_t v = env_u32("NV_HIZ_MIN_PER", 0); v >= 4 && v <= 64)
		ctx->listMinPer = v;
	ctx->dealScale = env_u32("NV_DEAL_SCALE", ctx->dealScale);
	if (const uint32_t v = env_u32("NV_CC_BLOCKS_PER_CU", 0))
		ctx->ccBlocksPerCU = std::min(v, 8u); // (the stamp buffer holds 8 per CU)
#endif

	if (scratch_alloc(&ctx->masks, nv::clustercull_mask_bytes()) != hipSuccess || scratch_alloc(&ctx->tileCounts, sizeof(nv::ClusterCounts)) != hipSuccess ||
	    scratch_alloc(&ctx->candList, nv::clustercull_list_bytes()) != hipSuccess ||
	    hipMemset(ctx->tileCounts, 0, sizeof(nv::ClusterCounts)) != hipSuccess ||
	    scratch_alloc(&ctx->drawTileCounts, sizeof(nv::ClusterCounts)) != hipSuccess ||
	    hipMemset(ctx->drawTileCounts, 0, sizeof(nv::ClusterCounts)) != hipSuccess || reserve_draw_results(ctx, 1u << 20) != NV_OK ||
	    reserve_raster_scratch(ctx, 1u << 20) != NV_OK ||
	    scratch_alloc(&ctx->totalsPartials, (size_t)persistent_grid(ctx, 8) * 4 * sizeof(unsigned long long)) != hipSuccess ||
	    scratch_alloc(&ctx->alphaPartials, (size_t)persistent_grid(ctx, 8) * 2 * sizeof(unsigned long long)) != hipSuccess)
	{
		nv_destroy(ctx);
		return NV_ENOMEM;
	}
	// optional: without it the kernels simply keep the deep ring
	{
		void* h = nullptr;
		if (hipHostMalloc(&h, 64, hipHostMallocMapped) == hipSuccess)
		{
			memset(h, 0, 64);
			void* d = nullptr;
			if (hipHostGetDevicePointer(&d, h, 0) == hipSuccess)
			{
				ctx->hintHost = static_cast<volatile uint32_t*>(h);
				ctx->hintDevice = static_cast<uint32_t*>(d);
			}
			else
				(void)hipHostFree(h);
		}
	}

	*out_ctx = ctx;
	return NV_OK;
}

void nv_destroy(nv_context* ctx)
{
	if (!ctx)
		return;
	DeviceGuard guard(ctx->device);
	if (ctx->hintHost)
		(void)hipHostFree(const_cast<uint32_t*>(ctx->hintHost));
	scratch_reset(ctx->drawResults);
	scratch_reset(ctx->drawTileCounts);
	scratch_reset(ctx->totalsPartials);
	scratch_reset(ctx->alphaPartials);
	scratch_reset(ctx->rasterScratch);
	scratch_reset(ctx->masks);
	scratch_reset(ctx->tileCounts);
	scratch_reset(ctx->candList);
	scene_release(ctx->scene);
	scratch_reset(ctx->timing);
	scratch_reset(ctx->rtScene);
	scratch_reset(ctx->animRecords);
	scratch_reset(ctx->animTimes);
	scratch_reset(ctx->animKeyframes);
	delete ctx->prof;
	delete ctx;
}

int nv_status(nv_context* ctx, void* stream)
{
	if (!ctx)
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	hipError_t e = hipStreamSynchronize((hipStream_t)stream);
	if (e != hipSuccess)
		return (int)e;
	return NV_OK;
}

int nv_set_option(nv_context* ctx, int option, int value)
{
	if (!ctx)
		return NV_EINVAL;
	switch (option)
	{
	case NV_OPT_FUSED_COUNT_RESET:
		ctx->fusedReset = value ? 1u : 0u;
		return NV_OK;
	case NV_OPT_FUSED_SUBMIT:
		ctx->fusedSubmit = value ? 1u : 0u;
		return NV_OK;
	case NV_OPT_SCATTER_WAVES:
		if (value != 4 && value != 8 && value != 16)
			return NV_EINVAL;
		ctx->scatterWaves = (uint32_t)value;
		return NV_OK;
	case NV_OPT_CULL_FORM:
		if (value < 0 || value > 5)
			return NV_EINVAL;
		ctx->forceDirect = value - 1; // 0 -> -1 (by statistic), 1 -> 0 (filter form), 2 -> 1 (direct form), 3 -> 2 (direct, one command per wave also with visibility bits), 4 -> 3 (as 3, and no packed walk), 5 -> 4 (direct, the packed walk also in the early pass with visibility bits)
		return NV_OK;
	case NV_OPT_TASK_EMIT:
		if (value < 0 || value > 2)
			return NV_EINVAL;
		ctx->forceTaskList = value - 1;
		return NV_OK;
	case NV_OPT_DRAW_RECORDS:
		if (value < 0 || value > 2)
			return NV_EINVAL;
		ctx->forceVisFirst = value - 1;
		return NV_OK;
	case NV_OPT_CULL_RING:
		if (value != 0 && value != 4 && value != 8)
			return NV_EINVAL;
		ctx->forceShallow = value == 0 ? -1 : (value == 4 ? 1 : 0);
		return NV_OK;
	case NV_OPT_RASTER_SMALL_LIMIT:
		if (value < 0)
			return NV_EINVAL;
		ctx->rasterSmallLimit = (uint32_t)value;
		return NV_OK;
	case NV_OPT_RASTER_NEAR_CLIP:
		if (value != 0 && value != 1)
			return NV_EINVAL;
		ctx->rasterNearClip = (uint32_t)value;
		return NV_OK;
	case NV_OPT_RASTER_VISIBILITY_ID:
		if (value != 0 && value != 1)
			return NV_EINVAL;
		ctx->rasterStableIds = (uint32_t)value;
		return NV_OK;
	case NV_OPT_BLOOM_FUSED_TAIL:
		if (value != 0 && value != 1)
			return NV_EINVAL;
		ctx->bloomFusedTail = (uint32_t)value;
		return NV_OK;
	case NV_OPT_CULL_WORKGROUPS_PER_CU:
		if (value < 1 || value > 8)
			return NV_EINVAL;
		ctx->ccBlocksPerCU = (uint32_t)value;
		return NV_OK;
	default:
		return NV_EINVAL;
	}
}

int nv_reserve(nv_context* ctx, uint32_t maxDraws, uint32_t maxCommands)
{
	if (!ctx)
		return NV_EINVAL;
	(void)maxCommands; // the per-command scratch (ballots, survivor lists) is sized for NV_TASK_WGLIMIT by nv_create: the passes never process more
	DeviceGuard guard(ctx->device);
	const int rc = reserve_draw_results(ctx, maxDraws);
	return rc ? rc : reserve_raster_scratch(ctx, maxDraws);
}

int nv_share_scene(nv_context* dst, nv_context* src)
{
	if (!dst || !src || dst->device != src->device)
		return NV_EINVAL;
	if (dst->scene == src->scene)
		return NV_OK;
	DeviceGuard guard(dst->device);
	// passes of dst still in flight read dst's current mirrors
	hipError_t e = hipDeviceSynchronize();
	if (e != hipSuccess)
		return (int)e;
	src->scene->refs.fetch_add(1);
	scene_release(dst->scene);
	dst->scene = src->scene;
	return NV_OK;
}

int nv_profile_enable(nv_context* ctx, int enabled)
{
	if (!ctx)
		return NV_EINVAL;
	if (!ctx->prof)
		ctx->prof = new (std::nothrow) std::vector<ProfRecord>();
	if (!ctx->prof)
		return NV_ENOMEM;
	ctx->profiling = enabled ? 1 : 0;
	return NV_OK;
}

int nv_profile_read(nv_context* ctx, float out_ms[NV_PROF_SLOTS], uint32_t out_count[NV_PROF_SLOTS])
{
	if (!ctx || !out_ms || !out_count)
		return NV_EINVAL;
	for (int i = 0; i < NV_PROF_SLOTS; ++i)
	{
		out_ms[i] = 0.0f;
		out_count[i] = 0;
	}
	if (!ctx->prof)
		return NV_OK;
	DeviceGuard guard(ctx->device);
	int rc = NV_OK;
	for (ProfRecord& r : *ctx->prof)
	{
		float ms = 0.0f;
		hipError_t e = hipEventSynchronize(r.end);
		if (e == hipSuccess)
			e = hipEventElapsedTime(&ms, r.begin, r.end);
		if (e == hipSuccess && r.slot >= 0 && r.slot < NV_PROF_SLOTS)
		{
			out_ms[r.slot] += ms;
			out_count[r.slot] += 1;
		}
		else if (e != hipSuccess)
			rc = (int)e;
	}
	// events are shared between adjacent records (end of one = begin of the next): destroy each once
	std::vector<hipEvent_t> seen;
	for (ProfRecord& r : *ctx->prof)
		for (hipEvent_t ev : { r.begin, r.end })
		{
			bool dup = false;
			for (hipEvent_t s : seen)
				dup = dup || s == ev;
			if (!dup)
			{
				seen.push_back(ev);
				(void)hipEventDestroy(ev);
			}
		}
	ctx->prof->clear();
	return rc;
}

int nv_profile_variants(nv_context* ctx, uint32_t out_count[NV_VARIANT_SLOTS])
{
	if (!ctx || !out_count)
		return NV_EINVAL;
	for (int i = 0; i < NV_VARIANT_SLOTS; ++i)
	{
		out_count[i] = ctx->variants[i];
		ctx->variants[i] = 0;
	}
	return NV_OK;
}

int nv_upload_meshlets(nv_context* ctx, void* stream, const NvMeshlet* d_meshlets, uint32_t meshletCount)
{
	if (!ctx || (!d_meshlets && meshletCount))
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	// one extra 64-entry block so that a command's 64-lane window never leaves the mirror
	uint32_t padded = round_up(meshletCount, 64) + 64;
	if (padded > ctx->scene->soaCapacity)
	{
		// a pass of this or of a sharing context may still be reading the old mirror on another stream
		hipError_t e = hipDeviceSynchronize();
		if (e != hipSuccess)
			return (int)e;
		scene_drop_meshlet_mirror(ctx->scene);
		if (scratch_alloc(&ctx->scene->soaBounds, (size_t)padded * sizeof(uint2)) != hipSuccess ||
		    scratch_alloc(&ctx->scene->soaCones, (size_t)padded * sizeof(uint32_t)) != hipSuccess ||
		    scratch_alloc(&ctx->scene->blockBounds, (size_t)(padded / 64) * sizeof(uint4)) != hipSuccess)
			return NV_ENOMEM;
		ctx->scene->soaCapacity = padded;
	}
	if (!ctx->scene->poolWords && scratch_alloc(&ctx->scene->poolWords, 4 * sizeof(uint32_t)) != hipSuccess)
	{
		ctx->scene->mirroredFrom = nullptr; // (no pool bounds: no SoA pass may name the old mirror either)
		return NV_ENOMEM;
	}
	int rc = nv::launch_soa_split((hipStream_t)stream, d_meshlets, meshletCount, padded, ctx->scene->soaBounds, ctx->scene->soaCones, ctx->scene->poolWords,
	                              ctx->scene->blockBounds);
	if (rc)
		return rc;
	ctx->scene->mirroredFrom = d_meshlets;
	ctx->scene->mirroredCount = meshletCount;
	return NV_OK;
}

int nv_debug_block_table(nv_context* ctx, void* hostOut, uint32_t maxRecords, uint32_t* out_records)
{
	if (!ctx || !out_records || (!hostOut && maxRecords))
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	const uint32_t n = ctx->scene->mirroredFrom && ctx->scene->blockBounds ? (round_up(ctx->scene->mirroredCount, 64) + 64) / 64 : 0u;
	*out_records = n;
	hipError_t e = hipDeviceSynchronize();
	if (e == hipSuccess && n && maxRecords)
		e = hipMemcpy(hostOut, ctx->scene->blockBounds, (size_t)(n < maxRecords ? n : maxRecords) * sizeof(uint4), hipMemcpyDeviceToHost);
	return (int)e;
}

int nv_upload_meshes(nv_context* ctx, void* stream, const NvMesh* d_meshes, uint32_t meshCount)
{
	(void)stream;
	if (!ctx || (!d_meshes && meshCount))
		return NV_EINVAL;
	ctx->scene->meshesFrom = d_meshes;
	ctx->scene->meshCount = meshCount;
	return NV_OK;
}

int nv_upload_draws(nv_context* ctx, void* stream, const NvMeshDraw* d_draws, uint32_t drawCount, const NvMesh* d_meshes)
{
	if (!ctx || (!d_draws && drawCount) || (d_draws && !d_meshes))
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	if (!d_draws)
	{
		ctx->scene->drawsFrom = nullptr;
		ctx->scene->drawsMeshes = nullptr;
		ctx->scene->drawsCount = 0;
		return NV_OK;
	}
	if (drawCount > ctx->scene->drawsCapacity)
	{
		//  a drawcull of this or of a sharing context may still be reading the old mirror on another stream
		hipError_t e = hipDeviceSynchronize();
		if (e != hipSuccess)
			return (int)e;
		scene_drop_draw_mirror(ctx->scene);
		const size_t cap = (size_t)drawCount + 64;
		if (scratch_alloc(&ctx->scene->soaWorld, cap * sizeof(float4)) != hipSuccess || scratch_alloc(&ctx->scene->soaScaleMesh, cap * sizeof(uint2)) != hipSuccess ||
		    scratch_alloc(&ctx->scene->soaPostPass, cap * sizeof(uint32_t)) != hipSuccess)
			return NV_ENOMEM;
		ctx->scene->drawsCapacity = drawCount;
	}
	int rc = nv::launch_draw_split((hipStream_t)stream, d_draws, d_meshes, ctx->scene->meshesFrom == d_meshes ? ctx->scene->meshCount : 0u, 0, drawCount, ctx->scene->soaWorld, ctx->scene->soaScaleMesh, ctx->scene->soaPostPass);
	if (rc)
		return rc;
	ctx->scene->drawsFrom = d_draws;
	ctx->scene->drawsMeshes = d_meshes;
	ctx->scene->drawsCount = drawCount;
	return NV_OK;
}

int nv_update_draws(nv_context* ctx, void* stream, const NvMeshDraw* d_draws, uint32_t first, uint32_t count)
{
	if (!ctx || !d_draws)
		return NV_EINVAL;
	size_t base = 0;
	if (!registered_draw_range(ctx->scene, d_draws, 1, &base))
		return NV_OK; // nothing registered for this buffer: the passes read it in place anyway
	base += first;
	if (base > ctx->scene->drawsCount || count > ctx->scene->drawsCount - base)
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	return nv::launch_draw_split((hipStream_t)stream, ctx->scene->drawsFrom, ctx->scene->drawsMeshes,
	                             ctx->scene->meshesFrom == ctx->scene->drawsMeshes ? ctx->scene->meshCount : 0u, (uint32_t)base, count, ctx->scene->soaWorld, ctx->scene->soaScaleMesh, ctx->scene->soaPostPass);
}

int nv_drawcull(nv_context* ctx, void* stream, const NvCullData* cull, int late, int task, const NvMeshDraw* d_draws,
                const NvMesh* d_meshes, void* d_commands, uint32_t* d_count4, uint32_t* d_drawVisibility,
                const NvPyramidDesc* pyramid)
{
	if (!ctx || !cull || !d_count4 || !d_drawVisibility || (cull->drawCount && (!d_draws || !d_meshes || !d_commands)))
		return NV_EINVAL;
	if (late && cull->occlusionEnabled == 1 && !(pyramid && pyramid->d_base))
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);

	if (nv::drawcull_result_bytes(cull->drawCount) > ctx->drawResultsCapacity)
		return NV_ENOMEM; // nv_reserve(ctx, maxDraws, ...) first: a pass never allocates
	int rc = NV_OK;

	nv::DrawArgs a;
	a.cd = *cull;
	a.pyr = pyramid ? *pyramid : null_pyramid();
	a.draws = d_draws;
	// the mirror serves the registered buffer and any sub-range of it that starts on a record (a pass over a shard of the draws)
	size_t drawOffset = 0;
	const bool mirrored = ctx->scene->soaWorld && registered_draw_range(ctx->scene, d_draws, cull->drawCount, &drawOffset) &&
	                      ctx->scene->drawsMeshes == d_meshes; // (the mirror folds THAT table's bounds in)
	a.soaWorld = mirrored ? ctx->scene->soaWorld + drawOffset : nullptr;
	a.soaScaleMesh = mirrored ? ctx->scene->soaScaleMesh + drawOffset : nullptr;
	a.soaPostPass = mirrored ? ctx->scene->soaPostPass + drawOffset : nullptr;
	a.meshes = d_meshes;
	a.commands = d_commands;
	a.count4 = d_count4;
	a.dvb = d_drawVisibility;
	a.results = ctx->drawResults;
	a.tileCounts = ctx->drawTileCounts;
	a.scatterTiles = scatter_grid(ctx);
#ifdef NV_EXPERIMENTS
	a.debugMode = ctx->debugMode;
#endif
	a.fusedReset = ctx->fusedReset;
	a.fusedSubmit = ctx->fusedSubmit;
	a.meshCount = ctx->scene->meshesFrom == d_meshes ? ctx->scene->meshCount : 0u;
	a.hostHint = ctx->hintDevice;
	// TASK scatter form: the list form (one lane per output command) when an earlier TASK pass emitted more than 4 commands per
	// emitting draw, the per-draw form otherwise (and until a pass has been seen); NV_OPT_TASK_EMIT pins it
	a.taskList = ctx->forceTaskList >= 0 ? (uint32_t)ctx->forceTaskList : (ctx->hintHost && ctx->hintHost[3] > 4u * ctx->hintHost[2] ? 1u : 0u);
	// early pass: visibility words first, and only the records of last frame's visible draws, when the last TASK pass emitted from fewer than one draw in eight
	a.visFirst = late ? 0u : (ctx->forceVisFirst >= 0 ? (uint32_t)ctx->forceVisFirst : (ctx->hintHost && ctx->hintHost[2] != 0u && (uint64_t)ctx->hintHost[2] * 8u < cull->drawCount ? 1u : 0u));
	if (task)
	{
		ctx->variants[a.taskList ? NV_VARIANT_TASK_LIST : NV_VARIANT_TASK_PER_DRAW] += 1u;
		ctx->taskCommandsFrom = d_commands;
	}
	hipEvent_t e0 = prof_mark(ctx, (hipStream_t)stream);
	rc = nv::launch_drawcull((hipStream_t)stream, a, late, task);
	prof_push(ctx, NV_PROF_DRAWCULL, e0, prof_mark(ctx, (hipStream_t)stream));
	return rc;
}

int nv_reset_count(nv_context* ctx, void* stream, uint32_t* d_count4a, uint32_t* d_count4b)
{
	if (!ctx || (!d_count4a && !d_count4b))
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	return nv::launch_reset_count((hipStream_t)stream, d_count4a, d_count4b);
}

int nv_tasksubmit(nv_context* ctx, void* stream, uint32_t* d_count4, NvMeshTaskCommand* d_commands)
{
	if (!ctx || !d_count4 || !d_commands)
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	return nv::launch_tasksubmit((hipStream_t)stream, d_count4, d_commands);
}

static int fill_cluster_args(nv_context* ctx, nv::ClusterArgs& a, const NvCullData* cull, int late,
                             const NvMeshTaskCommand* d_commands, const uint32_t* d_count4, const NvMeshDraw* d_draws,
                             const NvMeshlet* d_meshlets, uint32_t* d_meshletVisibility, const NvPyramidDesc* pyramid)
{
	if (!ctx || !cull || !d_commands || !d_draws || !d_meshlets)
		return NV_EINVAL;
	if (cull->clusterOcclusionEnabled == 1 && !d_meshletVisibility)
		return NV_EINVAL;
	if (late && cull->clusterOcclusionEnabled == 1 && !(pyramid && pyramid->d_base))
		return NV_EINVAL;
	memset(&a, 0, sizeof(a));
	a.cd = *cull;
	a.pyr = pyramid ? *pyramid : null_pyramid();
	a.commands = d_commands;
	a.count4 = d_count4;
	a.draws = d_draws;
	a.meshlets = d_meshlets;
	const bool soa = ctx->scene->mirroredFrom == d_meshlets && ctx->scene->soaBounds && ctx->scene->poolWords; // (poolWords: the SoA kernels read the pool's bounds unconditionally — ADVICE r5)
	a.soaBounds = soa ? ctx->scene->soaBounds : nullptr;
	a.soaCones = soa ? ctx->scene->soaCones : nullptr;
	a.poolBounds = soa ? reinterpret_cast<const float*>(ctx->scene->poolWords + 2) : nullptr;
	a.blockBounds = soa ? ctx->scene->blockBounds : nullptr;
	a.blockMeshlets = soa ? ctx->scene->mirroredCount : 0u;
	a.mvb = d_meshletVisibility;
	a.masks = ctx->masks;
	a.candList = ctx->candList;
	a.listStride = ctx->listStride;
	a.listMinPer = ctx->listMinPer;
	a.tileCounts = ctx->tileCounts;
	a.scatterTiles = scatter_grid(ctx);
	a.generations = ctx->ccBlocksPerCU;
	a.dealScale = ctx->dealScale;
	{
		// divisions by launch constants, for the kernels' prologues (args.h, host.cpp nv_division_magic): exact for n < 2^39 / d — the
		// largest numerator is 64 x the chunk count < 2^26, d <= 8192
		const uint32_t cullGrid = persistent_grid(ctx, ctx->ccBlocksPerCU);
		a.cullWavesMagic = nv_division_magic(cullGrid * 4u);
		a.genBlocks = cullGrid / 6u ? cullGrid / 6u : 1u;
		a.genBlocksMagic = nv_division_magic(a.genBlocks);
		a.tilesMagic = nv_division_magic(a.scatterTiles);
	}
	// Margin scale of the conservative filter / certified test and the view-only terms of its per-draw derivation: filtermath.h
	// (filter_k: 4 K u S with K = 48, u = 2^-24, S = max(1, |f0| + |f1|, |f2| + |f3|) — the error analysis is written for unit-length plane
	// coefficients; other finite coefficients scale the margins, non-finite or absurd ones, or near / far planes that are not finite,
	// switch both off and every command runs the reference arithmetic.  fp32, no contraction: this file is compiled with
	// -ffp-contract=off like the kernels).
	a.filterK = nv::filter_k(cull->frustum, cull->znear, cull->zfar);
	nv::filter_view_norms(cull->view, &a.viewRowNorm, &a.viewTransNorm, &a.viewSum);
	a.hostHint = ctx->hintDevice;
	return NV_OK;
}

int nv_clustercull(nv_context* ctx, void* stream, const NvCullData* cull, int late, const NvMeshTaskCommand* d_commands,
                   const uint32_t* d_count4, const NvMeshDraw* d_draws, const NvMeshlet* d_meshlets,
                   uint32_t* d_meshletVisibility, const NvPyramidDesc* pyramid, uint32_t* d_clusterIndices,
                   uint32_t* d_clusterCount4)
{
	if (!d_count4 || !d_clusterIndices || !d_clusterCount4)
		return NV_EINVAL;
	nv::ClusterArgs a;
	int rc = fill_cluster_args(ctx, a, cull, late, d_commands, d_count4, d_draws, d_meshlets, d_meshletVisibility, pyramid);
	if (rc)
		return rc;
	DeviceGuard guard(ctx->device);
	a.clusterIndices = d_clusterIndices;
	a.clusterCount4 = d_clusterCount4;
	a.fusedReset = ctx->fusedReset;
	a.fusedSubmit = ctx->fusedSubmit;
	a.countsSink = reinterpret_cast<unsigned long long*>(ctx->countsSink);
#ifdef NV_EXPERIMENTS
	a.debugMode = ctx->debugMode;
	if (ctx->debugMode & (8u | 268435456u)) // bit 3: the cull launch's wave stamps; bit 28: the occlusion stage's phase sums
	{
		// room for the cull launch at any NV_OPT_CULL_WORKGROUPS_PER_CU (4 waves per workgroup) AND for the occlusion stage's grid (bit 28:
		// listSharers x CC_LISTS blocks of 4 waves — more than the cull launch's on a small part or with NV_HIZ_SHARERS raised)
		const size_t timingWaves = std::max((size_t)persistent_grid(ctx, 8) * 4, (size_t)ctx->listSharers * nv::CC_LISTS * 4);
		if (ctx->timingWaves < timingWaves)
			scratch_reset(ctx->timing);
		if (!ctx->timing && scratch_alloc(&ctx->timing, timingWaves * 8 * sizeof(unsigned long long)) == hipSuccess)
			ctx->timingWaves = timingWaves;
		a.probeOut = ctx->timing;
	}
#endif
	// two pure maps: the cull kernel also accumulates survivors per scatter tile, so no workgroup waits on another
	hipStream_t s = (hipStream_t)stream;
	hipEvent_t e0 = prof_mark(ctx, s);
	const bool twoStage = launch_cull(ctx, s, a, false, late, d_commands, &rc).twoStage; // (late pass with HiZ: the occlusion stage follows)
	ctx->variants[NV_VARIANT_HIZ_STAGE] += twoStage ? 1u : 0u;
	hipEvent_t e1 = prof_mark(ctx, s);
	hipEvent_t eh = e1;
	if (rc == 0 && twoStage)
	{
		const uint32_t blocks = ctx->listSharers * nv::CC_LISTS;
		rc = nv::launch_cluster_hiz(s, a, a.soaBounds != nullptr, blocks);
		eh = prof_mark(ctx, s);
	}
	if (rc == 0 && !(ctx->debugMode & 16u)) // bit 4 (experiments): ballots only
		rc = nv::launch_cluster_scatter(s, a, a.scatterTiles, ctx->scatterWaves);
	hipEvent_t e2 = prof_mark(ctx, s);
	prof_push(ctx, NV_PROF_CLUSTER_CULL, e0, e1);
	if (twoStage)
		prof_push(ctx, NV_PROF_CLUSTER_HIZ, e1 ? e1 : nullptr, eh);
	prof_push(ctx, NV_PROF_CLUSTER_SCATTER, eh ? eh : nullptr, e2);
	return rc;
}

int nv_clustersubmit(nv_context* ctx, void* stream, uint32_t* d_clusterCount4, uint32_t* d_clusterIndices)
{
	if (!ctx || !d_clusterCount4 || !d_clusterIndices)
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	return nv::launch_clustersubmit((hipStream_t)stream, d_clusterCount4, d_clusterIndices);
}

int nv_taskcull(nv_context* ctx, void* stream, const NvCullData* cull, int late, const NvMeshTaskCommand* d_commands,
                const uint32_t* d_count4, const NvMeshDraw* d_draws, const NvMeshlet* d_meshlets,
                uint32_t* d_meshletVisibility, const NvPyramidDesc* pyramid, uint32_t* d_payloads, uint32_t* d_payloadCounts)
{
	if (!d_count4 || !d_payloads || !d_payloadCounts)
		return NV_EINVAL;
	nv::ClusterArgs a;
	int rc = fill_cluster_args(ctx, a, cull, late, d_commands, d_count4, d_draws, d_meshlets, d_meshletVisibility, pyramid);
	if (rc)
		return rc;
	DeviceGuard guard(ctx->device);
	a.clusterIndices = d_payloads;
	a.payloadCounts = d_payloadCounts;
	if (!late && !ctx->taskcullOneLaunch)
	{
		// Early pass: nv_clustercull's cull launch (filter / direct / lane-per-set-bit form by the same statistics), which writes the
		// payloads itself when ClusterArgs::payloadCounts is set (clustercull.hip: the end of a segment) — the filter form streams a
		// sparse pass at 8 bytes per meshlet and finishes most commands in 23 instructions, where the one-command-per-wave kernel
		// reads 12 and runs the reference's ~190 for every command (10 M meshlets: 38 us).  The cull kernel only snapshots the count
		// word when the reset is not fused; there is no count word here.
		a.fusedReset = 1u;
		a.clusterCount4 = nullptr;
		(void)launch_cull(ctx, (hipStream_t)stream, a, true, 0, d_commands, &rc);
		return rc;
	}
	return nv::launch_taskcull((hipStream_t)stream, a, late, a.soaBounds != nullptr, (uint32_t)ctx->numCUs * 8);
}

int nv_cluster_expand(nv_context* ctx, void* stream, const NvMeshTaskCommand* d_commands, const NvMeshlet* d_meshlets,
                      const uint32_t* d_clusterIndices, const uint32_t* d_clusterCount4, NvClusterRecord* d_records,
                      uint32_t recordCapacity, uint64_t* d_totals3)
{
	if (!ctx || !d_commands || !d_meshlets || !d_clusterIndices || !d_clusterCount4 || !d_totals3 || (!d_records && recordCapacity))
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	nv::ClusterExpandArgs a;
	a.commands = d_commands;
	a.meshlets = d_meshlets;
	a.clusterIndices = d_clusterIndices;
	a.cc4 = d_clusterCount4;
	a.records = d_records;
	a.capacity = recordCapacity;
	a.totals = reinterpret_cast<unsigned long long*>(d_totals3);
	a.partials = ctx->totalsPartials;
	return nv::launch_cluster_expand((hipStream_t)stream, a, persistent_grid(ctx, 8));
}

int nv_trianglecull(nv_context* ctx, void* stream, const NvGlobals* globals, const NvMeshTaskCommand* d_commands, const NvMeshDraw* d_draws,
                    const NvMeshlet* d_meshlets, const uint32_t* d_meshletData, const NvVertex* d_vertices, const uint32_t* d_clusterIndices,
                    const uint32_t* d_clusterCount4, NvTriangleMask* d_masks, uint32_t maskCapacity, uint64_t* d_totals3)
{
	if (!ctx || !globals || !d_commands || !d_draws || !d_meshlets || !d_meshletData || !d_vertices || !d_clusterIndices || !d_clusterCount4 ||
	    !d_totals3 || (!d_masks && maskCapacity))
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	nv::TriangleArgs a;
	a.globals = *globals;
	a.commands = d_commands;
	a.draws = d_draws;
	a.meshlets = d_meshlets;
	a.meshletData = d_meshletData;
	a.vertices = d_vertices;
	a.clusterIndices = d_clusterIndices;
	a.cc4 = d_clusterCount4;
	a.masks = d_masks;
	a.capacity = maskCapacity;
	a.totals = reinterpret_cast<unsigned long long*>(d_totals3);
	const uint32_t grid = persistent_grid(ctx, 8);
	a.partials = ctx->totalsPartials;
	return nv::launch_trianglecull((hipStream_t)stream, a, grid);
}

int nv_rasterdepth(nv_context* ctx, void* stream, const NvGlobals* globals, const NvMeshTaskCommand* d_commands, const NvMeshDraw* d_draws,
                   const NvMeshlet* d_meshlets, const uint32_t* d_meshletData, const NvVertex* d_vertices, const uint32_t* d_clusterIndices,
                   const uint32_t* d_clusterCount4, float* d_depth, uint32_t width, uint32_t height, uint64_t* d_visibility, uint64_t* d_totals4)
{
	nv::RasterArgs a;
	if (fill_raster_args(a, ctx, globals, d_commands, d_draws, d_meshlets, d_meshletData, d_vertices, d_clusterIndices, d_clusterCount4, d_depth, width, height,
	                     d_visibility, d_totals4) != NV_OK)
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	return nv::launch_rasterdepth((hipStream_t)stream, a, persistent_grid(ctx, 8), ctx->rasterNearClip != 0, ctx->rasterStableIds != 0);
}

int nv_rasterdepth_textured(nv_context* ctx, void* stream, const NvGlobals* globals, const NvMeshTaskCommand* d_commands, const NvMeshDraw* d_draws,
                            const NvMeshlet* d_meshlets, const uint32_t* d_meshletData, const NvVertex* d_vertices, const uint32_t* d_clusterIndices,
                            const uint32_t* d_clusterCount4, float* d_depth, uint32_t width, uint32_t height, uint64_t* d_visibility, uint64_t* d_totals4,
                            const NvMaterial* d_materials, uint32_t materialCount, const NvTextureDesc* d_textures, uint32_t textureCount,
                            const uint32_t* d_texels, uint64_t texelWords, uint64_t* d_alphaTotals2)
{
	nv::RasterAlphaArgs a;
	const int rc = fill_raster_set_args(a, ctx, globals, d_commands, d_draws, d_meshlets, d_meshletData, d_vertices, d_clusterIndices, d_clusterCount4, d_depth,
	                                    width, height, d_visibility, d_totals4, d_materials, materialCount, d_textures, textureCount, d_texels, 3u, texelWords,
	                                    d_alphaTotals2);
	if (rc != NV_OK)
		return rc;
	DeviceGuard guard(ctx->device);
	return nv::launch_rasterdepth_alpha((hipStream_t)stream, a, persistent_grid(ctx, 8), ctx->rasterNearClip != 0, ctx->rasterStableIds != 0);
}

// the same pass over a block-resident set
int nv_rasterdepth_blocks(nv_context* ctx, void* stream, const NvGlobals* globals, const NvMeshTaskCommand* d_commands, const NvMeshDraw* d_draws,
                          const NvMeshlet* d_meshlets, const uint32_t* d_meshletData, const NvVertex* d_vertices, const uint32_t* d_clusterIndices,
                          const uint32_t* d_clusterCount4, float* d_depth, uint32_t width, uint32_t height, uint64_t* d_visibility, uint64_t* d_totals4,
                          const NvMaterial* d_materials, uint32_t materialCount, const NvTextureBlockDesc* d_textures, uint32_t textureCount,
                          const void* d_blocks, uint64_t units16, uint64_t* d_alphaTotals2)
{
	nv::RasterBlockArgs a;
	const int rc = fill_raster_set_args(a, ctx, globals, d_commands, d_draws, d_meshlets, d_meshletData, d_vertices, d_clusterIndices, d_clusterCount4, d_depth,
	                                    width, height, d_visibility, d_totals4, d_materials, materialCount, d_textures, textureCount, d_blocks, 15u, units16,
	                                    d_alphaTotals2);
	if (rc != NV_OK)
		return rc;
	DeviceGuard guard(ctx->device);
	return nv::launch_rasterdepth_blocks((hipStream_t)stream, a, persistent_grid(ctx, 8), ctx->rasterNearClip != 0, ctx->rasterStableIds != 0);
}

int nv_rasterdepth_indexed(nv_context* ctx, void* stream, const NvGlobals* globals, const NvMeshDrawCommand* d_commands, const uint32_t* d_count,
                           const NvMeshDraw* d_draws, uint32_t drawCount, const uint32_t* d_indices, uint32_t indexCapacity,
                           const NvVertex* d_vertices, uint32_t vertexCapacity, float* d_depth, uint32_t width, uint32_t height, uint64_t* d_totals4)
{
	nv::RasterIndexedArgs a;
	const int rc = fill_rasterindexed_args(a, ctx, globals, d_commands, d_count, d_draws, drawCount, d_indices, indexCapacity, d_vertices, vertexCapacity,
	                                       d_depth, width, height, d_totals4);
	if (rc != NV_OK)
		return rc;
	DeviceGuard guard(ctx->device);
	return nv::launch_rasterindexed((hipStream_t)stream, a, ctx->rasterScratch, persistent_grid(ctx, 8), ctx->rasterNearClip != 0);
}

int nv_rasterdepth_indexed_visibility(nv_context* ctx, void* stream, const NvGlobals* globals, const NvMeshDrawCommand* d_commands,
                                      const uint32_t* d_count, const NvMeshDraw* d_draws, uint32_t drawCount, const uint32_t* d_indices,
                                      uint32_t indexCapacity, const NvVertex* d_vertices, uint32_t vertexCapacity, float* d_depth, uint32_t width,
                                      uint32_t height, uint64_t* d_totals4, const uint64_t* d_triangleOffsets, uint64_t* d_visibility)
{
	nv::RasterIndexedVisArgs a;
	const int rc = fill_rasterindexed_args(a, ctx, globals, d_commands, d_count, d_draws, drawCount, d_indices, indexCapacity, d_vertices, vertexCapacity,
	                                       d_depth, width, height, d_totals4);
	if (rc != NV_OK)
		return rc;
	if (!d_triangleOffsets || !d_visibility || misaligned(d_triangleOffsets, 7u) || misaligned(d_visibility, 7u))
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	a.triangleOffsets = reinterpret_cast<const unsigned long long*>(d_triangleOffsets);
	a.visibility = reinterpret_cast<unsigned long long*>(d_visibility);
	return nv::launch_rasterindexed_vis((hipStream_t)stream, a, ctx->rasterScratch, persistent_grid(ctx, 8), ctx->rasterNearClip != 0);
}

int nv_rasterdepth_indexed_textured(nv_context* ctx, void* stream, const NvGlobals* globals, const NvMeshDrawCommand* d_commands, const uint32_t* d_count,
                                    const NvMeshDraw* d_draws, uint32_t drawCount, const uint32_t* d_indices, uint32_t indexCapacity,
                                    const NvVertex* d_vertices, uint32_t vertexCapacity, float* d_depth, uint32_t width, uint32_t height,
                                    uint64_t* d_totals4, const uint64_t* d_triangleOffsets, uint64_t* d_visibility, const NvMaterial* d_materials,
                                    uint32_t materialCount, const NvTextureDesc* d_textures, uint32_t textureCount, const uint32_t* d_texels,
                                    uint64_t texelWords, uint64_t* d_alphaTotals2)
{
	nv::RasterIndexedAlphaArgs a;
	const int rc = fill_rasterindexed_set_args(a, ctx, globals, d_commands, d_count, d_draws, drawCount, d_indices, indexCapacity, d_vertices, vertexCapacity,
	                                           d_depth, width, height, d_totals4, d_triangleOffsets, d_visibility, d_materials, materialCount, d_textures,
	                                           textureCount, d_texels, 3u, texelWords, d_alphaTotals2);
	if (rc != NV_OK)
		return rc;
	DeviceGuard guard(ctx->device);
	return nv::launch_rasterindexed_alpha((hipStream_t)stream, a, ctx->rasterScratch, persistent_grid(ctx, 8), ctx->rasterNearClip != 0);
}

// the same pass over a block-resident set
int nv_rasterdepth_indexed_blocks(nv_context* ctx, void* stream, const NvGlobals* globals, const NvMeshDrawCommand* d_commands, const uint32_t* d_count,
                                  const NvMeshDraw* d_draws, uint32_t drawCount, const uint32_t* d_indices, uint32_t indexCapacity,
                                  const NvVertex* d_vertices, uint32_t vertexCapacity, float* d_depth, uint32_t width, uint32_t height,
                                  uint64_t* d_totals4, const uint64_t* d_triangleOffsets, uint64_t* d_visibility, const NvMaterial* d_materials,
                                  uint32_t materialCount, const NvTextureBlockDesc* d_textures, uint32_t textureCount, const void* d_blocks,
                                  uint64_t units16, uint64_t* d_alphaTotals2)
{
	nv::RasterIndexedBlockArgs a;
	const int rc = fill_rasterindexed_set_args(a, ctx, globals, d_commands, d_count, d_draws, drawCount, d_indices, indexCapacity, d_vertices, vertexCapacity,
	                                           d_depth, width, height, d_totals4, d_triangleOffsets, d_visibility, d_materials, materialCount, d_textures,
	                                           textureCount, d_blocks, 15u, units16, d_alphaTotals2);
	if (rc != NV_OK)
		return rc;
	DeviceGuard guard(ctx->device);
	return nv::launch_rasterindexed_blocks((hipStream_t)stream, a, ctx->rasterScratch, persistent_grid(ctx, 8), ctx->rasterNearClip != 0);
}

int nv_meshlet_bounds(nv_context* ctx, void* stream, const NvVertex* d_vertices, const uint32_t* d_meshletData, NvMeshlet* d_meshlets, uint32_t meshletCount,
                      float* d_bounds8)
{
	if (!ctx || (meshletCount && (!d_vertices || !d_meshletData || !d_meshlets)))
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	int rc = nv::launch_meshlet_bounds((hipStream_t)stream, d_vertices, d_meshletData, d_meshlets, meshletCount, d_bounds8,
	                                   nv::capped_grid(meshletCount, 4, persistent_grid(ctx, 16)));
	// a mirror built from these records is stale now (its registration is by pointer, its contents a snapshot)
	if (rc == 0 && ctx->scene->mirroredFrom == d_meshlets)
		ctx->scene->mirroredFrom = nullptr;
	return rc;
}

int nv_depthreduce(nv_context* ctx, void* stream, const float* d_depth, uint32_t width, uint32_t height,
                   const NvPyramidDesc* pyramid)
{
	if (!ctx || !d_depth || !pyramid || !pyramid->d_base || !width || !height || !pyramid->levels || pyramid->levels > NV_MAX_MIPS)
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	hipEvent_t e0 = prof_mark(ctx, (hipStream_t)stream);
	int rc = nv::launch_depthreduce((hipStream_t)stream, d_depth, width, height, *pyramid);
	prof_push(ctx, NV_PROF_DEPTHREDUCE, e0, prof_mark(ctx, (hipStream_t)stream));
	return rc;
}

int nv_depth_merge(nv_context* ctx, void* stream, float* d_dst, const float* const* d_srcs, uint32_t sources, uint32_t width, uint32_t height)
{
	if (!ctx || !d_dst || !d_srcs || sources == 0 || !image_size_ok(width, height) || misaligned(d_dst, 3u))
		return NV_EINVAL;
	for (uint32_t i = 0; i < sources; ++i)
		if (!d_srcs[i] || d_srcs[i] == d_dst || misaligned(d_srcs[i], 3u))
			return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	return nv::launch_depth_merge((hipStream_t)stream, d_dst, d_srcs, sources, width * height, persistent_grid(ctx, 8));
}

int nv_visibility_resolve(nv_context* ctx, void* stream, const NvCullData* cull, const uint64_t* d_visibility, uint32_t width, uint32_t height,
                          const NvMeshDraw* d_draws, uint32_t drawCount, const NvMesh* d_meshes, uint32_t meshCount, NvVisRecord* d_records,
                          uint32_t* d_meshletSeen, uint32_t* d_drawPixels, uint64_t* d_totals4)
{
	if (!ctx || !cull || !d_visibility || !image_size_ok(width, height) || (drawCount && !d_draws) || (meshCount && !d_meshes) ||
	    misaligned(d_visibility, 7u) || misaligned(d_records, 15u) || misaligned(d_totals4, 7u))
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	nv::VisResolveArgs a;
	a.cd = *cull;
	a.visibility = reinterpret_cast<const unsigned long long*>(d_visibility);
	a.n = width * height;
	a.draws = d_draws;
	a.drawCount = drawCount;
	a.meshes = d_meshes;
	a.meshCount = meshCount;
	a.records = reinterpret_cast<uint4*>(d_records);
	a.meshletSeen = d_meshletSeen;
	a.drawPixels = d_drawPixels;
	a.totals = reinterpret_cast<unsigned long long*>(d_totals4);
	return nv::launch_visibility_resolve((hipStream_t)stream, a, persistent_grid(ctx, 8), ctx->resolvePerPixel != 0);
}

int nv_visibility_resolve_indexed(nv_context* ctx, void* stream, const NvCullData* cull, const uint64_t* d_visibility, uint32_t width, uint32_t height,
                                  const NvMeshDraw* d_draws, uint32_t drawCount, const NvMesh* d_meshes, uint32_t meshCount,
                                  const uint64_t* d_triangleOffsets, NvVisIndexedRecord* d_records, uint32_t* d_drawPixels, uint64_t* d_totals4)
{
	if (!ctx || !cull || !d_visibility || !d_triangleOffsets || !image_size_ok(width, height) || (drawCount && !d_draws) || (meshCount && !d_meshes) ||
	    misaligned(d_visibility, 7u) || misaligned(d_triangleOffsets, 7u) || misaligned(d_records, 15u) || misaligned(d_totals4, 7u) ||
	    misaligned(d_draws, 15u) || misaligned(d_meshes, 15u))
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	nv::VisResolveIndexedArgs a;
	a.cd = *cull;
	a.visibility = reinterpret_cast<const unsigned long long*>(d_visibility);
	a.n = width * height;
	a.draws = d_draws;
	a.drawCount = drawCount;
	a.meshes = d_meshes;
	a.meshCount = meshCount;
	a.triangleOffsets = reinterpret_cast<const unsigned long long*>(d_triangleOffsets);
	a.records = reinterpret_cast<uint4*>(d_records);
	a.drawPixels = d_drawPixels;
	a.totals = reinterpret_cast<unsigned long long*>(d_totals4);
	return nv::launch_visibility_resolve_indexed((hipStream_t)stream, a, persistent_grid(ctx, 8));
}

int nv_visibility_attributes(nv_context* ctx, void* stream, const NvGlobals* globals, const NvVisRecord* d_records, uint32_t width, uint32_t height,
                             const NvMeshDraw* d_draws, uint32_t drawCount, const NvMeshlet* d_meshlets, uint32_t meshletCount,
                             const uint32_t* d_meshletData, uint32_t meshletDataWords, const NvVertex* d_vertices, uint32_t vertexCount,
                             const NvMaterial* d_materials, uint32_t materialCount, NvPixelAttributes* d_attributes, uint32_t* d_gbuffer0,
                             uint32_t* d_gbuffer1, uint64_t* d_totals4)
{
	nv::VisAttrArgs a;
	if (fill_attribute_args(a, ctx, globals, d_records, width, height, d_draws, drawCount, d_meshlets, meshletCount, d_meshletData, meshletDataWords, d_vertices,
	                        vertexCount, d_materials, materialCount, d_attributes, d_gbuffer0, d_gbuffer1, d_totals4) != NV_OK ||
	    (materialCount && !d_materials) || ((d_gbuffer0 || d_gbuffer1) && !d_materials))
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	return nv::launch_visibility_attributes((hipStream_t)stream, a, height, persistent_grid(ctx, 8), ctx->attributesPerPixel != 0);
}

int nv_visibility_attributes_indexed(nv_context* ctx, void* stream, const NvGlobals* globals, const NvVisIndexedRecord* d_records, uint32_t width,
                                     uint32_t height, const NvMeshDraw* d_draws, uint32_t drawCount, const uint32_t* d_indices, uint32_t indexCapacity,
                                     const NvVertex* d_vertices, uint32_t vertexCapacity, const NvMaterial* d_materials, uint32_t materialCount,
                                     NvPixelAttributes* d_attributes, uint32_t* d_gbuffer0, uint32_t* d_gbuffer1, uint64_t* d_totals4)
{
	nv::VisAttrIndexedArgs a;
	if (fill_attribute_args(a, ctx, globals, reinterpret_cast<const NvVisRecord*>(d_records), width, height, d_draws, drawCount, nullptr, 0u, nullptr, 0u,
	                        d_vertices, vertexCapacity, d_materials, materialCount, d_attributes, d_gbuffer0, d_gbuffer1, d_totals4) != NV_OK ||
	    (materialCount && !d_materials) || ((d_gbuffer0 || d_gbuffer1) && !d_materials) || (indexCapacity && !d_indices) || misaligned(d_indices, 3u))
		return NV_EINVAL;
	a.indices = d_indices;
	a.indexCapacity = indexCapacity;
	DeviceGuard guard(ctx->device);
	return nv::launch_visibility_attributes_indexed((hipStream_t)stream, a, height, persistent_grid(ctx, 8));
}

// ---- material textures (texdecode.hip, visattr_tex.hip)
int nv_visibility_attributes_textured(nv_context* ctx, void* stream, const NvGlobals* globals, const NvVisRecord* d_records, uint32_t width,
                                      uint32_t height, const NvMeshDraw* d_draws, uint32_t drawCount, const NvMeshlet* d_meshlets,
                                      uint32_t meshletCount, const uint32_t* d_meshletData, uint32_t meshletDataWords, const NvVertex* d_vertices,
                                      uint32_t vertexCount, const NvMaterial* d_materials, uint32_t materialCount, NvPixelAttributes* d_attributes,
                                      uint32_t* d_gbuffer0, uint32_t* d_gbuffer1, uint64_t* d_totals4, const NvTextureDesc* d_textures,
                                      uint32_t textureCount, const uint32_t* d_texels, uint64_t texelWords)
{
	nv::VisAttrTexArgs a;
	if (fill_attribute_set_args(a, ctx, globals, d_records, width, height, d_draws, drawCount, d_meshlets, meshletCount, d_meshletData, meshletDataWords,
	                            d_vertices, vertexCount, d_materials, materialCount, d_attributes, d_gbuffer0, d_gbuffer1, d_totals4, d_textures, textureCount,
	                            d_texels, 3u, texelWords) != NV_OK)
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	return nv::launch_visibility_attributes_textured((hipStream_t)stream, a, height, persistent_grid(ctx, 8));
}

// the same pass over a block-resident set
int nv_visibility_attributes_blocks(nv_context* ctx, void* stream, const NvGlobals* globals, const NvVisRecord* d_records, uint32_t width,
                                    uint32_t height, const NvMeshDraw* d_draws, uint32_t drawCount, const NvMeshlet* d_meshlets,
                                    uint32_t meshletCount, const uint32_t* d_meshletData, uint32_t meshletDataWords, const NvVertex* d_vertices,
                                    uint32_t vertexCount, const NvMaterial* d_materials, uint32_t materialCount, NvPixelAttributes* d_attributes,
                                    uint32_t* d_gbuffer0, uint32_t* d_gbuffer1, uint64_t* d_totals4, const NvTextureBlockDesc* d_textures,
                                    uint32_t textureCount, const void* d_blocks, uint64_t units16)
{
	nv::VisAttrBlockArgs a;
	if (fill_attribute_set_args(a, ctx, globals, d_records, width, height, d_draws, drawCount, d_meshlets, meshletCount, d_meshletData, meshletDataWords,
	                            d_vertices, vertexCount, d_materials, materialCount, d_attributes, d_gbuffer0, d_gbuffer1, d_totals4, d_textures, textureCount,
	                            d_blocks, 15u, units16) != NV_OK)
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	return nv::launch_visibility_attributes_blocks((hipStream_t)stream, a, height, persistent_grid(ctx, 8));
}

int nv_visibility_attributes_indexed_textured(nv_context* ctx, void* stream, const NvGlobals* globals, const NvVisIndexedRecord* d_records, uint32_t width,
                                              uint32_t height, const NvMeshDraw* d_draws, uint32_t drawCount, const uint32_t* d_indices,
                                              uint32_t indexCapacity, const NvVertex* d_vertices, uint32_t vertexCapacity, const NvMaterial* d_materials,
                                              uint32_t materialCount, NvPixelAttributes* d_attributes, uint32_t* d_gbuffer0, uint32_t* d_gbuffer1,
                                              uint64_t* d_totals4, const NvTextureDesc* d_textures, uint32_t textureCount, const uint32_t* d_texels,
                                              uint64_t texelWords)
{
	nv::VisAttrIndexedTexArgs a;
	if (fill_attribute_indexed_set_args(a, ctx, globals, d_records, width, height, d_draws, drawCount, d_indices, indexCapacity, d_vertices, vertexCapacity,
	                                    d_materials, materialCount, d_attributes, d_gbuffer0, d_gbuffer1, d_totals4, d_textures, textureCount, d_texels, 3u,
	                                    texelWords) != NV_OK)
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	return nv::launch_visibility_attributes_indexed_textured((hipStream_t)stream, a, height, persistent_grid(ctx, 8));
}

// the same pass over a block-resident set
int nv_visibility_attributes_indexed_blocks(nv_context* ctx, void* stream, const NvGlobals* globals, const NvVisIndexedRecord* d_records, uint32_t width,
                                            uint32_t height, const NvMeshDraw* d_draws, uint32_t drawCount, const uint32_t* d_indices,
                                            uint32_t indexCapacity, const NvVertex* d_vertices, uint32_t vertexCapacity, const NvMaterial* d_materials,
                                            uint32_t materialCount, NvPixelAttributes* d_attributes, uint32_t* d_gbuffer0, uint32_t* d_gbuffer1,
                                            uint64_t* d_totals4, const NvTextureBlockDesc* d_textures, uint32_t textureCount, const void* d_blocks,
                                            uint64_t units16)
{
	nv::VisAttrIndexedBlockArgs a;
	if (fill_attribute_indexed_set_args(a, ctx, globals, d_records, width, height, d_draws, drawCount, d_indices, indexCapacity, d_vertices, vertexCapacity,
	                                    d_materials, materialCount, d_attributes, d_gbuffer0, d_gbuffer1, d_totals4, d_textures, textureCount, d_blocks, 15u,
	                                    units16) != NV_OK)
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	return nv::launch_visibility_attributes_indexed_blocks((hipStream_t)stream, a, height, persistent_grid(ctx, 8));
}

int nv_texture_decode(nv_context* ctx, void* stream, const void* d_blocks, uint32_t format, uint32_t width, uint32_t height, uint32_t levels,
                      uint32_t* d_texels, const NvTextureDesc* desc)
{
	if (!ctx || !d_blocks || !d_texels || !desc || !image_size_ok(width, height) || levels == 0 || levels > NV_TEXTURE_MAX_LEVELS ||
	    desc->width != width || desc->height != height || desc->levels != levels || misaligned(d_blocks, 7u) || misaligned(d_texels, 3u))
		return NV_EINVAL;
	if (format == NV_FORMAT_BC4 || format == NV_FORMAT_BC5 || format == NV_FORMAT_BC6H)
		return NV_ETEXFORMAT;
	if (format != NV_FORMAT_BC1 && format != NV_FORMAT_BC2 && format != NV_FORMAT_BC3 && format != NV_FORMAT_BC7)
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	return nv::launch_texture_decode((hipStream_t)stream, d_blocks, format, width, height, levels, d_texels + desc->offset);
}

// ---- the shading end of the frame (shade.hip)
int nv_shadow_fill(nv_context* ctx, void* stream, uint8_t* d_shadow, const float* d_depth, uint32_t width, uint32_t height, int checkerboard)
{
	if (!ctx || !d_shadow || !d_depth || !image_size_ok(width, height) || misaligned(d_depth, 3u))
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	return nv::launch_shadow_fill((hipStream_t)stream, d_shadow, d_depth, width, height, checkerboard, persistent_grid(ctx, 8));
}

int nv_shadow_blur(nv_context* ctx, void* stream, uint8_t* d_out, const uint8_t* d_shadow, const float* d_depth, uint32_t width, uint32_t height,
                   int direction, float znear)
{
	if (!ctx || !d_out || !d_shadow || !d_depth || d_out == d_shadow || !image_size_ok(width, height) || (direction != 0 && direction != 1) ||
	    misaligned(d_depth, 3u))
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	return nv::launch_shadow_blur((hipStream_t)stream, d_out, d_shadow, d_depth, width, height, direction == 1, znear);
}

// what nv_shade_final and nv_shade_final_bloom share: the refusals, then the caller-facing fields of the launch (a.bloom stays nullptr)
static int fill_shade_args(nv::ShadeFinalBloomArgs& a, nv_context* ctx, const NvShadeData* shade, const uint32_t* d_gbuffer0, const uint32_t* d_gbuffer1,
                           const float* d_depth, const uint8_t* d_shadow, uint32_t* d_color, uint32_t width, uint32_t height)
{
	if (!ctx || !shade || !d_gbuffer0 || !d_gbuffer1 || !d_depth || !d_color || !image_size_ok(width, height) || shade->imageSize[0] != (float)width ||
	    shade->imageSize[1] != (float)height || (shade->shadowsEnabled == 1 && !d_shadow) || misaligned(d_gbuffer0, 3u) || misaligned(d_gbuffer1, 3u) ||
	    misaligned(d_depth, 3u) || misaligned(d_color, 3u))
		return NV_EINVAL;
	a.sd = *shade;
	a.gbuffer0 = d_gbuffer0;
	a.gbuffer1 = d_gbuffer1;
	a.depth = d_depth;
	a.shadow = d_shadow;
	a.color = d_color;
	a.width = width;
	a.bloom = nullptr;
	a.bloomWidth = a.bloomHeight = 0;
	return NV_OK;
}

int nv_shade_final(nv_context* ctx, void* stream, const NvShadeData* shade, const uint32_t* d_gbuffer0, const uint32_t* d_gbuffer1, const float* d_depth,
                   const uint8_t* d_shadow, uint32_t* d_color, uint32_t width, uint32_t height)
{
	nv::ShadeFinalBloomArgs a;
	if (fill_shade_args(a, ctx, shade, d_gbuffer0, d_gbuffer1, d_depth, d_shadow, d_color, width, height) != NV_OK)
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	return nv::launch_shade_final((hipStream_t)stream, a, height, persistent_grid(ctx, 8));
}

// ---- ray-traced sun shadows (shadowtrace.hip, rtbuild.cpp)
// Load time, like nv_reserve: allocates, copies and synchronises.  Only a blob nv_rt_scene_validate accepts reaches the device: every index the
// kernel follows stays inside the copy and every loop it runs ends.
int nv_rt_scene_upload(nv_context* ctx, void* stream, const void* blob, uint64_t bytes)
{
	if (!ctx || (blob == nullptr) != (bytes == 0))
		return NV_EINVAL;
	if (blob && nv_rt_scene_validate(blob, bytes) != NV_OK)
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	hipError_t e = hipStreamSynchronize((hipStream_t)stream); // a launch that still reads the old copy
	if (e != hipSuccess)
		return (int)e;
	void* fresh = nullptr;
	if (blob)
	{
		if (scratch_alloc(&fresh, (size_t)bytes) != hipSuccess)
			return NV_ENOMEM;
		e = hipMemcpy(fresh, blob, (size_t)bytes, hipMemcpyHostToDevice);
		if (e != hipSuccess)
		{
			scratch_free(fresh);
			return (int)e;
		}
	}
	if (ctx->rtScene)
		scratch_free(ctx->rtScene);
	ctx->rtScene = fresh;
	ctx->rtSceneBytes = bytes;
	ctx->rtSceneFlags = blob ? static_cast<const nv::RtHeader*>(blob)->flags : 0u;
	memset(&ctx->rtPlan, 0, sizeof(ctx->rtPlan)); // static again
	return NV_OK;
}

// ---- the TLAS rebuilt on the device (rttlas.hip)
// Load time: re-houses the device scene in one allocation [static blob][2 maxDraws TLAS nodes][maxDraws instances][scratch].  The header is
// copied with the blob: it keeps pointing at the static TLAS until the first nv_rt_tlas_build.
int nv_rt_scene_reserve_dynamic(nv_context* ctx, void* stream, uint32_t maxDraws)
{
	if (!ctx || !ctx->rtScene || maxDraws == 0 || maxDraws > nv::RT_LEAF_FIRST)
		return NV_EINVAL;
	nv::TlasPlan plan;
	if (nv::tlas_plan(ctx->rtSceneBytes, maxDraws, &plan) == 0)
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	hipError_t e = hipStreamSynchronize((hipStream_t)stream); // a launch that still reads the old copy
	if (e != hipSuccess)
		return (int)e;
	void* fresh = nullptr;
	if (scratch_alloc(&fresh, (size_t)plan.bytes) != hipSuccess)
		return NV_ENOMEM;
	nv::RtHeader h;
	e = hipMemcpy(&h, ctx->rtScene, sizeof(h), hipMemcpyDeviceToHost);
	if (e == hipSuccess && ctx->rtPlan.maxDraws) // reserved before: back to the canonical sections, the current TLAS included
	{
		std::vector<unsigned char> blob;
		uint64_t bytes = 0;
		int rc = nv_rt_scene_download(ctx, stream, nullptr, &bytes);
		if (rc == NV_OK)
		{
			blob.resize((size_t)bytes + 16u);
			unsigned char* at = blob.data() + ((16u - (reinterpret_cast<uintptr_t>(blob.data()) & 15u)) & 15u);
			rc = nv_rt_scene_download(ctx, stream, at, &bytes);
			if (rc == NV_OK && nv::tlas_plan(bytes, maxDraws, &plan) != 0)
			{
				scratch_free(fresh);
				fresh = nullptr;
				if (scratch_alloc(&fresh, (size_t)plan.bytes) != hipSuccess)
					return NV_ENOMEM;
				e = hipMemcpy(fresh, at, (size_t)bytes, hipMemcpyHostToDevice);
				ctx->rtSceneBytes = e == hipSuccess ? bytes : ctx->rtSceneBytes;
			}
			else
				rc = rc == NV_OK ? NV_EINVAL : rc;
		}
		if (rc != NV_OK)
		{
			scratch_free(fresh);
			return rc;
		}
	}
	else if (e == hipSuccess)
		e = hipMemcpy(fresh, ctx->rtScene, (size_t)ctx->rtSceneBytes, hipMemcpyDeviceToDevice);
	if (e != hipSuccess)
	{
		scratch_free(fresh);
		return (int)e;
	}
	scratch_free(ctx->rtScene);
	ctx->rtScene = fresh;
	ctx->rtPlan = plan;
	return NV_OK;
}

// Only enqueues: two memset nodes and the launches of rttlas.hip; the draws are read on the device when the launches run
int nv_rt_tlas_build(nv_context* ctx, void* stream, const NvMeshDraw* d_draws, uint32_t drawCount)
{
	if (!ctx || !ctx->rtScene || ctx->rtPlan.maxDraws == 0 || drawCount > ctx->rtPlan.maxDraws || (drawCount && !d_draws) ||
	    misaligned(d_draws, 3u))
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	return nv::launch_tlas_build((hipStream_t)stream, ctx->rtScene, ctx->rtPlan, d_draws, drawCount);
}

// ---- keyframe animation on the device (animate.hip, animmath.h)
// Load time, like nv_rt_scene_upload: validates, allocates, copies and synchronises.  Only a table nv_animation_validate_host accepts reaches
// the device: every keyframe and target index the kernel follows stays inside the bounds kept here, and no two lanes share a target.
int nv_upload_animations(nv_context* ctx, void* stream, const NvAnimation* h_animations, uint32_t animationCount, const NvKeyframe* h_keyframes,
                         uint32_t keyframeCount, uint32_t drawCount, uint32_t lightCount)
{
	if (!ctx || (!h_animations && animationCount) || (!h_keyframes && keyframeCount))
		return NV_EINVAL;
	if (nv_animation_validate_host(h_animations, animationCount, keyframeCount, drawCount, lightCount, nullptr, nullptr) != NV_OK)
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	hipError_t e = hipStreamSynchronize((hipStream_t)stream); // a launch that still reads the old copy
	if (e != hipSuccess)
		return (int)e;
	ctx->animUploaded = false;
	ctx->animCount = 0;
	if (!h_animations || animationCount > ctx->animCapacity || keyframeCount > ctx->animKeyCapacity)
	{
		if ((e = hipDeviceSynchronize()) != hipSuccess) // as nv_upload_draws: another stream may still be reading the old copies
			return (int)e;
		scratch_reset(ctx->animRecords);
		scratch_reset(ctx->animTimes);
		scratch_reset(ctx->animKeyframes);
		ctx->animCapacity = ctx->animKeyCapacity = 0;
		if (!h_animations)
			return NV_OK; // dropped
		if (scratch_alloc(&ctx->animRecords, (size_t)(animationCount ? animationCount : 1u) * sizeof(uint4)) != hipSuccess ||
		    scratch_alloc(&ctx->animTimes, (size_t)(animationCount ? animationCount : 1u) * sizeof(float2)) != hipSuccess ||
		    scratch_alloc(&ctx->animKeyframes, (size_t)(keyframeCount ? keyframeCount : 1u) * sizeof(NvKeyframe)) != hipSuccess)
		{
			scratch_reset(ctx->animRecords);
			scratch_reset(ctx->animTimes);
			scratch_reset(ctx->animKeyframes);
			return NV_ENOMEM;
		}
		ctx->animCapacity = animationCount;
		ctx->animKeyCapacity = keyframeCount;
	}
	if (animationCount)
	{
		// the 24-byte records as two streams a wave loads with one vector load each
		std::vector<uint4> records;
		std::vector<float2> times;
		try
		{
			records.resize(animationCount);
			times.resize(animationCount);
		}
		catch (...)
		{
			return NV_ENOMEM;
		}
		for (uint32_t i = 0; i < animationCount; ++i)
		{
			const NvAnimation& a = h_animations[i];
			records[i] = make_uint4((uint32_t)a.drawIndex, (uint32_t)a.lightIndex, a.keyframeOffset, a.keyframeCount);
			times[i] = make_float2(a.startTime, a.period);
		}
		if ((e = hipMemcpy(ctx->animRecords, records.data(), (size_t)animationCount * sizeof(uint4), hipMemcpyHostToDevice)) != hipSuccess ||
		    (e = hipMemcpy(ctx->animTimes, times.data(), (size_t)animationCount * sizeof(float2), hipMemcpyHostToDevice)) != hipSuccess ||
		    (e = hipMemcpy(ctx->animKeyframes, h_keyframes, (size_t)keyframeCount * sizeof(NvKeyframe), hipMemcpyHostToDevice)) != hipSuccess)
			return (int)e;
	}
	ctx->animCount = animationCount;
	ctx->animDrawBound = drawCount;
	ctx->animLightBound = lightCount;
	ctx->animUploaded = true;
	return NV_OK;
}

// Only enqueues: one launch, `time` by value
int nv_animate_draws(nv_context* ctx, void* stream, double time, NvMeshDraw* d_draws, uint32_t drawCount, NvLight* d_lights, uint32_t lightCount)
{
	if (!ctx || !(fabs(time) <= DBL_MAX))
		return NV_EINVAL;
	if (!ctx->animUploaded)
		return NV_ESTATE;
	if (drawCount < ctx->animDrawBound || (ctx->animDrawBound && !d_draws) || misaligned(d_draws, 15u) || (d_lights && lightCount < ctx->animLightBound) ||
	    misaligned(d_lights, 3u))
		return NV_EINVAL;
	if (!ctx->animCount)
		return NV_OK;
	nv::AnimateArgs a;
	a.time = time;
	a.records = ctx->animRecords;
	a.times = ctx->animTimes;
	a.keyframes = ctx->animKeyframes;
	a.count = ctx->animCount;
	a.draws = reinterpret_cast<float4*>(d_draws);
	a.lights = reinterpret_cast<float*>(d_lights);
	// the draws the table can name lie in the registered buffer: the lane writes their mirror entries too (nv_update_draws' statements)
	const nv_scene* sc = ctx->scene;
	size_t base = 0;
	const bool mirror = d_draws && sc->soaWorld && sc->drawsMeshes && registered_draw_range(sc, d_draws, ctx->animDrawBound, &base);
	a.meshes = mirror ? sc->drawsMeshes : nullptr;
	a.meshCount = mirror && sc->meshesFrom == sc->drawsMeshes ? sc->meshCount : 0u;
	a.world = mirror ? sc->soaWorld + base : nullptr;
	a.scaleMesh = mirror ? sc->soaScaleMesh + base : nullptr;
	DeviceGuard guard(ctx->device);
	return nv::launch_animate((hipStream_t)stream, a, mirror);
}

// Test and tooling accessor (synchronises): the context's current scene as a canonical blob
int nv_rt_scene_download(nv_context* ctx, void* stream, void* out, uint64_t* bytes)
{
	if (!ctx || !ctx->rtScene || !bytes || misaligned(out, 15u))
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	hipError_t e = hipStreamSynchronize((hipStream_t)stream);
	if (e != hipSuccess)
		return (int)e;
	const unsigned char* base = static_cast<const unsigned char*>(ctx->rtScene);
	nv::RtHeader h;
	if ((e = hipMemcpy(&h, base, sizeof(h), hipMemcpyDeviceToHost)) != hipSuccess)
		return (int)e;
	const uint64_t room = ctx->rtPlan.maxDraws ? ctx->rtPlan.bytes : ctx->rtSceneBytes;
	const uint64_t sizes[5] = { (uint64_t)h.meshCount * sizeof(nv::RtBlas), (uint64_t)h.tlasNodes * sizeof(nv::RtNode), (uint64_t)h.instances * sizeof(nv::RtInstance),
		                        (uint64_t)h.blasNodes * sizeof(nv::RtNode), (uint64_t)h.triangles * 48u };
	const uint32_t offs[5] = { h.tableOff, h.tlasOff, h.instOff, h.blasOff, h.triOff };
	try
	{
		std::vector<unsigned char> parts[5];
		for (int i = 0; i < 5; ++i)
		{
			if ((uint64_t)offs[i] + sizes[i] > room)
				return NV_EINVAL;
			parts[i].resize((size_t)sizes[i] + 1u);
			if (sizes[i] && (e = hipMemcpy(parts[i].data(), base + offs[i], (size_t)sizes[i], hipMemcpyDeviceToHost)) != hipSuccess)
				return (int)e;
		}
		return nv::rt_pack_blob(h, reinterpret_cast<const nv::RtBlas*>(parts[0].data()), reinterpret_cast<const nv::RtNode*>(parts[1].data()), h.tlasNodes,
		                        reinterpret_cast<const nv::RtInstance*>(parts[2].data()), h.instances, reinterpret_cast<const nv::RtNode*>(parts[3].data()),
		                        reinterpret_cast<const nv::RtF4*>(parts[4].data()), h.padOrigin, h.drawCount, out, bytes);
	}
	catch (const std::bad_alloc&)
	{
		return NV_ENOMEM;
	}
}

int nv_shadow_trace(nv_context* ctx, void* stream, const NvShadowData* shadow, const float* d_depth, uint8_t* d_shadow, uint32_t width, uint32_t height,
                    int quality)
{
	nv::ShadowTraceArgs a;
	if (fill_trace_args(a, ctx, shadow, d_depth, d_shadow, width, height, quality) != NV_OK)
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	return nv::launch_shadow_trace((hipStream_t)stream, a, quality, persistent_grid(ctx, 8));
}

// the alpha-tested trace; quality 0 has no alpha test and is nv_shadow_trace's launch
int nv_shadow_trace_textured(nv_context* ctx, void* stream, const NvShadowData* shadow, const float* d_depth, uint8_t* d_shadow, uint32_t width, uint32_t height,
                             int quality, const NvMeshDraw* d_draws, uint32_t drawCount, const NvMaterial* d_materials, uint32_t materialCount,
                             const NvTextureDesc* d_textures, uint32_t textureCount, const uint32_t* d_texels, uint64_t texelWords)
{
	nv::ShadowTraceArgs opaque;
	nv::ShadowTraceAlphaArgs a;
	if (fill_trace_alpha(a, opaque, ctx, shadow, d_depth, d_shadow, width, height, quality, d_draws, drawCount, d_materials, materialCount, d_textures,
	                     textureCount, d_texels, 3u, texelWords) != NV_OK)
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	if (quality == 0)
		return nv::launch_shadow_trace((hipStream_t)stream, opaque, 0, persistent_grid(ctx, 8));
	return nv::launch_shadow_trace_alpha((hipStream_t)stream, a, persistent_grid(ctx, 8));
}

// the same over a block-resident set
int nv_shadow_trace_blocks(nv_context* ctx, void* stream, const NvShadowData* shadow, const float* d_depth, uint8_t* d_shadow, uint32_t width, uint32_t height,
                           int quality, const NvMeshDraw* d_draws, uint32_t drawCount, const NvMaterial* d_materials, uint32_t materialCount,
                           const NvTextureBlockDesc* d_textures, uint32_t textureCount, const void* d_blocks, uint64_t units16)
{
	nv::ShadowTraceArgs opaque;
	nv::ShadowTraceBlockArgs a;
	if (fill_trace_alpha(a, opaque, ctx, shadow, d_depth, d_shadow, width, height, quality, d_draws, drawCount, d_materials, materialCount, d_textures,
	                     textureCount, d_blocks, 15u, units16) != NV_OK)
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	if (quality == 0)
		return nv::launch_shadow_trace((hipStream_t)stream, opaque, 0, persistent_grid(ctx, 8));
	return nv::launch_shadow_trace_blocks((hipStream_t)stream, a, persistent_grid(ctx, 8));
}

// ---- bloom (bloom.hip)
// desc is what nv_bloom_desc_init gives for a width x height image
static bool bloom_desc_ok(const NvBloomDesc* desc, uint32_t width, uint32_t height)
{
	NvBloomDesc want;
	return desc && nv_bloom_desc_init(&want, width, height) == NV_OK && memcmp(&want, desc, sizeof(want)) == 0;
}

// the per-level passes take no image size: desc is what nv_bloom_desc_init gives for its own level 0 (an image of twice that size)
static bool bloom_desc_ok(const NvBloomDesc* desc)
{
	return desc && desc->width != 0 && desc->height != 0 && desc->width <= 8192 && desc->height <= 8192 && bloom_desc_ok(desc, desc->width * 2u, desc->height * 2u);
}

int nv_bloom_extract(nv_context* ctx, void* stream, const uint32_t* d_gbuffer0, uint32_t width, uint32_t height, uint32_t* d_bloom, const NvBloomDesc* desc)
{
	if (!ctx || !d_gbuffer0 || !d_bloom || !image_size_ok(width, height) || !bloom_desc_ok(desc, width, height) || misaligned(d_gbuffer0, 3u) || misaligned(d_bloom, 3u))
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	return nv::launch_bloom_extract((hipStream_t)stream, d_gbuffer0, width, height, d_bloom, *desc, persistent_grid(ctx, 8));
}

int nv_bloom_downsample(nv_context* ctx, void* stream, uint32_t* d_bloom, const NvBloomDesc* desc, uint32_t level)
{
	if (!ctx || !d_bloom || !bloom_desc_ok(desc) || level < 1u || level >= desc->levels || misaligned(d_bloom, 3u))
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	return nv::launch_bloom_downsample((hipStream_t)stream, d_bloom, *desc, level);
}

int nv_bloom_upsample(nv_context* ctx, void* stream, uint32_t* d_bloom, const NvBloomDesc* desc, uint32_t level, float radius)
{
	// (level + 2 > levels would wrap for a level near 2^32 and let it through)
	if (!ctx || !d_bloom || !bloom_desc_ok(desc) || desc->levels < 2u || level > desc->levels - 2u || !(radius >= 0.0f) || !(radius <= 3.402823466e38f) || misaligned(d_bloom, 3u))
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	return nv::launch_bloom_upsample((hipStream_t)stream, d_bloom, *desc, level, radius);
}

int nv_bloom(nv_context* ctx, void* stream, const uint32_t* d_gbuffer0, uint32_t width, uint32_t height, uint32_t* d_bloom, const NvBloomDesc* desc)
{
	if (!ctx || !d_gbuffer0 || !d_bloom || !image_size_ok(width, height) || !bloom_desc_ok(desc, width, height) || misaligned(d_gbuffer0, 3u) || misaligned(d_bloom, 3u))
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	// src/niagara.cpp:1873-1901
	int rc = nv::launch_bloom_extract((hipStream_t)stream, d_gbuffer0, width, height, d_bloom, *desc, persistent_grid(ctx, 8));
	// the fused tail takes the levels from `tail` on (pass 1 into tail + 1 .. levels - 1, pass 2 into levels - 2 .. tail) when that saves a launch
	uint32_t tail = desc->levels;
	if (ctx->bloomFusedTail)
	{
		tail = nv::bloom_tail_first(*desc);
		if (tail + 2u > desc->levels)
			tail = desc->levels;
	}
	const uint32_t lastDown = tail < desc->levels ? tail : desc->levels - 1u; // the per-level downsamples end here
	for (uint32_t i = 1; rc == 0 && i <= lastDown; ++i)
		rc = nv::launch_bloom_downsample((hipStream_t)stream, d_bloom, *desc, i);
	if (rc == 0 && tail < desc->levels)
		rc = nv::launch_bloom_tail((hipStream_t)stream, d_bloom, *desc, tail, 2.0f);
	for (int i = (tail < desc->levels ? (int)tail - 1 : (int)desc->levels - 2); rc == 0 && i >= 0; --i)
		rc = nv::launch_bloom_upsample((hipStream_t)stream, d_bloom, *desc, (uint32_t)i, 2.0f);
	return rc;
}

int nv_shade_final_bloom(nv_context* ctx, void* stream, const NvShadeData* shade, const uint32_t* d_gbuffer0, const uint32_t* d_gbuffer1, const float* d_depth,
                         const uint8_t* d_shadow, uint32_t* d_color, uint32_t width, uint32_t height, const uint32_t* d_bloom, const NvBloomDesc* desc)
{
	nv::ShadeFinalBloomArgs a;
	if (fill_shade_args(a, ctx, shade, d_gbuffer0, d_gbuffer1, d_depth, d_shadow, d_color, width, height) != NV_OK || !d_bloom ||
	    !bloom_desc_ok(desc, width, height) || misaligned(d_bloom, 3u))
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	a.bloom = d_bloom + desc->levelOffset[0];
	a.bloomWidth = desc->width;
	a.bloomHeight = desc->height;
	return nv::launch_shade_final((hipStream_t)stream, a, height, persistent_grid(ctx, 8));
}

int nv_visibility_merge(nv_context* ctx, void* stream, uint64_t* d_dst, const uint64_t* const* d_srcs, uint32_t sources, uint32_t width, uint32_t height)
{
	if (!ctx || !d_dst || !d_srcs || sources == 0 || !image_size_ok(width, height) || misaligned(d_dst, 7u))
		return NV_EINVAL;
	for (uint32_t i = 0; i < sources; ++i)
		if (!d_srcs[i] || d_srcs[i] == d_dst || misaligned(d_srcs[i], 7u))
			return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	return nv::launch_visibility_merge((hipStream_t)stream, reinterpret_cast<unsigned long long*>(d_dst),
	                                   reinterpret_cast<const unsigned long long* const*>(d_srcs), sources, width * height, persistent_grid(ctx, 8));
}

#ifdef NV_EXPERIMENTS
// experiments build only: number of library-owned blocks (of every context of this process) whose canary zones no longer hold
// their pattern, after synchronising the device; tests/conftest.py calls it after every GPU test
int nv_debug_check_scratch(void)
{
	if (hipDeviceSynchronize() != hipSuccess)
		return -1;
	GuardLock lock;
	int damaged = 0;
	std::vector<unsigned char> host(2 * NV_GUARD_BYTES);
	for (const GuardedBlock& b : guarded_blocks())
	{
		if (hipMemcpy(host.data(), b.base, NV_GUARD_BYTES, hipMemcpyDeviceToHost) != hipSuccess ||
		    hipMemcpy(host.data() + NV_GUARD_BYTES, b.base + NV_GUARD_BYTES + b.bytes, NV_GUARD_BYTES, hipMemcpyDeviceToHost) != hipSuccess)
			return -1;
		bool ok = true;
		for (unsigned char c : host)
			ok = ok && c == 0xC5;
		damaged += ok ? 0 : 1;
	}
	return damaged;
}
#endif

#ifdef NV_EXPERIMENTS
// experiments build only (not part of the public header): copies the NV_DEBUG_MODE bit-3 wave stamps to the host
int nv_debug_read_timing(nv_context* ctx, unsigned long long* out, uint32_t maxWaves)
{
	if (!ctx || !ctx->timing || !out)
		return NV_EINVAL;
	uint32_t waves = (uint32_t)ctx->timingWaves; // (the caller says how many it wants: the cull launch's, or the occlusion stage's)
	if (waves > maxWaves)
		waves = maxWaves;
	return (int)hipMemcpy(out, ctx->timing, (size_t)waves * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
}
#endif

int nv_set_counts_sink(nv_context* ctx, uint64_t* d_out3)
{
	if (!ctx)
		return NV_EINVAL;
	ctx->countsSink = d_out3;
	return NV_OK;
}

int nv_pack_counts(nv_context* ctx, void* stream, const uint32_t* d_countA, const uint32_t* d_countB,
                   const uint32_t* d_countC, uint64_t* d_out3)
{
	if (!ctx || !d_out3)
		return NV_EINVAL;
	DeviceGuard guard(ctx->device);
	return nv::launch_pack_counts((hipStream_t)stream, d_countA, d_countB, d_countC, d_out3);
}

int nv_probe_cluster_scalars(nv_context* ctx, void* stream, const NvCullData* cull, const NvMeshTaskCommand* d_commands,
                             uint32_t commandCount, const NvMeshDraw* d_draws, const NvMeshlet* d_meshlets,
                             const NvPyramidDesc* pyramid, float* d_out16)
{
	if (!d_out16 || !commandCount)
		return NV_EINVAL;
	nv::ClusterArgs a;
	int rc = fill_cluster_args(ctx, a, cull, 0, d_commands, nullptr, d_draws, d_meshlets, nullptr, pyramid);
	if (rc == NV_EINVAL && cull && cull->clusterOcclusionEnabled == 1)
	{
		// the probe never touches visibility bits
		NvCullData c2 = *cull;
		c2.clusterOcclusionEnabled = 0;
		rc = fill_cluster_args(ctx, a, &c2, 0, d_commands, nullptr, d_draws, d_meshlets, nullptr, pyramid);
		if (rc == NV_OK)
			a.cd = *cull;
	}
	if (rc)
		return rc;
	DeviceGuard guard(ctx->device);
	a.commandCountOverride = commandCount;
	a.probeOut = d_out16;
	return nv::launch_probe((hipStream_t)stream, a, a.soaBounds != nullptr, nv::capped_grid(commandCount, 4, persistent_grid(ctx, 8)));
}

} // extern "C"
