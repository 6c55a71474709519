/*
 * niagara_vis.h — C ABI of the MI355X-native visibility front-end.
 *
 * Drop-in replacement for the compute passes niagara records between its scene
 * upload and its indirect draws:
 *
 *     drawcull -> tasksubmit -> clustercull -> clustersubmit      (+ depthreduce)
 *
 * Every struct below keeps the byte layout of the reference (citations are
 * relative to the reference tree, file:line).  Every entry point names the
 * reference interface it replaces.  All pointers named d_* are DEVICE pointers
 * owned by the caller; the library only owns scratch inside nv_context.
 *
 * Conventions (mirrors SURVEY.md §8b):
 *   - all functions return 0 on success, a negative NV_E* code or a positive
 *     hipError_t otherwise; nothing throws across this boundary;
 *   - work is enqueued asynchronously on the caller's hipStream_t (passed as
 *     void* so this header needs no HIP include);
 *   - the caller zeroes count words before each pass (src/niagara.cpp:1541,1586)
 *     and zeroes drawVisibility / meshletVisibility once (src/niagara.cpp:1450-1468);
 *   - stage ordering == stream order (replaces the Vulkan barriers at
 *     src/niagara.cpp:1561,1571,1601,1610,1725);
 *   - overflow past NV_TASK_WGLIMIT / NV_CLUSTER_LIMIT is dropped silently,
 *     exactly as drawcull.comp.glsl:128 and clustercull.comp.glsl:137 do.
 *
 * Output order.  The reference appends with unordered global atomics; this
 * library appends in ascending invocation order (draw index; command index then
 * lane), which is one valid serialisation of the reference and makes the lists
 * bit-reproducible.
 */
#ifndef NIAGARA_VIS_H
#define NIAGARA_VIS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- compile-time contract (src/config.h:2-28) ---- */
#define NV_TASK_WGSIZE 64u           /* src/config.h:2  */
#define NV_MESH_MAXVTX 64u           /* src/config.h:14 */
#define NV_MESH_MAXTRI 96u           /* src/config.h:15 */
#define NV_CLUSTER_TILE 16u          /* src/config.h:22 */
#define NV_TASK_WGLIMIT (1u << 22)   /* src/config.h:25 */
#define NV_CLUSTER_LIMIT (1u << 24)  /* src/config.h:28 */
#define NV_MAX_LODS 8u               /* src/scene.h:92  */
#define NV_MAX_MIPS 16u              /* sampler maxLod 16: src/resources.cpp:305 */

/* ---- status codes ---- */
#define NV_OK 0
#define NV_EINVAL (-1)   /* bad argument */
#define NV_ENOMEM (-2)   /* scratch allocation failed */
#define NV_ESTATE (-3)   /* reserved (no pass has a device-side protocol any more); never returned */
#define NV_ENODEV (-4)   /* no HIP device */
#define NV_EIO (-5)      /* file cannot be opened / read */
#define NV_EFORMAT (-6)  /* not a scene cache this build understands (magic, version, meshlet limits, truncated) */

/* ---- layouts ---- */

/* src/scene.h:10-23, src/shaders/mesh.h:11-24; 24 B, align 8. cull reads bytes 0-11 only */
typedef struct NvMeshlet
{
	uint16_t center[3]; /* fp16 bits */
	uint16_t radius;    /* fp16 bits */
	int8_t cone_axis[3];
	int8_t cone_cutoff;
	uint32_t dataOffset;
	uint32_t baseVertex;
	uint8_t vertexCount;
	uint8_t triangleCount;
	uint8_t shortRefs;
	uint8_t padding;
} NvMeshlet;

/* src/scene.h:39-49, src/shaders/mesh.h:92-102; 48 B, align 16; orientation is (x,y,z,w) */
typedef struct NvMeshDraw
{
	float position[3];
	float scale;
	float orientation[4];
	uint32_t meshIndex;
	uint32_t meshletVisibilityOffset;
	uint32_t postPass;
	uint32_t materialIndex;
} NvMeshDraw;

/* src/scene.h:51-58; 32 B, align 16 */
typedef struct NvLight
{
	float position[3];
	float range;
	float color[3];
	float intensity;
} NvLight;

/* src/scene.h:119-124; 32 B; rotation is (x,y,z,w) like NvMeshDraw.orientation */
typedef struct NvKeyframe
{
	float translation[3];
	float scale;
	float rotation[4];
} NvKeyframe;

/* src/scene.h:126-136; 24 B.  A negative drawIndex / lightIndex means "no such target" */
typedef struct NvAnimation
{
	int32_t drawIndex;
	int32_t lightIndex;
	float startTime;
	float period;
	uint32_t keyframeOffset;
	uint32_t keyframeCount;
} NvAnimation;

/* src/scene.h:68-75, src/shaders/mesh.h:53-60; 20 B */
typedef struct NvMeshLod
{
	uint32_t indexOffset;
	uint32_t indexCount;
	uint32_t meshletOffset;
	uint32_t meshletCount;
	float error;
} NvMeshLod;

/* src/scene.h:77-93, src/shaders/mesh.h:62-78; 208 B, align 16 */
typedef struct NvMesh
{
	float center[3];
	float radius;
	uint32_t vertexOffset;
	uint32_t vertexCount;
	uint32_t ommIndexData;
	uint32_t ommIndexBase;
	uint32_t lodCount;
	uint32_t lodRT;
	uint32_t padding[2];
	NvMeshLod lods[NV_MAX_LODS];
} NvMesh;

/* src/niagara.cpp:227-231, src/shaders/mesh.h:104-114; 24 B */
typedef struct NvMeshDrawCommand
{
	uint32_t drawId;
	uint32_t indexCount;
	uint32_t instanceCount;
	uint32_t firstIndex;
	uint32_t vertexOffset;
	uint32_t firstInstance;
} NvMeshDrawCommand;

/* src/niagara.cpp:233-240, src/shaders/mesh.h:116-123; 20 B */
typedef struct NvMeshTaskCommand
{
	uint32_t drawId;
	uint32_t taskOffset;
	uint32_t taskCount;
	uint32_t lateDrawVisibility;
	uint32_t meshletVisibilityOffset;
} NvMeshTaskCommand;

/* src/niagara.cpp:242-260, src/shaders/mesh.h:26-44; 144 B (136 used), align 16.
 * view is column-major: view[4*col + row]. */
typedef struct NvCullData
{
	float view[16];
	float P00, P11, znear, zfar;
	float frustum[4];
	float lodTarget;
	float pyramidWidth, pyramidHeight;
	uint32_t drawCount;
	int32_t cullingEnabled;
	int32_t lodEnabled;
	int32_t occlusionEnabled;
	int32_t clusterOcclusionEnabled;
	int32_t clusterBackfaceEnabled;
	uint32_t postPass;
	uint32_t _pad[2];
} NvCullData;

/* Replaces the (depthPyramid image, depthSampler) descriptor pair
 * (src/niagara.cpp:1339-1350 image + per-mip views; src/niagara.cpp:629 sampler =
 * LINEAR filter, NEAREST mip, CLAMP_TO_EDGE, MIN reduction).  The mip chain is one
 * linear fp32 buffer; level i is max(1,width>>i) x max(1,height>>i), row-major, at
 * d_base + mipOffset[i] (offsets in floats). */
typedef struct NvPyramidDesc
{
	float* d_base;
	uint32_t width;   /* level-0 width  = previousPow2(depth target width)  */
	uint32_t height;  /* level-0 height = previousPow2(depth target height) */
	uint32_t levels;  /* getImageMipLevels(width, height), src/resources.cpp:280-292 */
	uint32_t mipOffset[NV_MAX_MIPS];
	uint32_t totalTexels;
} NvPyramidDesc;

typedef struct nv_context nv_context;

/* ---- lifetime (replaces createProgram/createComputePipeline, src/niagara.cpp:652-762) ---- */
int nv_create(nv_context** out_ctx, int device);
void nv_destroy(nv_context* ctx);
const char* nv_version(void);
/* Synchronises the stream and returns its state: NV_OK or the HIP error.  (The library has no inter-workgroup waits
 * and therefore no device-side error word any more; NV_ESTATE is kept for ABI stability.) */
int nv_status(nv_context* ctx, void* stream);

/* Kernel-level timing with HIP events recorded on the launch stream (replaces the vkCmdWriteTimestamp pairs around
 * each pass, src/niagara.cpp:1537,1573,1705,1732).  While enabled, nv_clustercull brackets its cull kernel, its
 * occlusion stage (late pass) and its scatter kernel, nv_drawcull and nv_depthreduce their launches.  nv_profile_read synchronises the recorded events,
 * returns the accumulated milliseconds and launch count per slot and resets the accumulators. */
#define NV_PROF_CLUSTER_CULL 0
#define NV_PROF_CLUSTER_SCATTER 1
#define NV_PROF_DRAWCULL 2
#define NV_PROF_DEPTHREDUCE 3
#define NV_PROF_CLUSTER_HIZ 4 /* late pass with HiZ: the occlusion stage between the cull and the scatter kernel */
#define NV_PROF_SLOTS 5
int nv_profile_enable(nv_context* ctx, int enabled);
int nv_profile_read(nv_context* ctx, float out_ms[NV_PROF_SLOTS], uint32_t out_count[NV_PROF_SLOTS]);
/* Which kernel variant the passes took since the last call (the host picks per launch from the previous launches' statistics, or
 * what NV_OPT_CULL_FORM / NV_OPT_CULL_RING / NV_OPT_TASK_EMIT pin): launch counts per variant, so that a profile can say what it
 * timed.  Counted whether or not event profiling is enabled; reading resets the counts. */
#define NV_VARIANT_CULL_FILTER_RING4 0 /* cluster cull launch: conservative filter pass + certified pass, 4-deep ring */
#define NV_VARIANT_CULL_FILTER_RING8 1 /* the same with the 8-deep ring */
#define NV_VARIANT_CULL_DIRECT 2       /* no filter pass, one command per wave */
#define NV_VARIANT_CULL_LANES_BITS 3   /* early pass, one lane per set visibility bit */
#define NV_VARIANT_CULL_LANES 4        /* (0.3: early pass over a cache-resident pool, one lane per valid cluster; never chosen since 0.4) */
#define NV_VARIANT_CULL_AOS 5          /* no SoA mirror registered for the meshlet buffer: records read in place */
#define NV_VARIANT_HIZ_STAGE 6         /* late pass with HiZ: occlusion-stage launches */
#define NV_VARIANT_TASK_LIST 7         /* drawcull TASK scatter: one lane per output command */
#define NV_VARIANT_TASK_PER_DRAW 8     /* drawcull TASK scatter: per-draw form */
#define NV_VARIANT_CULL_DIRECT_PACKED 9 /* no filter pass, windows of 64 valid meshlets per wave iteration (early form without visibility bits) */
#define NV_VARIANT_SLOTS 10
int nv_profile_variants(nv_context* ctx, uint32_t out_count[NV_VARIANT_SLOTS]);

/* ---- options ----
 * NV_OPT_FUSED_COUNT_RESET (default 0): when 1, nv_drawcull and nv_clustercull start their append at index 0 whatever
 * the count word holds, i.e. they absorb the caller's vkCmdFillBuffer(count, 0, 4, 0) (src/niagara.cpp:1541,1586) and
 * the launch boundary that goes with it.  With 0 the reference contract holds: the append starts at the value found in
 * the count word, which the caller zeroes (nv_reset_count or any memset). */
#define NV_OPT_FUSED_COUNT_RESET 1
/* NV_OPT_FUSED_SUBMIT (default 0): when 1, nv_drawcull (task = 1) also leaves what tasksubmit.comp.glsl:27-47 writes — the
 * {X, 64, 1} dispatch words and the zeroed dummy commands up to the next multiple of 64 — and nv_clustercull what
 * clustersubmit.comp.glsl:25-45 writes (the {16, Y, 16} words and the ~0 padding up to the next multiple of 256): the
 * last workgroup of their scatter launches knows the final count.  nv_tasksubmit / nv_clustersubmit can then be
 * skipped (calling them anyway is harmless: they are idempotent); two launches less per frame phase. */
#define NV_OPT_FUSED_SUBMIT 2
/* NV_OPT_CULL_WORKGROUPS_PER_CU (default 6, 1..8): workgroups per CU of nv_clustercull's cull launch.  6 fill a CU and give
 * one pass its shortest time; a caller that keeps several independent passes in flight (contexts on different streams:
 * the cluster passes of several views) gets more throughput from 3, which let two passes' cull launches share the chip
 * (10 M meshlets, three passes in flight: 23.5 instead of 24.7 us per pass; a single pass: 26.3 instead of 25.0 us).
 * Speed only: the results do not depend on it. */
#define NV_OPT_CULL_WORKGROUPS_PER_CU 3
/* NV_OPT_SCATTER_WAVES (default 16; 4 or 8): waves per workgroup of nv_clustercull's scatter launch.  16 (one command per
 * lane) is the shortest launch; 4 leave the other wave slots of every CU to a neighbour pass's cull launch when several
 * passes are in flight (10 M meshlets, three passes in flight: 23.3 instead of 24.8 us per pass; a single pass: 31.5
 * instead of 30.1 us).  Speed only. */
#define NV_OPT_SCATTER_WAVES 4
/* NV_OPT_CULL_FORM (default 0) and NV_OPT_CULL_RING (default 0): pin what nv_clustercull otherwise chooses per launch from two
 * words the PREVIOUS launches of the context left in mapped host memory (frame coherence; read unsynchronised — possibly a launch
 * or two behind).  Results never depend on the choice, speed does, and a captured HIP graph freezes whatever the capture saw;
 * a caller that replays graphs, or wants run-to-run identical timing, pins it:
 *   NV_OPT_CULL_FORM  0 = by statistic (direct form when more than 35 % of the last launch's commands passed the frustum filter),
 *                     1 = always the filter form (sparse passes: few commands have survivors),
 *                     2 = always the direct form (dense passes: the commands of draws drawcull already found visible); an early
 *                         pass with visibility bits then tests one lane per SET BIT (last frame's visible clusters) instead of
 *                         one wave per command,
 *                     3 = as 2, but one wave per command also in the early pass with visibility bits;
 *                     4 = as 3, and one command per wave iteration also where the direct form would walk packed windows of 64 valid
 *                         meshlets (early form without visibility bits: the cluster pass behind drawcull's LOD select, the late pass's
 *                         first stage);
 *                     5 = as 2, but the early pass with visibility bits walks packed windows too (the valid meshlets of the commands that have a
 *                         set bit) instead of testing one lane per set bit;
 *   NV_OPT_CULL_RING  0 = by the last launch's command count, 4 = the 4-deep load ring (passes of a few hundred thousand commands),
 *                     8 = the 8-deep ring (long streams, late passes). */
#define NV_OPT_CULL_FORM 5
#define NV_OPT_CULL_RING 6
/* NV_OPT_TASK_EMIT (default 0): likewise the form in which nv_drawcull (task = 1) writes its MeshTaskCommands — 0 = by the statistic
 * of earlier task passes (list form once a pass emitted more than 4 commands per emitting draw), 1 = always per draw (every lane
 * writes its own draws' commands; fastest for meshes of one or two task groups), 2 = always the list form (one lane per output
 * command; fastest for meshes of many task groups).  Speed only. */
#define NV_OPT_TASK_EMIT 7
/* NV_OPT_DRAW_RECORDS (default 0): the order in which nv_drawcull's EARLY pass requests its inputs — 0 = by the statistic of the last
 * task pass (visibility words first once it emitted from fewer than one draw in eight), 1 = always the records together with the
 * visibility words, 2 = always the visibility words first and then only the records of last frame's visible draws (the others leave
 * at drawcull.comp.glsl:66 whatever their record holds).  Speed only; the late pass decides every draw and reads every record. */
#define NV_OPT_DRAW_RECORDS 8
/* NV_OPT_RASTER_SMALL_LIMIT (default 16, 0 .. INT_MAX): nv_rasterdepth walks a triangle whose clipped bounding box holds at most this
 * many pixel centres with one lane, a larger one with the whole wave (lane = pixel of an 8 x 8 stamp).  0 puts every triangle on the
 * wave path, INT_MAX every triangle on the lane path.  Speed only: both paths write the same bits. */
#define NV_OPT_RASTER_SMALL_LIMIT 9
/* NV_OPT_RASTER_NEAR_CLIP (default 0; 0 / 1, anything else NV_EINVAL): 1 makes nv_rasterdepth and nv_rasterdepth_indexed clip a triangle
 * that crosses the near plane instead of dropping it.  A triangle with one or two vertices that fail clip.w > 0 && clip.z <= clip.w is cut
 * at d = clip.w - clip.z = 0 into one or two pieces (the fan of the Sutherland-Hodgman polygon over the edges v0->v1, v1->v2, v2->v0),
 * provided all twelve clip components are finite and every failing vertex has d < 0; otherwise it is not drawn, as with 0.  A new vertex is
 * computed from the edge's inside end I towards its outside end O whatever the edge's direction (t = dI / (dI - dO); x, y, w = I + t (O - I),
 * fp32, no contraction), so two triangles sharing the edge get the same bits and a mesh stays watertight; its depth is exactly 1.  A new
 * vertex with w <= 0, a non-finite screen position or one at or past 2^21 pixels rejects the whole triangle.  There is NO clipping
 * against the guard band or the viewport: such a triangle still does not occlude, which is conservative.  Each piece is rasterised as a
 * triangle of its own (facing by its own area, top-left rule: a sample of the polygon belongs to exactly one piece).  Totals word 2 then
 * counts pieces; the visibility word of a piece carries the original triangle's id.  With 0 both entry points write the bits they
 * wrote before the option existed.  Not speed only: with 1 more samples are written. */
#define NV_OPT_RASTER_NEAR_CLIP 10
/* NV_OPT_RASTER_VISIBILITY_ID (default 0; 0 / 1, anything else NV_EINVAL): the form of the word nv_rasterdepth writes into d_visibility.
 *   0 = bits(z) << 32 | slot << 7 | triangle, slot being the position in THIS launch's cluster list: a name that holds until the list is
 *       overwritten, i.e. for one pass of one context.  The bits the entry point wrote before the option existed.
 *   1 = the stable form, bits(z) << 34 | id34 with id34 = ((mvi << 7) | triangle) + 1 and mvi = command.meshletVisibilityOffset + lane,
 *       the cluster's meshlet-visibility bit index (lane = the cluster-list entry >> 24).  mvi depends on the draw and its LOD only — not on
 *       the pass, the list or, in a frame sharded by draws, the rank — so the early, late and post rasters of a frame can share one
 *       target, the targets of several ranks composite with an unsigned 64-bit maximum (nv_visibility_merge), and
 *       nv_visibility_resolve turns the word back into {draw, meshlet, triangle}.  z is clamped to [0, 1] with NaN -> 0 before it is
 *       written, so bits(z) <= 0x3F800000 < 2^30 and the shift by 34 loses nothing; the order is depth first, id second, ties still go to
 *       the larger id; 0 means "no sample" (hence the + 1).  A cluster with mvi >= 2^27 - 1 cannot be named in 34 bits: its samples write
 *       depth as always and NO visibility word (dropping is conservative, as with the list limits).  With NV_OPT_RASTER_NEAR_CLIP 1 both
 *       pieces of a triangle carry its id, as with 0.
 * The depth target, the totals and a launch without d_visibility do not depend on the option. */
#define NV_OPT_RASTER_VISIBILITY_ID 11
/* NV_OPT_BLOOM_FUSED_TAIL (default 0; 0 / 1, anything else NV_EINVAL): 1 = nv_bloom runs the small end of its chain — every level from the
 * first one behind which the rest holds at most 5376 texels — as ONE launch of one workgroup out of LDS instead of one launch per pass
 * (DESIGN.md §4.15).  The words written are the same at every level; the option changes launches only.  Off until an A/B on the device
 * (tools/ab.sh -b) shows it faster than the per-level chain. */
#define NV_OPT_BLOOM_FUSED_TAIL 12
int nv_set_option(nv_context* ctx, int option, int value);

/* ---- capacities ----
 * The pass entry points only enqueue: none of them allocates, frees or synchronises, so all of them can be recorded into a
 * HIP graph (stream capture) with growing arguments.  nv_create sizes the library's scratch for 1 M draws and
 * NV_TASK_WGLIMIT task commands (the size niagara allocates dcb for, src/niagara.cpp:1070); nv_reserve raises the
 * per-draw scratch to maxDraws before the first pass over that many (it may synchronise the device: call it at scene
 * load, next to createBuffer(dvb), src/niagara.cpp:1060); per draw that is about 17 B for nv_drawcull and 4 B for nv_rasterdepth_indexed (+ 20 KiB
 * fixed).  nv_drawcull or nv_rasterdepth_indexed over more draws than were reserved returns
 * NV_ENOMEM and enqueues nothing.  maxCommands is accepted for symmetry; values above NV_TASK_WGLIMIT buy nothing (the
 * passes clamp there like the shaders do). */
int nv_reserve(nv_context* ctx, uint32_t maxDraws, uint32_t maxCommands);

/* Several contexts of ONE device (one per stream: several views or frames in flight) can use one set of scene mirrors:
 * after nv_share_scene(dst, src) the two contexts share what nv_upload_meshlets / nv_upload_meshes / nv_upload_draws /
 * nv_update_draws built or build from then on through either of them (reference-counted; dst's previous mirrors are
 * released; destroying one context leaves the other's mirrors alone).  Scratch (ballots, tile counts, result bytes)
 * stays per context.  An upload through one context is ordered on THAT call's stream only: the caller orders it
 * against passes the sharing contexts have in flight on other streams, as it would for its own buffer uploads. */
int nv_share_scene(nv_context* dst, nv_context* src);

/* ---- scene upload hook (next to uploadBuffer(mlb), src/niagara.cpp:1055) ----
 * Builds the library-owned SoA mirror of the 12 cull bytes of every meshlet
 * (bounds: 4 x fp16 = 8 B, cone: 4 x s8 = 4 B).  nv_clustercull uses the mirror when
 * its d_meshlets argument equals the pointer registered here, and reads the 24-B AoS
 * records directly otherwise.  The registration is by device pointer and the mirror is a
 * snapshot: call again after the buffer's contents change, and before the allocation is
 * freed or reused for something else — (NULL, 0) drops the registration (likewise for
 * nv_upload_meshes).  A re-upload must be ORDERED against the passes in flight over the old
 * contents (same stream, or the caller's event): next to the mirror it rewrites the pool's
 * largest |centre component| / |radius|, which the cull launch's filter margins are derived
 * from — a pass that pairs new records with the old bounds is no longer conservative (only
 * the capacity-growth path synchronises the device by itself). */
int nv_upload_meshlets(nv_context* ctx, void* stream, const NvMeshlet* d_meshlets, uint32_t meshletCount);
/* Test-only accessor: copies the block table nv_upload_meshlets builds next to the mirror (one 16-B record per 64 meshlets of the
 * mirror, the padding block included: {centre xyz as fp32, D | rho << 16 as fp16 bits}) to host memory, at most
 * maxRecords of them; *out_records = the table's length (0 without a mirror).  Synchronises the device. */
int nv_debug_block_table(nv_context* ctx, void* hostOut, uint32_t maxRecords, uint32_t* out_records);

/* Upload hook next to uploadBuffer(mb) (src/niagara.cpp:1049): registers the Mesh table's pointer and size.  nv_drawcull
 * stages a registered table of <= 64 meshes in LDS (every draw reads its mesh's bounds, LOD errors and LOD range);
 * unregistered or larger tables are gathered from global memory.  The table is only read at pass time. */
int nv_upload_meshes(nv_context* ctx, void* stream, const NvMesh* d_meshes, uint32_t meshCount);

/* Upload hook next to uploadBuffer(db) (src/niagara.cpp:1052): builds the library-owned mirror of what a draw decision
 * reads.  Everything drawcull.comp.glsl:73-75 computes BEFORE the view transform is view-independent — the world-space
 * sphere {rotateQuat(mesh.center, orientation) * scale + position, mesh.radius * scale} — so it is evaluated once here, in
 * the reference's operation order (the intermediates are bit-identical), and stored as a 16-B stream next to
 * {scale, meshIndex} (8 B) and postPass (4 B).  The decide kernel of nv_drawcull then reads three coalesced streams
 * (28 B per draw instead of 48-B-stride records plus a Mesh gather) and is left with the view transform and the tests.
 * Used when nv_drawcull's d_draws is the pointer registered here or a record inside that buffer with drawCount records
 * behind it (a pass over a shard of the draws) AND its d_meshes is the table given here; the 48-B AoS records are read
 * in place otherwise (same results).  Same registration contract as nv_upload_meshlets ((NULL, 0, NULL) drops it); call
 * again when the Mesh table's bounds change.
 * nv_update_draws re-evaluates [first, first + count) after the caller rewrote those records — the animation path,
 * src/niagara.cpp:1385-1391, which memcpy()s single MeshDraws into the mapped draw buffer every frame. */
int nv_upload_draws(nv_context* ctx, void* stream, const NvMeshDraw* d_draws, uint32_t drawCount, const NvMesh* d_meshes);
int nv_update_draws(nv_context* ctx, void* stream, const NvMeshDraw* d_draws, uint32_t first, uint32_t count);

/* ---- the passes ---- */

/* drawcull.comp.glsl:54-156; dispatch at src/niagara.cpp:1548-1556.
 * late/task are the LATE/TASK specialisation constants (src/niagara.cpp:724-727).
 * d_commands: NvMeshTaskCommand[NV_TASK_WGLIMIT] if task else NvMeshDrawCommand[drawCount].
 * d_count4: {commandCount, groupCountX, groupCountY, groupCountZ} (dccb).
 * pyramid may be NULL unless late && occlusionEnabled. */
int nv_drawcull(nv_context* ctx, void* stream, const NvCullData* cull, int late, int task,
                const NvMeshDraw* d_draws, const NvMesh* d_meshes, void* d_commands, uint32_t* d_count4,
                uint32_t* d_drawVisibility, const NvPyramidDesc* pyramid);

/* vkCmdFillBuffer(dccb / ccb, 0, 4, 0) in front of a pass (src/niagara.cpp:1541,1586): zeroes word 0 of one or two count
 * buffers (either may be NULL).  The passes themselves never clear a counter. */
int nv_reset_count(nv_context* ctx, void* stream, uint32_t* d_count4a, uint32_t* d_count4b);

/* tasksubmit.comp.glsl:27-47; dispatch at src/niagara.cpp:1563-1568 */
int nv_tasksubmit(nv_context* ctx, void* stream, uint32_t* d_count4, NvMeshTaskCommand* d_commands);

/* clustercull.comp.glsl:56-149; indirect dispatch at src/niagara.cpp:1590-1599.
 * The grid is taken on-device from d_count4[1] (groupCountX written by nv_tasksubmit):
 * commands [0, groupCountX*64) are processed, like vkCmdDispatchIndirect(dccb, 4). */
int nv_clustercull(nv_context* ctx, void* stream, const NvCullData* cull, int late,
                   const NvMeshTaskCommand* d_commands, const uint32_t* d_count4, const NvMeshDraw* d_draws,
                   const NvMeshlet* d_meshlets, uint32_t* d_meshletVisibility, const NvPyramidDesc* pyramid,
                   uint32_t* d_clusterIndices, uint32_t* d_clusterCount4);

/* clustersubmit.comp.glsl:25-45; dispatch at src/niagara.cpp:1603-1608 */
int nv_clustersubmit(nv_context* ctx, void* stream, uint32_t* d_clusterCount4, uint32_t* d_clusterIndices);

/* meshlet.task.glsl:53-149 (cull half): same tests as nv_clustercull but compacted per
 * task command into a 64-entry payload, d_payloadCounts[c] = EmitMeshTasksEXT count. */
int nv_taskcull(nv_context* ctx, void* stream, const NvCullData* cull, int late,
                const NvMeshTaskCommand* d_commands, const uint32_t* d_count4, const NvMeshDraw* d_draws,
                const NvMeshlet* d_meshlets, uint32_t* d_meshletVisibility, const NvPyramidDesc* pyramid,
                uint32_t* d_payloads, uint32_t* d_payloadCounts);

/* ---- downstream decode ----
 * What the mesh stage does with the lists before it touches a vertex (src/shaders/meshlet.mesh.glsl:91-116): the indirect
 * grid {16, Y, 16} written by nv_clustersubmit is walked as index = x + 256 y + 16 z, the entry is decoded
 * (~0 = padding -> no outputs; else command = ci & 0xffffff, meshlet = command.taskOffset + (ci >> 24)) and the meshlet
 * header is read.  One 32-byte record per index in [0, 256 Y) and three 64-bit totals (accumulated: zero them first). */
typedef struct NvClusterRecord
{
	uint32_t drawId;       /* ~0 for a padding entry */
	uint32_t meshletIndex; /* mi */
	uint32_t vertexCount, triangleCount; /* SetMeshOutputsEXT arguments */
	uint32_t vertexOffset; /* = dataOffset */
	uint32_t indexOffset;  /* dataOffset + (shortRefs ? (vertexCount + 1) / 2 : vertexCount) */
	uint32_t baseVertex;
	uint32_t shortRefs;
} NvClusterRecord;
int nv_cluster_expand(nv_context* ctx, void* stream, const NvMeshTaskCommand* d_commands, const NvMeshlet* d_meshlets,
                      const uint32_t* d_clusterIndices, const uint32_t* d_clusterCount4, NvClusterRecord* d_records,
                      uint32_t recordCapacity, uint64_t* d_totals3 /* clusters, vertices, triangles */);

/* ---- triangle cull of the mesh stage ----
 * src/shaders/meshlet.mesh.glsl:91-198 with MESH_CULL = 1 (src/config.h:10-11; the reference ships it switched off): for
 * every slot of the consumer's grid the meshlet's vertices are transformed exactly like the mesh shader does
 * (rotateQuat * scale + position, view, projection, perspective divide to screen space) and every triangle gets the
 * shader's gl_CullPrimitiveEXT decision: back-facing / zero-area (:176-181) or missing every sample centre (:183-190),
 * provided all three vertices are in front of the perspective plane (:192-193).
 * One NvTriangleMask per slot index in [0, 256 Y): keep bit i = triangle i is NOT culled (i < triangleCount);
 * counts = triangleCount | vertexCount << 8 | kept << 16; all zero for a padding slot (~0).  Totals are accumulated
 * (zero them first): clusters, triangles, triangles kept. */
typedef struct NvVertex /* src/shaders/mesh.h:3-9, 16 bytes */
{
	uint16_t vx, vy, vz; /* fp16 position */
	uint16_t tp;         /* packed tangent */
	uint32_t np;         /* packed normal */
	uint16_t tu, tv;     /* fp16 texcoord */
} NvVertex;
typedef struct NvGlobals /* src/shaders/mesh.h:46-51, the mesh pipeline's push constants */
{
	float projection[16]; /* column-major */
	NvCullData cullData;  /* only .view is read here */
	float screenWidth, screenHeight;
	float pad_[2];
} NvGlobals;
typedef struct NvTriangleMask
{
	uint32_t keep[3]; /* MESH_MAXTRI = 96 (src/config.h:15) */
	uint32_t counts;
} NvTriangleMask;
/* SURVEY.md §8(f) N2 — meshlet bounds (src/scene.cpp:69-85: meshopt_computeMeshletBounds, meshopt_quantizeHalf,
 * cone_axis_s8 / cone_cutoff_s8).  For every Meshlet of d_meshlets[0, meshletCount) — dataOffset, baseVertex, vertexCount,
 * triangleCount and shortRefs filled in by the caller, the payload in d_meshletData as src/scene.cpp:24-47 packs it, the
 * fp16 positions in d_vertices — computes the bounding sphere and the normal cone of its triangles and writes center[3],
 * radius (fp16) and cone_axis[3], cone_cutoff (s8) into the record (bytes 0-11; the rest is left alone).  d_bounds8
 * (optional) receives the unquantised {center.xyz, radius, axis.xyz, cutoff} per meshlet.  Call nv_upload_meshlets
 * afterwards (a mirror built from these records before is dropped).
 * PARITY UNPINNED: the arithmetic is meshoptimizer's, which the reference does not vendor; the library's published
 * algorithm is restated with defined fp32 semantics here and in the CPU oracle (orc_meshlet_bounds), and the two agree bit for bit.
 * Defined for any input: vertexCount / triangleCount above 64 / 96 are clamped, and the index bytes start where the
 * clamped vertex count puts them; an index byte is masked with 63, a slot at or above vertexCount is the point (0, 0, 0); shortRefs == 1
 * means 16-bit references, every other value 32-bit ones; x < NaN is false, so a NaN coordinate is never an extreme (unless it is the
 * first point) and never outside the sphere; cone_cutoff = q < 127 ? (int)q : 127 with q = 127 (cutoff + e) + 1, so a NaN (non-finite
 * vertices) gives 127, no cone culling; a NaN among the eight results is the quiet NaN 0x7fc00000 in d_bounds8 and 0x7e00 in the record.
 * The caller keeps every reference (baseVertex + reference < vertices, dataOffset and the payload inside d_meshletData) in bounds. */
int nv_meshlet_bounds(nv_context* ctx, void* stream, const NvVertex* d_vertices, const uint32_t* d_meshletData, NvMeshlet* d_meshlets,
                      uint32_t meshletCount, float* d_bounds8);

/* Buffer sizes: d_meshletData must hold at least one word and d_vertices at least one record even when every slot of d_clusterIndices is ~0 —
 * the lanes of a pass that have no vertex / triangle to fetch read element 0 of both (unconditional loads: no branch between a load and its
 * use), which the reference's mesh shader never touches for an empty slot. */
int nv_trianglecull(nv_context* ctx, void* stream, const NvGlobals* globals, const NvMeshTaskCommand* d_commands,
                    const NvMeshDraw* d_draws, const NvMeshlet* d_meshlets, const uint32_t* d_meshletData,
                    const NvVertex* d_vertices, const uint32_t* d_clusterIndices, const uint32_t* d_clusterCount4,
                    NvTriangleMask* d_masks, uint32_t maskCapacity, uint64_t* d_totals3 /* clusters, triangles, kept */);

/* ---- depth-only raster of the visible clusters ----
 * The [raster] box of niagara's frame (src/niagara.cpp:1765-1788) for a part without a graphics pipeline.  Inputs are nv_trianglecull's;
 * for every slot of the grid {cc4[1], cc4[2], cc4[3]} (index = x + 256 y + NV_CLUSTER_TILE z, ~0 = padding) the meshlet's vertices go to
 * screen space with nv_trianglecull's arithmetic plus z = clip.z / clip.w, snap to 8 sub-pixel bits (X = rint(sx * 256),
 * Y = height * 256 - rint(sy * 256): row 0 at the top, the reference's flipped viewport, src/niagara.cpp:1641) and every triangle
 * i < min(triangleCount, 96) is rasterised at pixel centres with the top-left rule, unless
 *   - an index byte is >= min(vertexCount, 64), or a vertex has !(clip.w > 0 && clip.z <= clip.w) (no near-plane clipping by default:
 *     such a triangle writes nothing, which keeps the pyramid conservative; NV_OPT_RASTER_NEAR_CLIP 1 clips it into one or two pieces
 *     instead, see the option), a non-finite screen position or |sx|, |sy| >= 2^21;
 *   - its doubled area is 0, or it is a back face while globals->cullData.postPass == 0 (front = counter-clockwise in y-up space,
 *     VK_CULL_MODE_BACK_BIT; postPass != 0 draws both faces; the post pass's depth bias is not modelled).
 * Depth: fp32, interpolated in a fixed order from the exact int64 edge functions, clamped to [0, 1], written with an atomic max on its
 * bits (reverse-Z, compare GREATER).  d_depth is width x height; the caller clears it (0 = far) before an early pass, not before a late
 * one.  d_visibility (optional, width x height u64) receives the max of bits(z) << 32 | slot index << 7 | triangle: ties go to the larger ID
 * (NV_OPT_RASTER_VISIBILITY_ID 1: of the stable form bits(z) << 34 | ((mvi << 7 | triangle) + 1), which names the cluster for the whole frame).
 * d_totals4 (optional, accumulated: zero it first): clusters, triangles (triangleCount as stored), triangles rasterised (with
 * NV_OPT_RASTER_NEAR_CLIP 1: pieces rasterised; both pieces of a triangle write its id into d_visibility), samples covered.
 * Every result is independent of the order of the GPU's work.  width and height must equal globals->screenWidth / screenHeight and lie in
 * 1 .. 16384. */
int nv_rasterdepth(nv_context* ctx, void* stream, const NvGlobals* globals, const NvMeshTaskCommand* d_commands,
                   const NvMeshDraw* d_draws, const NvMeshlet* d_meshlets, const uint32_t* d_meshletData,
                   const NvVertex* d_vertices, const uint32_t* d_clusterIndices, const uint32_t* d_clusterCount4,
                   float* d_depth, uint32_t width, uint32_t height,
                   uint64_t* d_visibility /* optional, width*height */, uint64_t* d_totals4 /* optional */);

/* ---- depth-only raster of the indexed draws ----
 * The classic branch of niagara's render() (src/niagara.cpp:1680-1694: vkCmdDrawIndexedIndirectCount(dcb, dccb, maxDrawCount) through
 * mesh.vert.glsl:39-63) on a part without a graphics pipeline: the MeshDrawCommands nv_drawcull(task = 0) writes (drawcull.comp.glsl:141-151).
 * Commands i < min(d_count[0], drawCount) are read on the device, like the indirect count; command i is skipped when its instanceCount is 0
 * or its drawId >= drawCount (instanceCount > 1 writes the same depth as 1; firstInstance is not read).  Its triangle t < indexCount / 3
 * (remainder indices are ignored) has the corners d_indices[firstIndex + 3t + k] + vertexOffset (mod 2^32, the index arithmetic in 64 bits)
 * under the transform d_draws[drawId]; the triangle is skipped, and not counted as rasterised, when an index position is >= indexCapacity or
 * a corner is >= vertexCapacity (0xFFFFFFFF included: there is no primitive restart), so every load stays inside the caller's buffers.
 * Everything else is nv_rasterdepth's rule set, unchanged — the vertex stage, the snap, the near-plane / non-finite / guard-band rejection,
 * facing by globals->cullData.postPass, top-left coverage, the fixed-order fp32 depth and the atomic max — so the same triangle under the same
 * draw writes the same bits through either entry point, with NV_OPT_RASTER_NEAR_CLIP 1 as well (the same clip rule, totals word 2 then counts
 * pieces).  This entry point writes no visibility buffer; nv_rasterdepth_indexed_visibility (below) does.
 * d_totals4 (optional, accumulated: zero it first): commands drawn, triangles (sum of their indexCount / 3), triangles rasterised, samples
 * covered.  d_draws holds drawCount records and d_commands up to drawCount commands; a zero capacity is allowed (nothing is read then).
 * Scratch: 4 B per command slot (drawCount) + 20 KiB, sized by nv_create for 1 M and by nv_reserve(maxDraws); a larger drawCount returns
 * NV_ENOMEM.  width and height must equal globals->screenWidth / screenHeight and lie in 1 .. 16384. */
int nv_rasterdepth_indexed(nv_context* ctx, void* stream, const NvGlobals* globals, const NvMeshDrawCommand* d_commands,
                           const uint32_t* d_count /* dccb: word 0 */, const NvMeshDraw* d_draws,
                           uint32_t drawCount /* = maxDrawCount, src/niagara.cpp:1693 */, const uint32_t* d_indices, uint32_t indexCapacity,
                           const NvVertex* d_vertices, uint32_t vertexCapacity, float* d_depth, uint32_t width, uint32_t height,
                           uint64_t* d_totals4 /* optional */);

/* ---- the visibility buffer of the indexed draws ----
 * A triangle t of draw d is named tri34 = offsets[d] + t, offsets being the prefix nv_assign_triangle_offsets (host helpers, below) takes over
 * the draws' widest LODs: like the cluster path's meshlet-visibility index the name depends on the draw only, not on the pass, the LOD that
 * was selected, the command slot or the rank of a sharded frame.
 *
 * nv_rasterdepth_indexed_visibility is nv_rasterdepth_indexed — the same arguments, rule set, skip rules, totals and NV_OPT_RASTER_NEAR_CLIP,
 * the same depth bits — and every covered sample also takes the atomic maximum of bits(z) << 34 | (tri34 + 1) into d_visibility (width * height
 * words, 8-byte aligned; the caller clears it; 0 = no sample), with tri34 = d_triangleOffsets[command.drawId] + t.  z is the clamped depth
 * that was written, so ties in depth go to the larger id; both pieces of a clipped triangle carry the triangle's id.  A triangle with
 * tri34 >= d_triangleOffsets[drawId + 1] or tri34 >= 2^34 - 1 writes depth as always and no word.  The word is always this stable form:
 * NV_OPT_RASTER_VISIBILITY_ID is not read.  d_triangleOffsets holds drawCount + 1 entries (8-byte aligned).  On a rank of a sharded frame
 * the commands' drawId is rank-local: pass the FULL array's pointer advanced by the rank's first draw — the values stay global, so every
 * rank writes the same word for the same sample and nv_visibility_merge composites the targets.  NV_EINVAL as nv_rasterdepth_indexed, and
 * for a NULL or misaligned d_triangleOffsets or d_visibility. */
int nv_rasterdepth_indexed_visibility(nv_context* ctx, void* stream, const NvGlobals* globals, const NvMeshDrawCommand* d_commands,
                                      const uint32_t* d_count /* dccb: word 0 */, const NvMeshDraw* d_draws, uint32_t drawCount,
                                      const uint32_t* d_indices, uint32_t indexCapacity, const NvVertex* d_vertices, uint32_t vertexCapacity,
                                      float* d_depth, uint32_t width, uint32_t height, uint64_t* d_totals4 /* optional */,
                                      const uint64_t* d_triangleOffsets /* drawCount + 1 */, uint64_t* d_visibility /* width*height */);

/* One resolved pixel of nv_visibility_resolve_indexed.  No sample: {0xFFFFFFFF, 0, 0, 0}.  Unresolved: all four words 0xFFFFFFFF. */
typedef struct NvVisIndexedRecord
{
	uint32_t drawId;        /* index into the d_draws the call was given (the full array: global ids in a sharded frame) */
	uint32_t indexPosition; /* position of the triangle's first index in the index buffer: corners at indexPosition + 0 .. 2 */
	uint32_t vertexOffset;  /* added to each index (mod 2^32), the mesh's vertexOffset */
	uint32_t depthBits;     /* bits of the fp32 depth of the sample */
} NvVisIndexedRecord;

/* nv_visibility_resolve_indexed: per pixel with a non-zero word of nv_rasterdepth_indexed_visibility's width x height target
 *   tri34 = (word & (2^34 - 1)) - 1, depthBits = word >> 34;
 *   drawId = the largest d < drawCount with d_triangleOffsets[d] <= tri34 (non-decreasing in d; pass the FULL arrays, also on a rank);
 *   t      = tri34 - d_triangleOffsets[drawId];
 *   lod    = what nv_drawcull selects for that draw under `cull` (as nv_visibility_resolve: pass the CullData of the rasterised frame);
 *   indexPosition = lods[lod].indexOffset + 3 t (in 64 bits), vertexOffset = mesh.vertexOffset: what drawcull.comp.glsl:145-150 puts into
 *            the draw's command.
 * The pixel is UNRESOLVED — its record all ones, counted, nothing else written — when the id field is 0, no draw has an offset <= tri34,
 * draw.meshIndex >= meshCount, t >= lods[lod].indexCount / 3, tri34 >= d_triangleOffsets[drawCount], or indexPosition + 2 does not fit 32
 * bits.  Outputs, each optional: d_records (width * height, 16-byte aligned), d_drawPixels (drawCount counters, += 1 per resolved pixel:
 * zero it first), d_totals4 (accumulated: covered pixels, unresolved pixels, 0, 0).
 * Enqueues one launch (no allocation, no synchronisation: it can be captured).  NV_EINVAL: a NULL ctx, cull, d_visibility or
 * d_triangleOffsets, width or height 0 or above 16384, d_draws NULL with drawCount > 0, d_meshes NULL with meshCount > 0, a misaligned
 * pointer (16 bytes: records, draws, meshes; 8: visibility, offsets, totals). */
int nv_visibility_resolve_indexed(nv_context* ctx, void* stream, const NvCullData* cull, const uint64_t* d_visibility, uint32_t width,
                                  uint32_t height, const NvMeshDraw* d_draws, uint32_t drawCount, const NvMesh* d_meshes, uint32_t meshCount,
                                  const uint64_t* d_triangleOffsets /* drawCount + 1 */, NvVisIndexedRecord* d_records /* optional */,
                                  uint32_t* d_drawPixels /* optional, drawCount */, uint64_t* d_totals4 /* optional */);

/* depthreduce.comp.glsl:14-22 + the level loop at src/niagara.cpp:1703-1733.
 * d_depth is the width x height fp32 depth target (reverse-Z, far = 0). */
int nv_depthreduce(nv_context* ctx, void* stream, const float* d_depth, uint32_t width, uint32_t height,
                   const NvPyramidDesc* pyramid);

/* ---- depth composite of a sharded frame (the reference has one device and no such step) ----
 * d_dst[i] = max(d_dst[i], d_srcs[0][i], ..., d_srcs[sources - 1][i]) for the width x height texels of tightly packed fp32 targets, the
 * maximum taken on the BIT PATTERNS as unsigned 32-bit integers.  For the depth the rasterisers write (reverse-Z, [0, 1], far = 0) that is
 * the maximum of the floats and the rule of their atomics, and it is exact, commutative and associative: shards that each rasterised a
 * part of the draws composite to the bits one pass over all draws writes, in any order and grouping.  Nothing else is special-cased: -0.0,
 * negative values and NaNs order by their bits (any pattern with the sign bit set is above every positive float, a NaN above infinity of
 * its sign), denormals are kept as they are.
 * d_srcs is a HOST array of `sources` device pointers (a pointer list, not base + stride: the targets of several contexts or a receive
 * buffer are separate allocations); it is read during the call only.  Enqueues only (sources / 8 rounded up launches), so it can be
 * captured.  NV_EINVAL: a NULL argument or list entry, sources == 0, width or height 0 or above 16384, a pointer that is not 4-byte
 * aligned, a source equal to d_dst.  A source that overlaps d_dst partially is the caller's error; sources may repeat or overlap each
 * other.  16-byte aligned pointers (any fresh allocation) take 16-byte loads and stores. */
int nv_depth_merge(nv_context* ctx, void* stream, float* d_dst, const float* const* d_srcs, uint32_t sources, uint32_t width,
                   uint32_t height);

/* ---- the stable-ID visibility buffer: composite and resolve (the reference reads its visibility in a fragment shader) ----
 * nv_visibility_merge: d_dst[i] = max(d_dst[i], d_srcs[0][i], ..., d_srcs[sources - 1][i]) for width x height unsigned 64-bit words.  With
 * NV_OPT_RASTER_VISIBILITY_ID 1 every shard of a frame writes the same word for the same sample, so the maximum over the shards' targets
 * is, bit for bit, the target one pass over all draws leaves.  Arguments, NV_EINVAL rules and launch shape as nv_depth_merge (8-byte
 * alignment required, 16-byte alignment takes 16-byte loads and stores; sources / 8 rounded up launches; enqueues only). */
int nv_visibility_merge(nv_context* ctx, void* stream, uint64_t* d_dst, const uint64_t* const* d_srcs, uint32_t sources, uint32_t width,
                        uint32_t height);

/* One resolved pixel of nv_visibility_resolve.  No sample: {0xFFFFFFFF, 0, 0, 0}.  Unresolved: all four words 0xFFFFFFFF. */
typedef struct NvVisRecord
{
	uint32_t drawId;       /* index into the d_draws the call was given (the full array: global ids in a sharded frame) */
	uint32_t meshletIndex; /* index into the scene's meshlets */
	uint32_t triangle;     /* < 96 */
	uint32_t depthBits;    /* bits of the fp32 depth of the sample */
} NvVisRecord;

/* nv_visibility_resolve: per pixel with a non-zero stable-form word (NV_OPT_RASTER_VISIBILITY_ID 1) of the width x height target
 *   mvi = (id34 - 1) >> 7, triangle = (id34 - 1) & 127, depthBits = word >> 34;
 *   drawId = the largest d < drawCount with d_draws[d].meshletVisibilityOffset <= mvi (the offsets must be non-decreasing in d, as
 *            nv_assign_visibility_offsets writes them; pass the FULL draw array, also on a rank of a sharded frame);
 *   lod    = what nv_drawcull selects for that draw under `cull` (drawcull.comp.glsl:104-112; cull->view, lodTarget and lodEnabled are
 *            read: pass the CullData of the frame that was rasterised);
 *   meshletIndex = d_meshes[draw.meshIndex].lods[lod].meshletOffset + (mvi - draw.meshletVisibilityOffset).
 * The pixel is UNRESOLVED — its record all ones, counted, nothing else written — when no draw has an offset <= mvi, draw.meshIndex >=
 * meshCount, mvi - offset >= lods[lod].meshletCount, triangle >= 96 or id34 == 0.  Outputs, each optional:
 *   d_records      width * height records (16-byte aligned);
 *   d_meshletSeen  bit mvi set (atomic OR) for every resolved pixel, in nv_clustercull's d_meshletVisibility layout (the same size):
 *                  the pixel-exact counterpart of that buffer; the caller clears it;
 *   d_drawPixels   drawCount counters, d_drawPixels[drawId] += 1 per resolved pixel (accumulated: zero it first);
 *   d_totals4      accumulated: covered pixels (non-zero words), unresolved pixels, 0, 0.
 * Enqueues one launch (no allocation, no synchronisation: it can be captured).  NV_EINVAL: a NULL ctx, cull or d_visibility, width or
 * height 0 or above 16384, d_draws NULL with drawCount > 0, d_meshes NULL with meshCount > 0, a misaligned pointer. */
int nv_visibility_resolve(nv_context* ctx, void* stream, const NvCullData* cull, const uint64_t* d_visibility, uint32_t width, uint32_t height,
                          const NvMeshDraw* d_draws, uint32_t drawCount, const NvMesh* d_meshes, uint32_t meshCount,
                          NvVisRecord* d_records /* optional, width*height */, uint32_t* d_meshletSeen /* optional */,
                          uint32_t* d_drawPixels /* optional, drawCount */, uint64_t* d_totals4 /* optional */);

/* ---- the attribute pass of the visibility buffer (replaces the varyings of meshlet.mesh.glsl and mesh.frag.glsl) ---- */

/* src/scene.h:25-37, src/shaders/mesh.h:80-90 (std430: the vec3 emissiveFactor is padded to 16 bytes); 64 B, align 16 */
typedef struct NvMaterial
{
	uint32_t albedoTexture;
	uint32_t normalTexture;
	uint32_t specularTexture;
	uint32_t emissiveTexture;
	float diffuseFactor[4];
	float specularFactor[4];
	float emissiveFactor[3];
	uint32_t padding;
} NvMaterial;

/* One pixel of nv_visibility_attributes: what mesh.frag.glsl:27-31 receives, plus the barycentrics.  No sample and invalid records: all
 * zero except drawId = 0xFFFFFFFF. */
typedef struct NvPixelAttributes
{
	float uv[2];
	float bary[2];          /* lambda1, lambda2 (lambda0 belongs to the triangle's first index); not clamped */
	float normal[3];        /* interpolated, not normalised */
	uint32_t drawId;
	float tangent[4];
	float wpos[3];
	uint32_t materialIndex; /* d_draws[drawId].materialIndex */
} NvPixelAttributes;

/* nv_visibility_attributes: per pixel of nv_visibility_resolve's records (width x height, the frame's `globals`: projection, cullData.view)
 * the triangle's three vertices go through the mesh shader's vertex stage (meshlet.mesh.glsl:125-147: index and vertex fetch with shortRefs,
 * position -> wpos -> clip with nv_rasterdepth's arithmetic, texcoord from fp16, unpackTBN, rotateQuat of normal and tangent), homogeneous
 * barycentrics are taken at the pixel centre nx = ((px + 0.5) / width) 2 - 1, ny = 1 - ((py + 0.5) / height) 2 (row 0 at the top):
 *   d_i = (x_i - nx w_i, y_i - ny w_i), b0 = d1 x d2, b1 = d2 x d0, b2 = d0 x d1, s = (b0 + b1) + b2, lambda_i = b_i / s
 * (vertices with w <= 0 of a near-clipped triangle need no special case), and every varying is (l0 a0 + l1 a1) + l2 a2.  A pixel whose s is 0
 * or whose lambdas are not all finite is DEGENERATE: lambda = (1, 0, 0), counted.  The lambdas are not clamped: the rasteriser covers by
 * positions snapped to 1/256 pixel, so a lambda of a covered pixel can be slightly negative.  With d_materials the fragment stage
 * (mesh.frag.glsl:57-89) is evaluated from the material's factors — this entry point samples no textures (nv_visibility_attributes_textured
 * does); a material with a texture index > 0 is shaded from its factors and its pixels are counted — and packed: d_gbuffer0 R8G8B8A8_UNORM {tosrgb(albedo).rgb, log2(1 + emissivef) / 5},
 * d_gbuffer1 A2B10G10R10_UNORM_PACK32 {encodeOct(nrm) * 0.5 + 0.5 + deband * (0.5 / 1023), specgloss.a, 0} (src/niagara.cpp:634-637), UNORM =
 * clamp to [0, 1] with NaN -> 0, times 2^bits - 1, rounded half to even.  The POST alpha discard (:88) is coverage: nv_rasterdepth_textured applies it, this pass does not.
 * Every fp32 operation is one IEEE operation in a fixed order; pow and log2 (gbuffer0 only) are the device's.
 * A record with drawId == 0xFFFFFFFF (no sample, unresolved) writes the no-sample attributes and 0 into both G-buffer words.  A record is
 * INVALID — counted, written like no sample — when drawId >= drawCount, meshletIndex >= meshletCount, triangle >= min(triangleCount, 96), an
 * index byte >= min(vertexCount, 64), an index byte or vertex reference lies past meshletDataWords, a resolved vertex index >= vertexCount,
 * or (with d_materials) materialIndex >= materialCount: every load stays inside the caller's buffers, which need no padding.
 * Outputs, each optional: d_attributes (width * height NvPixelAttributes, 16-byte aligned), d_gbuffer0 / d_gbuffer1 (width * height u32; either
 * requires d_materials), d_totals4 (accumulated: pixels shaded, invalid records, degenerate pixels, pixels whose material names a texture; the
 * last one stays 0 without d_materials).
 * Enqueues one launch (no allocation, no synchronisation: it can be captured).  NV_EINVAL: a NULL ctx, globals or d_records, width or height 0
 * or above 16384, or not globals->screenWidth / screenHeight, a NULL array with a non-zero count, a G-buffer output without d_materials, a
 * misaligned pointer (16 bytes: records, attributes, draws, vertices, materials; 8: totals; 4: the rest). */
int nv_visibility_attributes(nv_context* ctx, void* stream, const NvGlobals* globals, const NvVisRecord* d_records, uint32_t width, uint32_t height,
                             const NvMeshDraw* d_draws, uint32_t drawCount, const NvMeshlet* d_meshlets, uint32_t meshletCount,
                             const uint32_t* d_meshletData, uint32_t meshletDataWords, const NvVertex* d_vertices, uint32_t vertexCount,
                             const NvMaterial* d_materials /* optional */, uint32_t materialCount, NvPixelAttributes* d_attributes /* optional */,
                             uint32_t* d_gbuffer0 /* optional */, uint32_t* d_gbuffer1 /* optional */, uint64_t* d_totals4 /* optional */);

/* nv_visibility_attributes_indexed: nv_visibility_attributes over nv_visibility_resolve_indexed's records — the classic
 * path's vertex stage (mesh.vert.glsl:41-62) per corner, vi = d_indices[indexPosition + k] + vertexOffset (mod 2^32), k = 0 .. 2, then
 * mesh.frag.glsl.  From the three fetched vertices on it is nv_visibility_attributes, word for word: the clip position, unpackTBN, the
 * homogeneous barycentrics, the degenerate rule, the fragment stage from the material's factors (no texture is sampled; a material that
 * names one is counted in totals word 3), the UNORM packs, the output structs and d_totals4.  A record is INVALID — counted, written like
 * no sample — when drawId >= drawCount, indexPosition + 2 >= indexCapacity (in 64 bits), a corner >= vertexCapacity, or (with d_materials)
 * materialIndex >= materialCount: every load stays inside the caller's buffers.  Alignment rules and NV_EINVAL as nv_visibility_attributes
 * (d_indices: 4 bytes, NULL only with indexCapacity 0).  Enqueues one launch; it can be captured. */
int nv_visibility_attributes_indexed(nv_context* ctx, void* stream, const NvGlobals* globals, const NvVisIndexedRecord* d_records, uint32_t width,
                                     uint32_t height, const NvMeshDraw* d_draws, uint32_t drawCount, const uint32_t* d_indices,
                                     uint32_t indexCapacity, const NvVertex* d_vertices, uint32_t vertexCapacity,
                                     const NvMaterial* d_materials /* optional */, uint32_t materialCount,
                                     NvPixelAttributes* d_attributes /* optional */, uint32_t* d_gbuffer0 /* optional */,
                                     uint32_t* d_gbuffer1 /* optional */, uint64_t* d_totals4 /* optional */);

/* ---- material textures (replaces binding 8 `textureSampler` and set 1 `textures[]` of mesh.frag.glsl) ----
 * CDNA has no texture unit a HIP kernel can use: the library reads niagara's DDS files, decodes their BC blocks to RGBA8 once at load time
 * and samples the decoded mip chains in software.  The caller owns every buffer.
 *
 * nv_dds_parse restates loadImage's accept / reject rules (src/textures.cpp:159-210) on a file image in memory: the magic "DDS ", a 124-byte
 * header with a 32-byte pixel format, the DX10 header when the FourCC says so, no cube map and no volume, a DX10 resourceDimension of
 * TEXTURE2D, the FourCC / DXGI table of getFormat (:82-127), and a payload of EXACTLY getImageSizeBC(width, height, mipCount, blockSize) bytes
 * with nothing behind it (level l is max(1, w >> l) x max(1, h >> l), partial blocks round up).  NV_EFORMAT otherwise (also: width, height or
 * the mip count 0, a side above 16384, more than NV_TEXTURE_MAX_LEVELS levels — shapes the library's own arithmetic excludes).  Host only. */
#define NV_TEXTURE_MAX_LEVELS 15
#define NV_ETEXFORMAT (-7) /* a well-formed texture in a format the library does not decode (BC4, BC5, BC6H) */
enum
{
	NV_FORMAT_BC1 = 1,
	NV_FORMAT_BC2 = 2,
	NV_FORMAT_BC3 = 3,
	NV_FORMAT_BC4 = 4, /* parses; refused by nv_texture_set_layout and the decoders with NV_ETEXFORMAT */
	NV_FORMAT_BC5 = 5, /* as BC4 */
	NV_FORMAT_BC6H = 6, /* as BC4 */
	NV_FORMAT_BC7 = 7
};
typedef struct NvDdsInfo
{
	uint32_t format;    /* NV_FORMAT_* */
	uint32_t width, height, levels;
	uint32_t blockBytes; /* 8: BC1, BC4; 16: the rest */
	uint32_t payloadOffset; /* of level 0's first block in the file: 128, or 148 with a DX10 header */
	uint64_t payloadBytes;
	uint64_t levelOffset[NV_TEXTURE_MAX_LEVELS]; /* byte offset of each level's blocks FROM payloadOffset; entries past `levels` are 0 */
} NvDdsInfo;
int nv_dds_parse(const void* bytes, uint64_t size, NvDdsInfo* out);

/* One decoded texture: its RGBA8 levels (R in the low byte; UNORM, never SRGB — getFormat, textures.cpp:82-127) lie one after the other, each
 * row-major without padding, from word `offset` of the set's texel buffer.  16 bytes, fixed (niagara_amd/layouts.py TEXTUREDESC). */
typedef struct NvTextureDesc
{
	uint32_t offset; /* in 32-bit words */
	uint32_t width, height, levels;
} NvTextureDesc;

/* nv_texture_set_layout: a pure function that places `count` textures in one linear buffer.  descs has count + 1 entries: entry 0 is the
 * reserved "no texture" entry (all zero; textures[id] binds texturePaths[id - 1], src/niagara.cpp:934), entry i + 1 belongs to infos[i].
 * *texelWords = the words the caller allocates.  NV_ETEXFORMAT: a BC4 / BC5 / BC6H texture; NV_EINVAL: a NULL pointer, a shape nv_dds_parse
 * would not report, or a total of 2^32 words or more. */
int nv_texture_set_layout(const NvDdsInfo* infos, uint32_t count, NvTextureDesc* descs, uint64_t* texelWords);

/* the decode of one texture's levels on the CPU (csrc/texmath.h, the text the kernel runs): blocks = the file's payload (info->payloadBytes
 * bytes), texels = the set's buffer (texelWords words), written at desc->offset.  NV_EINVAL when desc and info disagree or the chain does not
 * fit texelWords; NV_ETEXFORMAT as above. */
int nv_texture_decode_host(const NvDdsInfo* info, const void* blocks, const NvTextureDesc* desc, uint32_t* texels, uint64_t texelWords);

/* nv_texture_decode: the same on the device, every level in one launch (d_blocks: the payload, 8-byte aligned; d_texels + desc->offset .. :
 * width x height x levels chain).  A work item decodes one row of a block and stores it cropped at the level's right and bottom edges, so
 * nothing past a level's last texel is written; the caller's buffer holds desc->offset + the chain's words (nv_texture_set_layout).  desc is
 * read on the host.  Only enqueued work: capturable.  NV_EINVAL: a NULL or misaligned pointer, a shape nv_dds_parse would not report, desc
 * not of this shape; NV_ETEXFORMAT as the host function. */
int nv_texture_decode(nv_context* ctx, void* stream, const void* d_blocks, uint32_t format, uint32_t width, uint32_t height, uint32_t levels,
                      uint32_t* d_texels, const NvTextureDesc* desc);

/* one sample of textures[id] on the CPU, the sampler of §4.18 (`textureSampler`: LINEAR / LINEAR / mipmap LINEAR, REPEAT, lod 0..16, no
 * anisotropy): uv, and its derivatives per pixel step in x and y (the level of detail is the Vulkan isotropic rule).  out_rgba: four floats.
 * NV_EINVAL: id == 0 or >= textureCount (descs has textureCount entries, entry 0 reserved), or a descriptor whose chain does not lie inside
 * texelWords.  No index reaches a load out of range for ANY bit pattern of uv and the derivatives. */
int nv_texture_sample_host(const NvTextureDesc* descs, uint32_t textureCount, const uint32_t* texels, uint64_t texelWords, uint32_t id,
                           const float uv[2], const float duvdx[2], const float duvdy[2], float out_rgba[4]);

/* nv_visibility_attributes_textured: nv_visibility_attributes with the COMPLETE fragment stage (mesh.frag.glsl:57-89): albedo, specgloss
 * and emissive times fromsrgb(texture(...)), nmap = texture(...).rgb * 2 - 1 through tangent, bitangent and normal.  All arguments, outputs,
 * rules and errors of nv_visibility_attributes hold; d_materials is required.  d_textures: textureCount descriptors (entry 0 reserved),
 * d_texels: the decoded set, texelWords words.  The derivatives are analytic: the triangle's barycentrics are evaluated again at the
 * centres of (px + 1, py) and (px, py + 1) (nothing is loaded there; a degenerate neighbour contributes a zero difference).  Before any
 * texel load the index is checked against textureCount and the descriptor's whole chain against texelWords; a texture that fails is treated
 * as absent and the pixel is counted in d_totals4[3], which keeps its meaning — pixels whose material names a texture the pass did not
 * sample — and is 0 on a complete set.  With d_textures NULL (textureCount 0) the outputs equal nv_visibility_attributes' bit for bit.
 * One launch, capturable.  NV_EINVAL also: d_materials NULL, textureCount > 0 with d_textures or d_texels NULL, a misaligned d_textures
 * (16) or d_texels (4). */
int nv_visibility_attributes_textured(nv_context* ctx, void* stream, const NvGlobals* globals, const NvVisRecord* d_records, uint32_t width,
                                      uint32_t height, const NvMeshDraw* d_draws, uint32_t drawCount, const NvMeshlet* d_meshlets,
                                      uint32_t meshletCount, const uint32_t* d_meshletData, uint32_t meshletDataWords, const NvVertex* d_vertices,
                                      uint32_t vertexCount, const NvMaterial* d_materials, uint32_t materialCount,
                                      NvPixelAttributes* d_attributes /* optional */, uint32_t* d_gbuffer0 /* optional */,
                                      uint32_t* d_gbuffer1 /* optional */, uint64_t* d_totals4 /* optional */, const NvTextureDesc* d_textures,
                                      uint32_t textureCount, const uint32_t* d_texels, uint64_t texelWords);

/* ---- block-resident texture sets ----
 * A second residency for a texture set: the device buffer holds the DDS payloads verbatim (8 bytes per 16 texels for BC1, 16 for BC2 / BC3 /
 * BC7, against 64 decoded) and the sampler decodes each tap's texel from its block when it fetches it.  A tap decoded from its block is the
 * RGBA8 code nv_texture_decode stores, and everything after the fetch is the decoded sampler's text: the results are the decoded entry
 * points', bit for bit.  Opt-in: the decoded entry points are untouched.
 *
 * One block-resident texture: its payload — level after level exactly as the file has them (NvDdsInfo.levelOffset) — lies from byte
 * 16 * offset of the set's block buffer.  Level l is a grid of ceil(w_l / 4) x ceil(h_l / 4) blocks, row-major; texel (x, y) is texel
 * (y & 3) * 4 + (x & 3) of block (x >> 2, y >> 2).  16 bytes, fixed (niagara_amd/layouts.py TEXTUREBLOCKDESC). */
typedef struct NvTextureBlockDesc
{
	uint32_t offset;       /* in 16-byte units: every 16-byte block stays aligned, a set can reach 64 GiB */
	uint32_t width, height;
	uint32_t levelsFormat; /* the level count in bits 0-7, NV_FORMAT_* in bits 8-15, bits 16-31 zero */
} NvTextureBlockDesc;

/* nv_texture_block_layout: nv_texture_set_layout for the block form, a pure function.  descs has count + 1 entries (entry 0 reserved, all
 * zero; entry i + 1 belongs to infos[i]); each payload is rounded up to 16 bytes; *units16 = the 16-byte units the caller allocates.
 * Uploading is a plain copy of infos[i]'s payload to byte 16 * descs[i + 1].offset: no kernel.  Refuses what nv_texture_set_layout refuses,
 * with its codes; NV_EINVAL also for a total of 2^32 units or more. */
int nv_texture_block_layout(const NvDdsInfo* infos, uint32_t count, NvTextureBlockDesc* descs, uint64_t* units16);

/* the RGBA8 code of texel (x, y) of `level`, decoded from its block on the CPU (csrc/texmath.h, the text the kernels run): the word
 * nv_texture_decode_host stores there.  blocks: the set's block buffer, units16 units.  NV_EINVAL: a NULL pointer, a descriptor the check in
 * front of every block load refuses (shape, format, levelsFormat's upper bits, a chain past units16), level, x or y outside the texture. */
int nv_texture_block_fetch_host(const NvTextureBlockDesc* desc, const void* blocks, uint64_t units16, uint32_t level, uint32_t x, uint32_t y,
                                uint32_t* rgba);

/* nv_texture_sample_host over a block-resident set: the same bits */
int nv_texture_block_sample_host(const NvTextureBlockDesc* descs, uint32_t textureCount, const void* blocks, uint64_t units16, uint32_t id,
                                 const float uv[2], const float duvdx[2], const float duvdy[2], float out_rgba[4]);

/* test accessors of the per-block decode: out_alpha[t] = the alpha-only decode of texel t, out_split[t] = the RGBA8 code through the BC7
 * header / per-texel split (the plain decode for the other formats), of the block {lo, hi} of a decodable format (NV_EINVAL otherwise) */
int nv_texture_block_decode_host(uint32_t format, uint64_t lo, uint64_t hi, uint32_t out_alpha[16], uint32_t out_split[16]);

/* nv_visibility_attributes_blocks: nv_visibility_attributes_textured over a block-resident set.  Its arguments, outputs, d_totals4[3] rule
 * and errors; d_textures: NvTextureBlockDesc, d_blocks: the block buffer (16-byte aligned), units16 its size.  Before any block load the index
 * is checked against textureCount and the descriptor against units16 (shape, format, whole chain, in 64 bits).  Outputs equal
 * nv_visibility_attributes_textured's over the decoded form of the same set bit for bit.  One launch, capturable. */
int nv_visibility_attributes_blocks(nv_context* ctx, void* stream, const NvGlobals* globals, const NvVisRecord* d_records, uint32_t width,
                                    uint32_t height, const NvMeshDraw* d_draws, uint32_t drawCount, const NvMeshlet* d_meshlets,
                                    uint32_t meshletCount, const uint32_t* d_meshletData, uint32_t meshletDataWords, const NvVertex* d_vertices,
                                    uint32_t vertexCount, const NvMaterial* d_materials, uint32_t materialCount,
                                    NvPixelAttributes* d_attributes /* optional */, uint32_t* d_gbuffer0 /* optional */,
                                    uint32_t* d_gbuffer1 /* optional */, uint64_t* d_totals4 /* optional */, const NvTextureBlockDesc* d_textures,
                                    uint32_t textureCount, const void* d_blocks, uint64_t units16);

/* nv_rasterdepth_blocks: nv_rasterdepth_textured (below) over a block-resident set — its parameters, rules, counters and errors, with
 * NvTextureBlockDesc descriptors, d_blocks (16-byte aligned) and units16.  Depth, visibility, d_totals4 and d_alphaTotals2 equal
 * nv_rasterdepth_textured's over the decoded form of the same set bit for bit. */
int nv_rasterdepth_blocks(nv_context* ctx, void* stream, const NvGlobals* globals, const NvMeshTaskCommand* d_commands, const NvMeshDraw* d_draws,
                          const NvMeshlet* d_meshlets, const uint32_t* d_meshletData, const NvVertex* d_vertices, const uint32_t* d_clusterIndices,
                          const uint32_t* d_clusterCount4, float* d_depth, uint32_t width, uint32_t height, uint64_t* d_visibility /* optional */,
                          uint64_t* d_totals4 /* optional */, const NvMaterial* d_materials /* optional */, uint32_t materialCount,
                          const NvTextureBlockDesc* d_textures /* optional */, uint32_t textureCount, const void* d_blocks /* optional */,
                          uint64_t units16, uint64_t* d_alphaTotals2 /* optional */);

/* ---- depth raster with the POST alpha discard as coverage ----
 * nv_rasterdepth whose covered samples of a post-pass launch also pass the fragment's alpha test (mesh.frag.glsl:88,
 * `if (POST > 0 && albedo.a < 0.5) discard;`) before they touch d_depth or d_visibility.  The first fifteen parameters, the options
 * (NV_OPT_RASTER_SMALL_LIMIT, NV_OPT_RASTER_NEAR_CLIP, NV_OPT_RASTER_VISIBILITY_ID) and every rule of coverage and depth are nv_rasterdepth's.
 * The test applies only when globals->cullData.postPass != 0 and d_materials is given; otherwise the call writes exactly nv_rasterdepth's bits
 * and totals, and both alpha totals stay as they are.  Per slot (cluster) the draw's materialIndex selects materials[materialIndex]:
 *   - materialIndex >= materialCount: the slot is opaque (nv_rasterdepth's road); its covered samples are counted as unevaluated;
 *   - albedoTexture == 0: albedo.a = diffuseFactor.a for every sample of the slot;
 *   - albedoTexture >= textureCount, or d_textures[albedoTexture] does not describe a chain inside texelWords (nv_visibility_attributes_textured's
 *     descriptor rule): the texture is treated as absent, albedo.a = diffuseFactor.a, and the covered samples are counted as unevaluated;
 *   - otherwise albedo.a = diffuseFactor.a * texture(albedo, uv).a per covered sample, with uv and its per-pixel steps taken from the ORIGINAL
 *     triangle (with NV_OPT_RASTER_NEAR_CLIP 1 too: not from the piece) at the pixel centre exactly as nv_visibility_attributes_textured takes them
 *     for the same triangle and pixel, and the same sampler (REPEAT, trilinear, the level of detail's log2 is the device's).
 * A covered sample with albedo.a < 0.5 is dropped: no load, no atomic on either target.  A NaN albedo.a keeps the sample.  Every texel index
 * stays inside d_texels for every bit pattern of the texcoords.  The depth bias of the post pass stays unmodelled.
 * d_totals4 words 0-2 are nv_rasterdepth's; word 3 counts the samples KEPT.  d_alphaTotals2 (optional, accumulated: zero it first): samples
 * dropped, samples unevaluated.  Word 3 + dropped = nv_rasterdepth's word 3 on the same inputs; every total is independent of the order of the
 * GPU's work (alpha is evaluated for every covered sample of an alpha-tested slot, whether or not it could still raise the targets).
 * NV_EINVAL, nothing launched: nv_rasterdepth's refusals; d_commands / d_clusterIndices / d_clusterCount4 / d_depth / d_meshlets /
 * d_meshletData / d_texels not 4-byte aligned, d_visibility / d_totals4 / d_alphaTotals2 not 8-byte aligned, d_draws / d_vertices / d_materials /
 * d_textures not 16-byte aligned; d_textures without d_texels or the reverse; textureCount != 0 without d_textures; d_materials with
 * materialCount == 0.  NV_ENOMEM: d_alphaTotals2 while the context holds no partial sums for it (nv_create reserves them). */
int nv_rasterdepth_textured(nv_context* ctx, void* stream, const NvGlobals* globals, const NvMeshTaskCommand* d_commands,
                            const NvMeshDraw* d_draws, const NvMeshlet* d_meshlets, const uint32_t* d_meshletData,
                            const NvVertex* d_vertices, const uint32_t* d_clusterIndices, const uint32_t* d_clusterCount4,
                            float* d_depth, uint32_t width, uint32_t height,
                            uint64_t* d_visibility /* optional, width*height */, uint64_t* d_totals4 /* optional */,
                            const NvMaterial* d_materials /* optional */, uint32_t materialCount,
                            const NvTextureDesc* d_textures /* optional */, uint32_t textureCount,
                            const uint32_t* d_texels /* optional */, uint64_t texelWords, uint64_t* d_alphaTotals2 /* optional */);

/* ---- the classic path with textures: the complete fragment stage and the POST alpha discard for the indexed draws ----
 * nv_visibility_attributes_indexed_textured: nv_visibility_attributes_indexed with the complete fragment stage.  The records, the corner
 * validity, the run key, d_totals4 words 0-2 and the output of an invalid record are nv_visibility_attributes_indexed's; the descriptor rule
 * (an id past textureCount or a descriptor that does not describe a chain inside texelWords: the texture is treated as absent), the
 * d_totals4[3] rule (pixels whose material names a texture the pass could not sample) and the sampler are nv_visibility_attributes_textured's.
 * NV_EINVAL, nothing launched: the union of the two parents' refusals (d_materials is required).  One launch, capturable. */
int nv_visibility_attributes_indexed_textured(nv_context* ctx, void* stream, const NvGlobals* globals, const NvVisIndexedRecord* d_records, uint32_t width,
                                              uint32_t height, const NvMeshDraw* d_draws, uint32_t drawCount, const uint32_t* d_indices,
                                              uint32_t indexCapacity, const NvVertex* d_vertices, uint32_t vertexCapacity, const NvMaterial* d_materials,
                                              uint32_t materialCount, NvPixelAttributes* d_attributes /* optional */, uint32_t* d_gbuffer0 /* optional */,
                                              uint32_t* d_gbuffer1 /* optional */, uint64_t* d_totals4 /* optional */, const NvTextureDesc* d_textures,
                                              uint32_t textureCount, const uint32_t* d_texels, uint64_t texelWords);

/* the same pass over a block-resident set (NvTextureBlockDesc, d_blocks 16-byte aligned, units16): the same outputs bit for bit */
int nv_visibility_attributes_indexed_blocks(nv_context* ctx, void* stream, const NvGlobals* globals, const NvVisIndexedRecord* d_records, uint32_t width,
                                            uint32_t height, const NvMeshDraw* d_draws, uint32_t drawCount, const uint32_t* d_indices,
                                            uint32_t indexCapacity, const NvVertex* d_vertices, uint32_t vertexCapacity, const NvMaterial* d_materials,
                                            uint32_t materialCount, NvPixelAttributes* d_attributes /* optional */, uint32_t* d_gbuffer0 /* optional */,
                                            uint32_t* d_gbuffer1 /* optional */, uint64_t* d_totals4 /* optional */, const NvTextureBlockDesc* d_textures,
                                            uint32_t textureCount, const void* d_blocks, uint64_t units16);

/* nv_rasterdepth_indexed_textured: nv_rasterdepth_indexed_visibility whose covered samples of a post-pass launch also pass the fragment's alpha
 * test before they touch d_depth or d_visibility.  d_triangleOffsets / d_visibility are optional as a pair: both NULL is depth only.  The
 * options, smallLimit, both faces in the post pass, the skip rules and the count / scan launches are nv_rasterdepth_indexed's.
 * The test is nv_rasterdepth_textured's, stated per command where that states it per slot.  It applies only when
 * globals->cullData.postPass != 0 and d_materials is given; otherwise the call writes nv_rasterdepth_indexed_visibility's bits and totals (with
 * both visibility pointers NULL nv_rasterdepth_indexed's) and both alpha totals stay as they are.  The command's draw gives materialIndex:
 *   - materialIndex >= materialCount: the command is opaque; its covered samples are counted as unevaluated;
 *   - albedoTexture == 0: albedo.a = diffuseFactor.a for every sample of the command;
 *   - albedoTexture >= textureCount or a refused descriptor: the texture is absent, albedo.a = diffuseFactor.a, the samples are unevaluated;
 *   - otherwise albedo.a = diffuseFactor.a * texture(albedo, uv).a per covered sample, uv and its per-pixel steps from the ORIGINAL triangle's
 *     corners (with NV_OPT_RASTER_NEAR_CLIP 1 too) exactly as nv_visibility_attributes_indexed_textured takes them for that triangle and pixel.
 * A covered sample with albedo.a < 0.5 is dropped: no load, no atomic on either target.  A NaN albedo.a keeps the sample.  The depth bias of
 * the post pass stays unmodelled.  d_totals4 words 0-2 are nv_rasterdepth_indexed's; word 3 counts the samples KEPT.  d_alphaTotals2
 * (optional, accumulated: zero it first): samples dropped, samples unevaluated.  Word 3 + dropped = nv_rasterdepth_indexed's word 3 on the
 * same inputs; every total is independent of the order of the GPU's work.
 * NV_EINVAL, nothing launched: nv_rasterdepth_indexed's refusals; one of d_triangleOffsets / d_visibility without the other; d_commands /
 * d_count / d_indices / d_depth / d_texels not 4-byte aligned, d_triangleOffsets / d_visibility / d_totals4 / d_alphaTotals2 not 8-byte aligned,
 * d_draws / d_vertices / d_materials / d_textures not 16-byte aligned; d_textures without d_texels or the reverse; textureCount != 0 without
 * d_textures; d_materials with materialCount == 0.  NV_ENOMEM: nv_rasterdepth_indexed's, and d_alphaTotals2 while the context holds no
 * partial sums for it (nv_create reserves them).  Capturable: the launches only enqueue work. */
int nv_rasterdepth_indexed_textured(nv_context* ctx, void* stream, const NvGlobals* globals, const NvMeshDrawCommand* d_commands, const uint32_t* d_count,
                                    const NvMeshDraw* d_draws, uint32_t drawCount, const uint32_t* d_indices, uint32_t indexCapacity,
                                    const NvVertex* d_vertices, uint32_t vertexCapacity, float* d_depth, uint32_t width, uint32_t height,
                                    uint64_t* d_totals4 /* optional */, const uint64_t* d_triangleOffsets /* optional */,
                                    uint64_t* d_visibility /* optional */, const NvMaterial* d_materials /* optional */, uint32_t materialCount,
                                    const NvTextureDesc* d_textures /* optional */, uint32_t textureCount, const uint32_t* d_texels /* optional */,
                                    uint64_t texelWords, uint64_t* d_alphaTotals2 /* optional */);

/* the same pass over a block-resident set (NvTextureBlockDesc, d_blocks 16-byte aligned, units16): targets and counters bit for bit */
int nv_rasterdepth_indexed_blocks(nv_context* ctx, void* stream, const NvGlobals* globals, const NvMeshDrawCommand* d_commands, const uint32_t* d_count,
                                  const NvMeshDraw* d_draws, uint32_t drawCount, const uint32_t* d_indices, uint32_t indexCapacity,
                                  const NvVertex* d_vertices, uint32_t vertexCapacity, float* d_depth, uint32_t width, uint32_t height,
                                  uint64_t* d_totals4 /* optional */, const uint64_t* d_triangleOffsets /* optional */,
                                  uint64_t* d_visibility /* optional */, const NvMaterial* d_materials /* optional */, uint32_t materialCount,
                                  const NvTextureBlockDesc* d_textures /* optional */, uint32_t textureCount, const void* d_blocks /* optional */,
                                  uint64_t units16, uint64_t* d_alphaTotals2 /* optional */);

/* ---- the shading end of the frame (replaces shadowfill.comp.glsl, shadowblur.comp.glsl and final.comp.glsl) ----
 * Three of niagara's compute passes behind the G-buffer.  All images are linear buffers with row 0 at the top, as the raster target is:
 *   depth               width * height fp32, the raster target as it stands: reverse-Z, 0 = no sample;
 *   gbuffer0 / gbuffer1 width * height u32 as nv_visibility_attributes packs them: R8G8B8A8_UNORM, and A2B10G10R10_UNORM_PACK32 with R in bits 0-9;
 *   shadow images       width * height u8 (VK_FORMAT_R8_UNORM, src/niagara.cpp:1328-1329), row pitch = width;
 *   output colour       width * height u32 R8G8B8A8_UNORM, R in the low byte.  niagara writes the output in the swapchain's format
 *                       (src/niagara.cpp:1864,1915 bind the swapchain image): a caller with a BGRA swapchain swizzles R and B.
 * Rule set: every fp32 operation is one IEEE operation in the shader's order; max(a, b) = a < b ? b : a and min(a, b) =
 * b < a ? b : a with the shader's argument order; UNORM fetch = code / (2^bits - 1); UNORM store = clamp to [0, 1] with NaN -> 0, times
 * 2^bits - 1, round half to even; pow and exp2 are the device's.  A texelFetch / imageLoad OUTSIDE the image returns 0 and an imageStore
 * outside it is dropped (Vulkan leaves both undefined without robust access; this is the library's defined semantic): every load stays
 * inside the caller's buffers, which need no padding.
 * Each entry point enqueues one launch (no allocation, no synchronisation: it can be captured).  NV_EINVAL: a NULL ctx or required pointer,
 * width or height 0 or above 16384, a depth / G-buffer / colour pointer that is not 4-byte aligned, and what each entry point names. */

/* src/niagara.cpp:280-290, final.comp.glsl:10-19; 112 B (104 used), align 16.  inverseViewProjection is column-major */
typedef struct NvShadeData
{
	float cameraPosition[3];
	float pad0;
	float sunDirection[3];
	int32_t shadowsEnabled;
	float inverseViewProjection[16];
	float imageSize[2];
	float _pad[2];
} NvShadeData;

/* shadowfill.comp.glsl:17-46 over (width + 1) / 2 x height invocations (src/niagara.cpp:1797,1833), IN PLACE: invocation (x, y) owns the
 * texel (2 x + (~(y ^ checkerboard) & 1), y) and replaces it by the depth-weighted mean of its four neighbours,
 * dot(w, shadows) / (dot(w, 1) + 1e-2) with w = exp2(-abs(depths / depth - 1) * 20).  It reads texels of the other checkerboard parity only, so
 * the update has no race; the texels of that other parity keep their bytes.  With an odd width the last invocation of a row can own x ==
 * width: its store is dropped. */
int nv_shadow_fill(nv_context* ctx, void* stream, uint8_t* d_shadow, const float* d_depth, uint32_t width, uint32_t height, int checkerboard);

/* shadowblur.comp.glsl:24-64 with BLUR 1: a 21-tap depth-aware filter along one axis, direction 1 = horizontal, 0 = vertical
 * (src/niagara.cpp:1847; anything else NV_EINVAL), znear as in NvCullData (the shader compares znear / depth, the view-space distance).
 * exp2(-i * i / 50) is the shader's integer arithmetic: 1 for i = 1..7, 0.5 for 8 and 9, 0.25 for 10.  A tap outside the image has depth 0,
 * distance +inf and therefore weight 0.  d_out == d_shadow is NV_EINVAL (partly overlapping images are the caller's error). */
int nv_shadow_blur(nv_context* ctx, void* stream, uint8_t* d_out, const uint8_t* d_shadow, const float* d_depth, uint32_t width, uint32_t height,
                   int direction, float znear);

/* final.comp.glsl:37-80: the lit, tonemapped, debanded colour of every pixel from the two G-buffer words, the depth and (shadowsEnabled == 1)
 * the shadow image; alpha is 255.  THE BLOOM TERM IS LEFT OUT: the result is exactly the shader's with an all-zero bloom image.  A sky pixel
 * (depth 0) has wposh.w == 0 and a NaN view vector, as in the shader; tonemap's max(0, c - 0.004) turns it into 0.  gradientNoise takes the
 * integer pixel position (no half-pixel offset, unlike mesh.frag.glsl).  NV_EINVAL also: shade->imageSize not (width, height); d_shadow NULL
 * with shade->shadowsEnabled == 1 (with any other value the shadow image is never read and may be NULL). */
int nv_shade_final(nv_context* ctx, void* stream, const NvShadeData* shade, const uint32_t* d_gbuffer0, const uint32_t* d_gbuffer1,
                   const float* d_depth, const uint8_t* d_shadow /* optional */, uint32_t* d_color, uint32_t width, uint32_t height);

/* ---- bloom (replaces bloom.comp.glsl and the bloom term of final.comp.glsl) ----
 * The bloom target is ONE linear buffer of u32 holding VK_FORMAT_B10G11R11_UFLOAT_PACK32 texels (R in bits 0-10, G in bits 11-21, B in bits
 * 22-31), the levels concatenated, row 0 at the top, row pitch = the level's width; level i is max(1, width >> i) x max(1, height >> i) texels
 * at d_bloom + levelOffset[i] (src/niagara.cpp:1331-1333: width = (image width + 1) / 2, height likewise, levels = min(8, mip levels)).
 * Rule set: the UFLOAT decode is exact; the store rounds toward zero, clamps a finite value to the largest finite code,
 * keeps +inf, stores NaN as exponent 31 with the top mantissa bit and anything else with the sign bit as 0; texture() with filterSampler is
 * bilinear with fp32 weights and clamp to edge, (t00 (1 - a) + t10 a) (1 - b) + (t01 (1 - a) + t11 a) b; everything else is §4.14's.
 * Each single-pass entry point enqueues one launch, nv_bloom 2 * levels - 1 of them (no allocation, no synchronisation: capturable).
 * NV_EINVAL: a NULL ctx, pointer or desc, an image width or height 0 or above 16384, a pointer that is not 4-byte aligned, a desc that is not
 * what nv_bloom_desc_init gives for the image size (for the per-level passes: for its own width and height), a level out of range, a
 * radius that is not finite or is negative.  A refused call launches nothing. */
#define NV_BLOOM_MAX_LEVELS 8
typedef struct NvBloomDesc
{
	uint32_t width;  /* level 0: (image width + 1) / 2 */
	uint32_t height; /* level 0: (image height + 1) / 2 */
	uint32_t levels; /* min(8, nv_image_mip_levels(width, height)) */
	uint32_t levelOffset[NV_BLOOM_MAX_LEVELS]; /* in texels; entries from `levels` on hold totalTexels */
	uint32_t totalTexels;
} NvBloomDesc;

/* bloom.comp.glsl:29-46, pass 0: the emissive term of the full-resolution gbuffer0 (width x height, as nv_visibility_attributes packs it),
 * four bilinear samples a quarter texel around each half-resolution texel, into level 0 */
int nv_bloom_extract(nv_context* ctx, void* stream, const uint32_t* d_gbuffer0, uint32_t width, uint32_t height, uint32_t* d_bloom,
                     const NvBloomDesc* desc);
/* bloom.comp.glsl:47-77, pass 1 (QUALITY 1): the 13-tap downsample of level - 1 into level, 1 <= level < desc->levels */
int nv_bloom_downsample(nv_context* ctx, void* stream, uint32_t* d_bloom, const NvBloomDesc* desc, uint32_t level);
/* bloom.comp.glsl:78-107, pass 2 (QUALITY 1): the 9-tap tent of level + 1, `radius` texels of `level` wide, added to level IN PLACE (an
 * invocation reads and writes its own texel of `level` only), level <= desc->levels - 2 */
int nv_bloom_upsample(nv_context* ctx, void* stream, uint32_t* d_bloom, const NvBloomDesc* desc, uint32_t level, float radius);
/* src/niagara.cpp:1873-1901: extract, downsample 1 .. levels - 1, upsample levels - 2 .. 0 with radius 2.0 — by definition the result of
 * the single-pass entry points called in that order (NV_OPT_BLOOM_FUSED_TAIL fuses launches, not results) */
int nv_bloom(nv_context* ctx, void* stream, const uint32_t* d_gbuffer0, uint32_t width, uint32_t height, uint32_t* d_bloom, const NvBloomDesc* desc);
/* final.comp.glsl:37-80 complete: nv_shade_final plus texture(bloomImage, uv).rgb * 0.1 from level 0 of d_bloom (read only),
 * outputColor = ((albedo * lit + spec) + emissive) + bloom * 0.1 per channel.  NV_EINVAL as nv_shade_final, and for d_bloom / desc as above */
int nv_shade_final_bloom(nv_context* ctx, void* stream, const NvShadeData* shade, const uint32_t* d_gbuffer0, const uint32_t* d_gbuffer1,
                         const float* d_depth, const uint8_t* d_shadow /* optional */, uint32_t* d_color, uint32_t width, uint32_t height,
                         const uint32_t* d_bloom, const NvBloomDesc* desc);

/* ---- ray-traced sun shadows (replaces shadow.comp.glsl and the BLAS / TLAS of src/scenert.cpp) ----
 * gfx950 has no ray accelerator and HIP no acceleration-structure API: the scene is a software BVH built on the host at load time
 * (nv_rt_scene_build), kept on the device by the context (nv_rt_scene_upload) and walked by one kernel (nv_shadow_trace).
 *
 * The RESULT is defined without a BVH (tests/shadow_ref.c is the brute-force restatement): per invocation of shadow.comp.glsl:125-161 the ray
 * origin = wpos (final.comp.glsl's arithmetic), direction = normalize(sunDirection + jitter), tmin = 1e-2, tmax = 1e3, and the byte is 0 when
 * ANY casting triangle passes the triangle test T for it, 255 otherwise.  T is the watertight test of Woop, Benthin and Wald (JCGT 2013) with
 * its fp64 fallback, every fp32 operation one IEEE operation in a fixed order (niagara_amd/csrc/rtmath.h); two triangles
 * that share an edge cannot both miss a ray that crosses it.  No face culling.  A ray with a non-finite origin or direction component (a sky
 * pixel: depth 0 gives wposh.w == 0; a zero sun vector) hits nothing and stores 255: Vulkan leaves it undefined, this is the defined semantic.
 * Casting instances (src/scenert.cpp:504-518, src/niagara.cpp:1803): draw i casts iff meshIndex < meshCount, position, orientation and scale
 * are finite, scale > 0, and postPass == 0 (quality 0) or postPass <= 1 (quality 1).  Its triangles are those of meshes[meshIndex].lods[lodRT]
 * (none when lodRT >= 8 or >= lodCount): corner k of triangle t < indexCount / 3 is vertices[vertexOffset + indices[indexOffset + 3 t + k]],
 * the fp16 position converted to fp32; a triangle with an index position >= indexCapacity or a corner >= vertexCapacity is left out
 * (nv_rasterdepth_indexed's rule).  The ray is taken into object space with t preserved: o' = rotateQuat(o - position, conj(q)) / scale,
 * d' = rotateQuat(d, conj(q)) / scale.
 * nv_shadow_trace samples no textures: its quality 1 sees alpha = 1, and a post-pass material with a cut-out albedo texture casts the shadow of its
 * whole triangles.  nv_shadow_trace_textured (below) runs the alpha test of shadow.comp.glsl:86-123.  NOT MODELLED by either:
 * opacity micromaps.  For quality 0 the reference's outcome for non-opaque instances depends on its driver's
 * traversal order (one rayQueryProceedEXT, nothing confirmed): post-pass draws are defined as non-casters there.  Animation: when draws move,
 * nv_rt_tlas_build (below) rebuilds the TLAS on the device from the rewritten draw records, in place of the reference's
 * buildTLAS(MODE_UPDATE) (src/niagara.cpp:1396, :1482).  The mask does not depend on which TLAS is walked.  The keyframe evaluation that
 * rewrites them (src/niagara.cpp:1368-1409) is nv_animate_draws (below).  Not modelled: a BLAS rebuild (geometry is static),
 * lights as shadow casters. */

/* shadow.comp.glsl:26-35, src/niagara.cpp:269-278; 96 B (92 used), align 16.  inverseViewProjection is column-major */
typedef struct NvShadowData
{
	float sunDirection[3];
	float sunJitter;
	float inverseViewProjection[16];
	float imageSize[2];
	int32_t checkerboard;
	uint32_t _pad;
} NvShadowData;

typedef struct NvRtSceneStats
{
	uint32_t bytes;
	uint32_t instances;    /* casting draws (postPass <= 1) whose mesh has triangles */
	uint32_t tlasNodes, tlasLeaves, tlasMaxLeaf;
	uint32_t blasCount;    /* meshes with triangles */
	uint32_t blasNodes, blasLeaves, blasMaxLeaf;
	uint32_t triangles;    /* kept triangles of all BLAS */
} NvRtSceneStats;

/* Host only, no context.  Builds the scene blob: one BLAS per mesh that has triangles and one TLAS over the casting draws, both binary BVHs
 * in depth-first preorder with skip links (a box hit goes to i + 1, a miss or a leaf to skip[i] > i), median split, leaves of at most 4
 * triangles / 1 instance.  The blob is relocatable (offsets only, 16-byte aligned sections) and deterministic.  out == NULL: *bytes = the size
 * needed.  Otherwise *bytes is the room at `out` (16-byte aligned) on entry and the bytes written on return.  NV_EINVAL: a NULL bytes, a NULL
 * array with a non-zero count, too little room, a misaligned out, counts that do not fit the blob's 32-bit fields. */
int nv_rt_scene_build(const NvMesh* meshes, uint32_t meshCount, const uint32_t* indices, uint32_t indexCapacity, const NvVertex* vertices,
                      uint32_t vertexCapacity, const NvMeshDraw* draws, uint32_t drawCount, void* out, uint64_t* bytes);
/* NV_OK, or NV_EINVAL when the blob is not one nv_rt_scene_trace_host / nv_shadow_trace can walk safely: header and section bounds, every skip
 * > its index and <= the count, leaf ranges inside their arrays, BLAS references valid */
int nv_rt_scene_validate(const void* blob, uint64_t bytes);
int nv_rt_scene_stats(const void* blob, uint64_t bytes, NvRtSceneStats* out);
/* the traversal nv_shadow_trace runs, on the CPU (the same text, rtmath.h): 1 = occluded, 0 = not; NV_EINVAL for a NULL pointer or quality
 * outside 0..1.  The blob must have passed nv_rt_scene_validate. */
int nv_rt_scene_trace_host(const void* blob, const float origin[3], const float dir[3], float tmin, float tmax, int quality);
/* the same for `count` rays (origins, dirs: count x 3 floats): out[i] = 0 (occluded) or 255, the mask's bytes */
int nv_rt_scene_trace_host_rays(const void* blob, const float* origins, const float* dirs, uint64_t count, float tmin, float tmax, int quality,
                                uint8_t* out);
/* Validates the blob and keeps a context-owned device copy (allocates and synchronises, like nv_reserve: load time); (NULL, 0) drops it */
int nv_rt_scene_upload(nv_context* ctx, void* stream, const void* blob, uint64_t bytes);
/* shadow.comp.glsl over W' x height invocations, W' = checkerboard > 0 ? (width + 1) / 2 : width: with checkerboard the invocation (x, y) owns
 * the texel (2 x + ((y ^ checkerboard) & 1), y) and the texels of the other parity keep their bytes (nv_shadow_fill fills them); a store at
 * x >= width is dropped.  d_depth: width * height fp32, d_shadow: width * height u8.  Enqueues one launch (no allocation, no synchronisation:
 * it can be captured).  NV_EINVAL: no uploaded scene, a NULL pointer, width or height 0 or above 16384, shadow->imageSize not (width, height),
 * quality outside 0..1, a depth pointer that is not 4-byte aligned. */
int nv_shadow_trace(nv_context* ctx, void* stream, const NvShadowData* shadow, const float* d_depth, uint8_t* d_shadow, uint32_t width,
                    uint32_t height, int quality);

/* ---- the alpha-tested trace (shadowTraceTransparent, shadow.comp.glsl:86-123; niagara_amd/csrc/rtalpha.h is the text) ----
 * Every rule of nv_shadow_trace holds: ray set-up, casting rule, object-space ray, T with its fp64 fallback, tmin / tmax, checkerboard ownership,
 * non-finite rays lit; one IEEE fp32 operation per source operation, no contraction, sums left to right.  tests/shadow_alpha_ref.c is the
 * brute-force restatement.
 * Quality 0: nv_shadow_trace's bytes.  Quality 1: the byte is 0 iff some casting instance (postPass <= 1) has a triangle that T accepts for the
 * ray and that is CONFIRMED.  A triangle of a postPass == 0 instance is always confirmed (fillInstanceRT sets FORCE_OPAQUE there,
 * src/scenert.cpp:516: the loop never sees it, whatever its material).  A triangle of a postPass == 1 instance is confirmed iff alpha >= 0.5f (a
 * NaN alpha does not confirm), where, with draw = d_draws[instance.drawId], material = d_materials[draw.materialIndex] and tex =
 * material.albedoTexture: alpha = 1 when drawId >= drawCount, materialIndex >= materialCount, tex == 0 (:116), tex >= textureCount, or the
 * descriptor's chain does not lie inside texelWords (a texture the pass cannot sample is absent, as in nv_visibility_attributes_textured; no
 * load leaves the caller's buffers for any input bits).  Otherwise, with T's U, V, W and det (after the fp64 fallback where T took it):
 * b1 = V / det, b2 = W / det, w0 = (1 - b1) - b2, per component uv = (uv0 w0 + uv1 b1) + uv2 b2 (:113) with uvk the fp16 tu, tv of the
 * triangle's corner k converted exactly, and alpha = textureLod(textures[tex], uv, 0).w by the sampler of §4.18: REPEAT, bilinear, level 0 only.
 * The result is an OR over the accepted triangles: it does not depend on the order of the walk (what TerminateOnFirstHit with a confirming loop
 * computes).  Vulkan leaves the bits of the barycentrics to the implementation: the formula above is this library's definition.
 *
 * The scene must carry the texcoords: nv_rt_scene_build_textured is nv_rt_scene_build (arguments, size protocol, errors) whose triangles hold
 * in corner k's w word the BITS tu | tv << 16 of that corner's vertex, and whose header's flags word (the reserved word of nv_rt_scene_build's
 * blob, 0 there) has bit 0 set.  Everything else is byte for byte nv_rt_scene_build's blob.  nv_rt_scene_validate accepts flags 0 or 1 and
 * refuses any other bit; any bit pattern in a w word is safe.  nv_rt_tlas_build_host, nv_rt_scene_reserve_dynamic, nv_rt_tlas_build and
 * nv_rt_scene_download keep the flag and the w words. */
int nv_rt_scene_build_textured(const NvMesh* meshes, uint32_t meshCount, const uint32_t* indices, uint32_t indexCapacity, const NvVertex* vertices,
                               uint32_t vertexCapacity, const NvMeshDraw* draws, uint32_t drawCount, void* out, uint64_t* bytes);
/* the traversal nv_shadow_trace_textured runs, on the CPU (the same text), for `count` rays: out[i] = 0 (occluded) or 255.  draws, materials,
 * textures (entry 0 reserved) and texels are host arrays.  The blob must have passed nv_rt_scene_validate.  NV_EINVAL: a NULL blob, a NULL
 * array with a non-zero count, quality outside 0..1, a blob without the texcoord flag. */
int nv_rt_scene_trace_host_textured_rays(const void* blob, const float* origins, const float* dirs, uint64_t count, float tmin, float tmax, int quality,
                                         const NvMeshDraw* draws, uint32_t drawCount, const NvMaterial* materials, uint32_t materialCount,
                                         const NvTextureDesc* textures, uint32_t textureCount, const uint32_t* texels, uint64_t texelWords, uint8_t* out);
/* Test accessor: the pass's four-tap alpha (fourTap) and textureLod(..., 0).w of the full sampler (sampler) of one texture at `count` uv pairs;
 * the two must agree bit for bit.  NV_EINVAL: a NULL pointer, a descriptor whose chain does not lie inside texelWords. */
int nv_rt_alpha_sample_host(const NvTextureDesc* desc, const uint32_t* texels, uint64_t texelWords, const float* uv, uint64_t count, float* fourTap,
                            float* sampler);
/* nv_shadow_trace with the alpha test.  d_draws: the draw array the scene's instances index (the one nv_rt_scene_build_textured or the last
 * nv_rt_tlas_build read); d_materials, d_textures (entry 0 reserved), d_texels: as nv_visibility_attributes_textured takes them.  Quality 0
 * dispatches nv_shadow_trace's kernel; quality 1 enqueues one launch of its own (no allocation, no synchronisation: it can be captured).
 * NV_EINVAL, with nothing launched: everything nv_shadow_trace refuses, an uploaded scene without the texcoord flag, a NULL array with a
 * non-zero count, a misaligned pointer (16 bytes: draws, materials, descriptors; 4: texels). */
int nv_shadow_trace_textured(nv_context* ctx, void* stream, const NvShadowData* shadow, const float* d_depth, uint8_t* d_shadow, uint32_t width,
                             uint32_t height, int quality, const NvMeshDraw* d_draws, uint32_t drawCount, const NvMaterial* d_materials,
                             uint32_t materialCount, const NvTextureDesc* d_textures, uint32_t textureCount, const uint32_t* d_texels,
                             uint64_t texelWords);

/* nv_shadow_trace_blocks: nv_shadow_trace_textured (the shadow passes, below) over a block-resident set — its parameters, rules and errors,
 * with NvTextureBlockDesc descriptors, d_blocks (16-byte aligned) and units16; the four alpha taps of a candidate are decoded from their
 * blocks, alpha alone.  The mask equals nv_shadow_trace_textured's over the decoded form of the same set byte for byte. */
int nv_shadow_trace_blocks(nv_context* ctx, void* stream, const NvShadowData* shadow, const float* d_depth, uint8_t* d_shadow, uint32_t width,
                           uint32_t height, int quality, const NvMeshDraw* d_draws, uint32_t drawCount, const NvMaterial* d_materials,
                           uint32_t materialCount, const NvTextureBlockDesc* d_textures, uint32_t textureCount, const void* d_blocks,
                           uint64_t units16);


/* ---- the TLAS rebuilt for moving draws (niagara_amd/csrc/rttlas.h is the definition) ----
 * The rebuilt TLAS is a function of the blob's BLAS side and the current draw array alone: the instances are the draws that cast by the rule
 * above (re-derived at every rebuild), each with nv_rt_scene_build's fp64 box; they are ordered by (key, drawId), key the 30-bit Morton code of
 * the box middles quantised to 1024 cells per axis of the middles' own range; the tree is the binary radix tree of the strings key << 32 | k
 * over the sorted instances k, laid out in preorder with skip links: 2 n - 1 nodes for n instances, leaf k holds instance k.
 *
 * Host twin, no context: a canonical blob (nv_rt_scene_build's section order and packing) whose BLAS table, BLAS nodes and triangles are copied
 * from `blob` and whose TLAS, instances, padOrigin and drawCount are rebuilt from `draws`.  The size protocol of nv_rt_scene_build.  NV_EINVAL:
 * a blob nv_rt_scene_validate refuses, a NULL bytes, a NULL array with a non-zero count, too little room, a misaligned out, drawCount above
 * 2^29 - 1. */
int nv_rt_tlas_build_host(const void* blob, uint64_t blobBytes, const NvMeshDraw* draws, uint32_t drawCount, void* out, uint64_t* bytes);
/* Load time, like nv_reserve (allocates and synchronises): re-houses the uploaded scene in one allocation that holds the static blob, room for
 * 2 maxDraws TLAS nodes and maxDraws instances, and the rebuild's scratch.  The device header keeps pointing at the static TLAS until the first
 * nv_rt_tlas_build.  NV_EINVAL: no uploaded scene, maxDraws 0 or above 2^29 - 1, an allocation that does not fit the blob's 32-bit offsets
 * (4 GiB).  A later nv_rt_scene_upload drops the reservation: the scene is static again and nv_rt_tlas_build refuses. */
int nv_rt_scene_reserve_dynamic(nv_context* ctx, void* stream, uint32_t maxDraws);
/* Rebuilds the TLAS from d_draws[0, drawCount), read ON THE DEVICE when the launches run.  Only enqueues on `stream` (two memset nodes and
 * kernel launches; no allocation, no synchronisation, no read-back: it can be captured); the last launch rewrites tlasNodes, instances, tlasOff,
 * instOff, padOrigin and drawCount of the device header, and nv_shadow_trace calls behind it in stream order walk the new TLAS.  drawCount 0 or
 * no casting draw: tlasNodes = 0, every ray is lit.  NV_EINVAL with nothing launched: no reservation, drawCount above the reserved maxDraws, a
 * NULL d_draws with a non-zero count, a d_draws that is not 4-byte aligned. */
int nv_rt_tlas_build(nv_context* ctx, void* stream, const NvMeshDraw* d_draws, uint32_t drawCount);
/* Test and tooling accessor (synchronises): the context's current scene as a canonical blob in nv_rt_tlas_build_host's packing, with the size
 * protocol of nv_rt_scene_build.  NV_EINVAL: no scene, a NULL bytes, a misaligned out, too little room. */
int nv_rt_scene_download(nv_context* ctx, void* stream, void* out, uint64_t* bytes);

/* ---- keyframe animation on the device (src/niagara.cpp:1368-1409; niagara_amd/csrc/animmath.h is the text) ----
 * Per animation, in the reference's statements: index = (time - startTime) / period in fp64; index < 0 skips the animation; index =
 * fmod(index, keyframeCount); index0 = int(index) % keyframeCount, index1 = (index0 + 1) % keyframeCount; t = float(index - floor(index)); with
 * k0 / k1 = keyframes[keyframeOffset + index0 / index1]: position = mix(k0.translation, k1.translation, t), scale = mix(k0.scale, k1.scale, t),
 * orientation = slerp(k0.rotation, k1.rotation, t) of the draw drawIndex >= 0, and position = mix(...) of the light lightIndex >= 0.
 * mix(x, y, a) = x * (1 - a) + y * a.  slerp as glm publishes it: cosTheta = (x.w y.w + x.x y.x) + (x.y y.y + x.z y.z); z = cosTheta < 0 ? -y : y
 * (and cosTheta = -cosTheta); cosTheta > 1 - FLT_EPSILON: the component-wise mix; otherwise (sin((1 - a) angle) x + sin(a angle) z) / sin(angle)
 * with angle = acos(cosTheta).  Every fp32 operation is one IEEE operation in that order, no contraction: the device and nv_animate_draws_host
 * compile the same text and agree bit for bit except in sinf / acosf, whose libraries differ (bound: DESIGN.md §4.22).  glm itself is not part
 * of the reference's snapshot: the parity of mix / slerp is "glm's published definition", unpinned, as for nv_meshlet_bounds.
 * Defined where the reference is not: an index that is not finite (time - startTime overflowing) skips the animation.
 * ORDER: the reference applies the animations in array order, so of two that name the same draw (or light) the last one wins.  A lane per
 * animation cannot keep that order, and loadScene never produces such a pair: duplicates are REFUSED by the validator instead. */
enum
{
	NV_ANIM_OK = 0,
	NV_ANIM_NO_KEYFRAMES = 1,    /* keyframeCount == 0 */
	NV_ANIM_KEYFRAME_RANGE = 2,  /* keyframeOffset + keyframeCount beyond the table (or a keyframeCount above 2^31 - 1: int(index)) */
	NV_ANIM_PERIOD = 3,          /* period not finite or <= 0 (the reference divides by it); startTime not finite */
	NV_ANIM_DRAW_INDEX = 4,      /* drawIndex >= drawCount */
	NV_ANIM_LIGHT_INDEX = 5,     /* lightIndex >= lightCount */
	NV_ANIM_DUPLICATE_DRAW = 6,  /* two animations with the same drawIndex >= 0 */
	NV_ANIM_DUPLICATE_LIGHT = 7  /* two animations with the same lightIndex >= 0 */
};
/* Host only.  NV_OK, or NV_EINVAL with *out_reason = the NV_ANIM_* reason and *out_index = the first animation it holds for (either may be
 * NULL).  The reasons are tried in the order of the enum per animation, the duplicates after every animation has passed the others. */
int nv_animation_validate_host(const NvAnimation* animations, uint32_t animationCount, uint32_t keyframeCount, uint32_t drawCount,
                               uint32_t lightCount, uint32_t* out_reason, uint32_t* out_index);
/* Host only: the time statements alone (tests), one sample per (animations[which[i]], times[i]), i < n: out_skipped[i] = 1 when the animation
 * is skipped at that time, else 0 with the keyframe pair and t (the outputs of a skipped sample are left alone).  NV_EINVAL: a NULL pointer with
 * n > 0, a non-finite time, a sampled animation with keyframeCount 0 or above 2^31 - 1. */
int nv_animation_phase_host(const NvAnimation* animations, const uint32_t* which, const double* times, uint64_t n, uint8_t* out_skipped,
                            uint32_t* out_index0, uint32_t* out_index1, float* out_t);
/* The host twin of nv_animate_draws (the same text): validates like nv_upload_animations, then rewrites draws / lights in place.  draws or
 * lights may be NULL (those targets are skipped; the indices are still validated against the counts).  NV_EINVAL: a refused table, a
 * non-finite time, a NULL array with a non-zero animationCount. */
int nv_animate_draws_host(double time, const NvAnimation* animations, uint32_t animationCount, const NvKeyframe* keyframes,
                          uint32_t keyframeCount, NvMeshDraw* draws, uint32_t drawCount, NvLight* lights, uint32_t lightCount);
/* Load time, like nv_rt_scene_upload (allocates, copies and synchronises the stream; a grow frees the old copies after a device synchronise,
 * as nv_upload_draws does): validates the HOST arrays (nv_animation_validate_host; NV_EINVAL) and keeps context-owned device copies, the
 * 24-byte records re-laid into one 16-byte and one 8-byte stream.  h_animations == NULL with animationCount 0 drops them (a non-NULL pointer
 * with count 0 uploads an empty table).  drawCount / lightCount are the bounds
 * the indices were checked against: nv_animate_draws refuses smaller buffers. */
int nv_upload_animations(nv_context* ctx, void* stream, const NvAnimation* h_animations, uint32_t animationCount, const NvKeyframe* h_keyframes,
                         uint32_t keyframeCount, uint32_t drawCount, uint32_t lightCount);
/* One launch, a lane per uploaded animation: words 0-7 of the target draws of d_draws (two 16-byte stores; words 8-11 are never written) and,
 * when d_lights is given, the 12 position bytes of the target lights (d_lights == NULL skips light targets).  When d_draws lies in the buffer
 * registered by nv_upload_draws, the same lane also rewrites that draw's entry of the cull mirror (the statements of nv_update_draws, from the
 * draw's own meshIndex word): no nv_update_draws is needed behind it.  Only enqueues (no allocation, no synchronisation: it can be captured);
 * `time` travels BY VALUE in the launch, so a replayed graph repeats the captured time.  An uploaded table of 0 animations: NV_OK, nothing
 * enqueued.  NV_EINVAL with nothing launched: a non-finite time, drawCount / lightCount (with d_lights) below the bounds given to
 * nv_upload_animations, a NULL d_draws with a non-zero bound, d_draws not 16-byte aligned, d_lights not 4-byte aligned.  NV_ESTATE: no uploaded
 * table (never uploaded, or dropped). */
int nv_animate_draws(nv_context* ctx, void* stream, double time, NvMeshDraw* d_draws, uint32_t drawCount, NvLight* d_lights, uint32_t lightCount);

/* ---- host helpers mirroring src/niagara.cpp / src/resources.cpp (no device work) ---- */
uint32_t nv_previous_pow2(uint32_t v);                        /* src/niagara.cpp:439-447 */
uint32_t nv_image_mip_levels(uint32_t width, uint32_t height); /* src/resources.cpp:280-292 */
/* fills width/height/levels/mipOffset/totalTexels from the depth target size; d_base untouched */
int nv_pyramid_desc_init(NvPyramidDesc* desc, uint32_t depthWidth, uint32_t depthHeight);
/* src/niagara.cpp:1331-1333: the bloom target of a width x height image (every field; NV_EINVAL: NULL, a size 0 or above 16384) */
int nv_bloom_desc_init(NvBloomDesc* desc, uint32_t width, uint32_t height);
/* the multiplier with which the kernels divide by a launch constant d (grid sizes): mulhi(n, m) >> 7 == n / d for every
 * n < 2^39 / d; 0 (the kernels then divide) for d outside 256 .. 8192.  Exported so that the bound can be tested. */
uint32_t nv_division_magic(uint32_t d);
/* src/niagara.cpp:424-437,1487-1516: CullData from a camera (position, orientation quat xyzw, fovY,
 * znear), viewport, draw distance and pyramid size; flags are left 0 for the caller to set. */
int nv_build_cull_data(NvCullData* out, const float cameraPosition[3], const float cameraOrientation[4],
                       float fovY, float znear, float drawDistance, uint32_t viewportWidth,
                       uint32_t viewportHeight, uint32_t pyramidWidth, uint32_t pyramidHeight,
                       uint32_t drawCount, int debugLodStep);
/* src/niagara.cpp:1917-1922: the ShadeData of nv_shade_final from the frame's globals (projection, cullData.view): cameraPosition,
 * sunDirection, shadowsEnabled, imageSize = (width, height) and inverseViewProjection = inverse(projection * view), the product and the
 * inverse (adjugate / determinant) evaluated in fp64 from the fp32 entries and rounded once to fp32.  The reference uses glm's fp32 inverse,
 * which is not vendored in its snapshot: the matrix is an INPUT of the pass, not part of its parity.  NV_EINVAL: a NULL pointer, width or
 * height 0, a singular or non-finite product. */
int nv_build_shade_data(NvShadeData* out, const NvGlobals* globals, const float cameraPosition[3], const float sunDirection[3],
                        int shadowsEnabled, uint32_t width, uint32_t height);
/* src/niagara.cpp:1806-1812: the ShadowData of nv_shadow_trace; inverseViewProjection exactly as nv_build_shade_data computes it (the same
 * code), imageSize = (width, height).  niagara passes sunJitter = 1e-2 when the shadow blur is on, else 0.  NV_EINVAL as nv_build_shade_data */
int nv_build_shadow_data(NvShadowData* out, const NvGlobals* globals, const float sunDirection[3], float sunJitter, int checkerboard,
                         uint32_t width, uint32_t height);
/* src/niagara.cpp:1002-1020: per-draw meshletVisibilityOffset prefix; returns the slot count
 * through out_slots (meshletVisibility bytes = (slots+31)/32*4) and the postPass mask. */
int nv_assign_visibility_offsets(NvMeshDraw* draws, uint32_t drawCount, const NvMesh* meshes,
                                 uint32_t meshCount, uint32_t* out_slots, uint32_t* out_postPassMask);
/* The names of the triangles of indexed draws (nv_rasterdepth_indexed_visibility): offsets[0] = 0, offsets[d + 1] =
 * offsets[d] + span(d), span(d) = the maximum of lods[l].indexCount / 3 over l < min(lodCount, NV_MAX_LODS) of the draw's mesh, 0 when
 * meshIndex >= meshCount.  `offsets` holds drawCount + 1 entries.  NV_EINVAL: a NULL array with a non-zero count, NULL offsets, or a total
 * above 2^34 - 2 (the array is written all the same). */
int nv_assign_triangle_offsets(const NvMeshDraw* draws, uint32_t drawCount, const NvMesh* meshes, uint32_t meshCount,
                               uint64_t* offsets /* drawCount + 1 */);
/* src/niagara.cpp:449-481,969-998: PCG32-seeded synthetic scene (state 0x42) */
int nv_synth_draws(NvMeshDraw* draws, uint32_t drawCount, uint32_t meshCount, float sceneRadius);

/* src/scene.cpp:207-220: Mesh.center = mean of the positions (fp32, accumulated in array order), Mesh.radius = the
 * largest distance from it — the bounding sphere drawcull tests (the part of the asset pipeline that is the reference's
 * own arithmetic; meshlet bounds are meshoptimizer's).  positions = vertexCount x {x, y, z}. */
int nv_mesh_bounds(const float* positions, uint32_t vertexCount, float out_center[3], float* out_radius);

/* ---- multi-GPU helper: contiguous shard of `total` units for `rank` ---- */
void nv_shard_range(uint64_t total, uint32_t rank, uint32_t world, uint64_t* begin, uint64_t* end);
/* Where the next nv_clustercull calls also leave {0, d_count4[0], final cluster count} as three u64 — the words
 * nv_pack_counts(NULL, d_count4, d_clusterCount4, d_out3) would write, from the scatter launch that computes the count,
 * so a sharded caller feeds its all-reduce without one more launch per pass.  NULL (the default) turns it off. */
int nv_set_counts_sink(nv_context* ctx, uint64_t* d_out3);
/* packs {count4a[0], count4b[0], count4c[0]} (any may be NULL -> 0) into d_out[3] as u64,
 * the payload of the one ncclAllReduce(sum) per phase */
int nv_pack_counts(nv_context* ctx, void* stream, const uint32_t* d_countA, const uint32_t* d_countB,
                   const uint32_t* d_countC, uint64_t* d_out3);

/* ---- scene cache ingestion ----
 * niagara's `.cache` file (src/scenecache.cpp: header :16-55, section order :163-203, load-time checks :273-293) holds
 * the three arrays the visibility path consumes — Meshlet, Mesh, MeshDraw — as RAW struct arrays even in compressed mode
 * (:170, :181, :183); only the vertex / index / meshlet-data / RT-vertex streams are meshopt-coded, and their byte sizes
 * are in the header, so they can be stepped over without a decoder.  nv_scenecache_info validates the header like
 * loadSceneCache does (magic 'SCNC', version 7, MESH_MAXVTX / MESH_MAXTRI; hashMeta, clrtMode and ommStates are
 * returned for the caller to compare with its own settings) and locates the arrays; nv_scenecache_read copies them
 * out (any destination may be NULL).  Host-only: no device work. */
typedef struct NvSceneCacheInfo
{
	uint32_t version, compressed, clrtMode, ommStates;
	uint64_t hashMeta;
	uint32_t meshletMaxVertices, meshletMaxTriangles;
	uint32_t vertexCount, indexCount, meshletCount, meshletdataCount, meshletvtx0Count, meshCount;
	uint32_t materialCount, drawCount, texturePathCount, lightCount, animationCount, keyframeCount;
	float cameraPosition[3];    /* Camera (src/scene.h:111-117) */
	float cameraOrientation[4]; /* quat x, y, z, w */
	float cameraFovY, cameraZnear;
	float sunDirection[3];
	uint64_t fileSize;
	uint64_t vertexOffset, indexOffset, meshletOffset, meshletdataOffset, meshOffset, drawOffset; /* byte offsets in the file */
	uint64_t vertexBytes, indexBytes, meshletdataBytes; /* stored (possibly compressed) sizes of those streams */
} NvSceneCacheInfo;
int nv_scenecache_info(const char* path, NvSceneCacheInfo* out);
int nv_scenecache_read(const char* path, const NvSceneCacheInfo* info, NvMesh* meshes, NvMeshlet* meshlets, NvMeshDraw* draws);
/* the info->texturePathCount fixed 256-byte, NUL-padded records the file ends with (src/scenecache.cpp:192-197,355): textures[i + 1] is the
 * DDS file paths[i] names.  The records sit behind sections this reader does not size (lights, animations, opacity micromaps), so they are
 * taken from the END of the file; every record is NUL-terminated on return.  NV_EFORMAT: the file is too short to hold them. */
int nv_scenecache_texture_paths(const char* path, const NvSceneCacheInfo* info, char (*paths)[256]);
/* the info->lightCount Light, info->animationCount Animation and info->keyframeCount Keyframe records, three raw arrays that follow the draws
 * directly (src/scenecache.cpp:183-186): they start at info->drawOffset + drawCount * 48.  Any destination may be NULL.  NV_EFORMAT: the
 * file is too short to hold them; NV_EIO: it cannot be read. */
int nv_scenecache_animations(const char* path, const NvSceneCacheInfo* info, NvLight* lights, NvAnimation* animations, NvKeyframe* keyframes);

/* ---- verification probe (tests only): per-meshlet scalar intermediates of the cluster cull
 * (view-space centre xyz, radius, cone lhs, cone rhs, aabb[4], mip level, sampled depth,
 * depthSphere, flags) = 16 floats per lane, for the <=1-ULP scalar parity tests. */
int nv_probe_cluster_scalars(nv_context* ctx, void* stream, const NvCullData* cull,
                             const NvMeshTaskCommand* d_commands, uint32_t commandCount,
                             const NvMeshDraw* d_draws, const NvMeshlet* d_meshlets,
                             const NvPyramidDesc* pyramid, float* d_out16);

#ifdef __cplusplus
}

static_assert(sizeof(NvMeshlet) == 24, "Meshlet layout (src/scene.h:10-23)");
static_assert(sizeof(NvMeshDraw) == 48, "MeshDraw layout (src/scene.h:39-49)");
static_assert(sizeof(NvLight) == 32 && sizeof(NvKeyframe) == 32 && sizeof(NvAnimation) == 24, "Light / Keyframe / Animation layouts (src/scene.h:51-58, 119-136)");
static_assert(sizeof(NvMeshLod) == 20, "MeshLod layout (src/scene.h:68-75)");
static_assert(sizeof(NvMesh) == 208, "Mesh layout (src/scene.h:77-93)");
static_assert(offsetof(NvMesh, lods) == 48, "Mesh.lods offset");
static_assert(sizeof(NvMeshDrawCommand) == 24, "MeshDrawCommand layout (src/niagara.cpp:227-231)");
static_assert(sizeof(NvMeshTaskCommand) == 20, "MeshTaskCommand layout (src/niagara.cpp:233-240)");
static_assert(sizeof(NvCullData) == 144, "CullData layout (src/niagara.cpp:242-260)");
static_assert(offsetof(NvCullData, P00) == 64 && offsetof(NvCullData, frustum) == 80, "CullData offsets");
static_assert(offsetof(NvCullData, lodTarget) == 96 && offsetof(NvCullData, drawCount) == 108, "CullData offsets");
static_assert(offsetof(NvCullData, cullingEnabled) == 112 && offsetof(NvCullData, postPass) == 132, "CullData offsets");
static_assert(sizeof(NvVertex) == 16, "Vertex layout (src/shaders/mesh.h:3-9)");
static_assert(sizeof(NvGlobals) == 224 && offsetof(NvGlobals, cullData) == 64 && offsetof(NvGlobals, screenWidth) == 208, "Globals layout (src/shaders/mesh.h:46-51)");
static_assert(sizeof(NvTriangleMask) == 16, "one mask per grid slot");
static_assert(sizeof(NvVisRecord) == 16, "one 16-byte store per pixel");
static_assert(sizeof(NvMaterial) == 64 && offsetof(NvMaterial, diffuseFactor) == 16 && offsetof(NvMaterial, emissiveFactor) == 48, "Material layout (src/scene.h:25-37)");
static_assert(sizeof(NvPixelAttributes) == 64 && offsetof(NvPixelAttributes, drawId) == 28 && offsetof(NvPixelAttributes, materialIndex) == 60, "four 16-byte stores per pixel");
static_assert(sizeof(NvShadeData) == 112 && offsetof(NvShadeData, sunDirection) == 16 && offsetof(NvShadeData, shadowsEnabled) == 28 &&
              offsetof(NvShadeData, inverseViewProjection) == 32 && offsetof(NvShadeData, imageSize) == 96, "ShadeData layout (src/niagara.cpp:280-290)");
static_assert(sizeof(NvShadowData) == 96 && offsetof(NvShadowData, sunJitter) == 12 && offsetof(NvShadowData, inverseViewProjection) == 16 &&
              offsetof(NvShadowData, imageSize) == 80 && offsetof(NvShadowData, checkerboard) == 88, "ShadowData layout (src/niagara.cpp:269-278)");
static_assert(sizeof(NvRtSceneStats) == 40, "NvRtSceneStats is mirrored by niagara_amd/_lib.py");
static_assert(sizeof(NvBloomDesc) == 48 && offsetof(NvBloomDesc, levels) == 8 && offsetof(NvBloomDesc, levelOffset) == 12 &&
              offsetof(NvBloomDesc, totalTexels) == 44, "NvBloomDesc is mirrored by niagara_amd/_lib.py and niagara_amd/layouts.py");
static_assert(sizeof(NvTextureDesc) == 16 && offsetof(NvTextureDesc, width) == 4 && offsetof(NvTextureDesc, levels) == 12, "NvTextureDesc is mirrored by niagara_amd/layouts.py");
static_assert(sizeof(NvTextureBlockDesc) == 16 && offsetof(NvTextureBlockDesc, width) == 4 && offsetof(NvTextureBlockDesc, height) == 8 && offsetof(NvTextureBlockDesc, levelsFormat) == 12, "NvTextureBlockDesc is mirrored by niagara_amd/layouts.py");
static_assert(sizeof(NvDdsInfo) == 152 && offsetof(NvDdsInfo, payloadBytes) == 24 && offsetof(NvDdsInfo, levelOffset) == 32, "NvDdsInfo is mirrored by niagara_amd/_lib.py");
static_assert(sizeof(NvSceneCacheInfo) == 208, "NvSceneCacheInfo is mirrored by niagara_amd/_lib.py");
#endif

#endif /* NIAGARA_VIS_H */
