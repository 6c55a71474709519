/*
 * ref_runner.cpp — runs the reference's translated shader main()s on the CPU (TEST INFRASTRUCTURE).
 *
 * Compiled once per shader by oracle/Makefile with -DREF_<SHADER> -DREF_GEN="<generated header>".  The generated
 * header is the reference's own source text (see ref_translate.py); this file only supplies what Vulkan would:
 * descriptor binding (pointer assignment), specialisation constants, push constants and the invocation loops,
 * serialised in ascending workgroup / local id order.
 */
#include "glsl_shim.h"

#include <stddef.h>

namespace glsl
{
static uvec3 gl_GlobalInvocationID, gl_LocalInvocationID, gl_WorkGroupID;
#ifdef REF_MESHLET_MESH
/* GL_EXT_mesh_shader built-ins the mesh stage writes (the runner reads them back after each workgroup) */
static uint gl_LocalInvocationIndex;
struct MeshVertexOut
{
	vec4 gl_Position;
};
struct MeshPrimitiveOut
{
	bool gl_CullPrimitiveEXT;
};
static MeshVertexOut gl_MeshVerticesEXT[256];
static uvec3 gl_PrimitiveTriangleIndicesEXT[256];
static MeshPrimitiveOut gl_MeshPrimitivesEXT[256];
static uint ref_outVertices, ref_outPrimitives;
static void SetMeshOutputsEXT(uint vertexCount, uint primitiveCount)
{
	ref_outVertices = vertexCount;
	ref_outPrimitives = primitiveCount;
}
static void barrier() {} /* the runner executes the workgroup twice instead (see ref_meshlet_mesh) */
#endif

#ifdef REF_MESHLET_TASK
/* GL_EXT_mesh_shader built-ins of the task stage.  Invocations are serialised in ascending order, so the last one's
 * EmitMeshTasksEXT carries the workgroup's final sharedCount; barrier() is honoured by the translator's --once rewrite of
 * the shared counter's initialisation (oracle/Makefile) and by that ordering. */
static uint ref_emitCount;
static void EmitMeshTasksEXT(uint x, uint, uint) { ref_emitCount = x; }
static void barrier() {}
#endif

#ifdef REF_MESH_FRAG
/* fragment-stage built-ins: gl_FragCoord, and `discard` (rewritten by the translator to set this flag and return) */
static vec4 gl_FragCoord;
static bool ref_discard;
#endif

namespace REF_NS
{
#include REF_GEN
}
} // namespace glsl

using namespace glsl;
using namespace glsl::REF_NS;

struct RefPyramid
{
	const float* base;
	uint32_t width, height, levels;
	uint32_t mipOffset[16];
	uint32_t totalTexels;
};

#if defined(REF_DRAWCULL) || defined(REF_CLUSTERCULL) || defined(REF_MESHLET_TASK)
static texture2D bind_pyramid(const RefPyramid* p)
{
	texture2D t = { 0, 0, 0, 0, 0 };
	if (p)
	{
		t.base = p->base;
		t.width = p->width;
		t.height = p->height;
		t.levels = p->levels;
		t.mipOffset = p->mipOffset;
	}
	return t;
}
#endif

#ifdef REF_DRAWCULL
/* vkCmdDispatch(ceil(drawCount/64)) of drawcull.comp.glsl, local_size_x = 64 (src/niagara.cpp:1548-1556) */
extern "C" void ref_drawcull(const void* cull, int late, int task, void* draws_, void* meshes_, void* commands, uint32_t* count4,
                             uint32_t* dvb, const RefPyramid* pyr)
{
	cullData = *(const CullData*)cull;
	LATE = late != 0;
	TASK = task != 0;
	draws = (MeshDraw*)draws_;
	meshes = (Mesh*)meshes_;
	drawCommands = (MeshDrawCommand*)commands;
	taskCommands = (MeshTaskCommand*)commands;
	CommandCount_buf = (CommandCount_t*)count4;
	drawVisibility = dvb;
	depthPyramid = bind_pyramid(pyr);

	uint groups = (cullData.drawCount + 63) / 64;
	for (uint g = 0; g < groups; ++g)
		for (uint l = 0; l < 64; ++l)
		{
			gl_WorkGroupID.x = g;
			gl_LocalInvocationID.x = l;
			gl_GlobalInvocationID.x = g * 64 + l;
			shader_main();
		}
}

/* layout pinning + scalar helpers of src/shaders/math.h:2-49 */
extern "C" uint32_t ref_sizeof(int what)
{
	switch (what)
	{
	case 0: return sizeof(Meshlet);
	case 1: return sizeof(MeshDraw);
	case 2: return sizeof(MeshLod);
	case 3: return sizeof(Mesh);
	case 4: return sizeof(MeshDrawCommand);
	case 5: return sizeof(MeshTaskCommand);
	case 6: return sizeof(CullData);
	case 7: return offsetof(Mesh, lods);
	case 8: return offsetof(CullData, P00);
	case 9: return offsetof(CullData, frustum);
	case 10: return offsetof(CullData, lodTarget);
	case 11: return offsetof(CullData, drawCount);
	case 12: return offsetof(CullData, cullingEnabled);
	case 13: return offsetof(CullData, postPass);
	case 14: return offsetof(MeshDraw, orientation);
	case 15: return offsetof(MeshDraw, meshIndex);
	case 16: return offsetof(Meshlet, cone_axis);
	case 17: return offsetof(Meshlet, dataOffset);
	case 18: return TASK_WGSIZE;
	case 19: return TASK_WGLIMIT;
	case 20: return CLUSTER_LIMIT;
	case 21: return CLUSTER_TILE;
	case 22: return TASK_CULL;
	}
	return 0;
}
extern "C" void ref_rotate_quat(const float v[3], const float q[4], float out[3])
{
	vec3 r = rotateQuat(vec3(v[0], v[1], v[2]), vec4(q[0], q[1], q[2], q[3]));
	out[0] = r.x, out[1] = r.y, out[2] = r.z;
}
extern "C" int ref_project_sphere(const float c[3], float r, float znear, float P00, float P11, float aabb[4])
{
	vec4 a;
	bool ok = projectSphere(vec3(c[0], c[1], c[2]), r, znear, P00, P11, a);
	aabb[0] = a.x, aabb[1] = a.y, aabb[2] = a.z, aabb[3] = a.w;
	return ok;
}
extern "C" float ref_occlusion_mip(const float aabb[4], float pw, float ph)
{
	return getOcclusionMip(vec4(aabb[0], aabb[1], aabb[2], aabb[3]), pw, ph);
}
extern "C" int ref_cone_cull(const float c[3], float r, const float axis[3], float cutoff)
{
	return coneCull(vec3(c[0], c[1], c[2]), r, vec3(axis[0], axis[1], axis[2]), cutoff, vec3(0, 0, 0));
}
#endif

#ifdef REF_TASKSUBMIT
/* vkCmdDispatch(1,1,1) of tasksubmit.comp.glsl (src/niagara.cpp:1563-1568) */
extern "C" void ref_tasksubmit(uint32_t* count4, void* commands)
{
	CommandCount_buf = (CommandCount_t*)count4;
	taskCommands = (MeshTaskCommand*)commands;
	for (uint l = 0; l < 64; ++l)
	{
		gl_LocalInvocationID.x = l;
		gl_GlobalInvocationID.x = l;
		shader_main();
	}
}
#endif

#ifdef REF_CLUSTERCULL
/* vkCmdDispatchIndirect(dccb, 4) of clustercull.comp.glsl: grid (count4[1], count4[2], count4[3]) (src/niagara.cpp:1590-1599) */
extern "C" void ref_clustercull(const void* cull, int late, void* commands, const uint32_t* count4, void* draws_, void* meshlets_,
                                uint32_t* mvb, const RefPyramid* pyr, uint32_t* cib, uint32_t* cc4)
{
	cullData = *(const CullData*)cull;
	LATE = late != 0;
	taskCommands = (MeshTaskCommand*)commands;
	draws = (MeshDraw*)draws_;
	meshlets = (Meshlet*)meshlets_;
	meshletVisibility = mvb;
	depthPyramid = bind_pyramid(pyr);
	clusterIndices = cib;
	ClusterCount_buf = (ClusterCount_t*)cc4;

	for (uint gx = 0; gx < count4[1]; ++gx)
		for (uint gy = 0; gy < count4[2]; ++gy)
			for (uint l = 0; l < 64; ++l)
			{
				gl_WorkGroupID.x = gx;
				gl_WorkGroupID.y = gy;
				gl_LocalInvocationID.x = l;
				shader_main();
			}
}
#endif

#ifdef REF_CLUSTERSUBMIT
/* vkCmdDispatch(1,1,1) of clustersubmit.comp.glsl (src/niagara.cpp:1603-1608) */
extern "C" void ref_clustersubmit(uint32_t* cc4, uint32_t* cib)
{
	ClusterCount_buf = (ClusterCount_t*)cc4;
	clusterIndices = cib;
	for (uint l = 0; l < 256; ++l)
	{
		gl_LocalInvocationID.x = l;
		shader_main();
	}
}
#endif

#ifdef REF_DEPTHREDUCE
/* the level loop of src/niagara.cpp:1713-1728 around depthreduce.comp.glsl (local size 32x32) */
extern "C" void ref_depthreduce(const float* depth, uint32_t w, uint32_t h, float* base, uint32_t pw, uint32_t ph, uint32_t levels,
                                const uint32_t* mipOffset)
{
	static const uint zero = 0;
	texture2D src = { depth, w, h, 1, &zero };
	for (uint i = 0; i < levels; ++i)
	{
		uint lw = pw >> i, lh = ph >> i;
		lw = lw ? lw : 1;
		lh = lh ? lh : 1;
		image2D dst = { base + mipOffset[i], lw, lh };
		outImage = dst;
		inImage = src;
		imageSize = vec2((float)lw, (float)lh);
		/* dispatch() rounds the grid up to whole 32x32 groups (src/niagara.cpp:213-225); the image store of an
		 * out-of-range texel is discarded by Vulkan, so only in-range invocations are run here */
		for (uint y = 0; y < lh; ++y)
			for (uint x = 0; x < lw; ++x)
			{
				gl_GlobalInvocationID.x = x;
				gl_GlobalInvocationID.y = y;
				shader_main();
			}
		texture2D next = { dst.data, lw, lh, 1, &zero };
		src = next;
	}
}
#endif

#ifdef REF_HOST
/* verbatim host helpers: src/niagara.cpp:424-481 (projection, normalizePlane, previousPow2, PCG32),
 * src/resources.cpp:280-292 (getImageMipLevels) */
extern "C" uint32_t ref_previous_pow2(uint32_t v) { return previousPow2(v); }
extern "C" uint32_t ref_image_mip_levels(uint32_t w, uint32_t h) { return getImageMipLevels(w, h); }
extern "C" void ref_rng_seed(uint64_t state) { rngstate.state = state; }
extern "C" uint32_t ref_rand32(void) { return rand32(); }
extern "C" double ref_rand01(void) { return rand01(); }
extern "C" void ref_perspective(float fovY, float aspect, float znear, float out16[16], float frustum[4])
{
	mat4 projection = perspectiveProjection(fovY, aspect, znear);
	for (int c = 0; c < 4; ++c)
	{
		out16[4 * c + 0] = projection[c].x;
		out16[4 * c + 1] = projection[c].y;
		out16[4 * c + 2] = projection[c].z;
		out16[4 * c + 3] = projection[c].w;
	}
	/* src/niagara.cpp:1494-1497,1506-1509 (statements restated: they live inside main()) */
	mat4 projectionT = transpose(projection);
	vec4 frustumX = normalizePlane(projectionT[3] + projectionT[0]);
	vec4 frustumY = normalizePlane(projectionT[3] + projectionT[1]);
	frustum[0] = frustumX.x;
	frustum[1] = frustumX.z;
	frustum[2] = frustumY.y;
	frustum[3] = frustumY.z;
}
#endif

#ifdef REF_HOST
#include <algorithm>
#include <vector>
/* src/scene.cpp:207-220 compiled verbatim inside a function that supplies the names those statements use: `positions`
 * (the de-quantised vertex positions), `vertices` (only its size), `mesh` (center, radius) */
extern "C" void ref_mesh_bounds(const float* xyz, uint32_t count, float out_center[3], float* out_radius)
{
	std::vector<vec3> positions(count);
	for (uint32_t i = 0; i < count; ++i)
		positions[i] = vec3(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
	std::vector<int> vertices(count);
	struct
	{
		vec3 center;
		float radius;
	} mesh;
#include "_ref/host_bounds.gen.h"
	out_center[0] = mesh.center.x;
	out_center[1] = mesh.center.y;
	out_center[2] = mesh.center.z;
	*out_radius = mesh.radius;
}
#endif

#ifdef REF_MESHLET_MESH
/* vkCmdDrawMeshTasksIndirectEXT(ccb, 4) of meshlet.mesh.glsl without a task stage (TASK = false): one workgroup of
 * MESH_WGSIZE = 64 invocations per grid cell {x < cc4[1], y < cc4[2], z < cc4[3]} (src/niagara.cpp:1664).  The shader
 * has one barrier() between its vertex and triangle phases; invocations are serialised here, so every workgroup is run
 * TWICE: the first run leaves vertexClip[] complete, the second run's triangle phase then reads what a real
 * workgroup would read after the barrier (main() has no other cross-invocation state and only overwrites its outputs). */
extern "C" void ref_meshlet_mesh(const void* globals_, void* commands, void* draws_, void* meshlets_, uint32_t* meshletData_, void* vertices_,
                                 uint32_t* clusterIndices_, const uint32_t* cc4, uint32_t* masks4, uint32_t capacity, uint64_t* totals3)
{
	/* push-constant block in the GLSL (std430) layout: mat4 @0, CullData @64 (144 bytes: a struct that contains a mat4 is
	 * 16-byte aligned, the shim's plain-float CullData is 136), screenWidth / screenHeight @208 */
	memcpy(&globals.projection, globals_, 64);
	memcpy(&globals.cullData, (const char*)globals_ + 64, sizeof(CullData));
	memcpy(&globals.screenWidth, (const char*)globals_ + 208, 4);
	memcpy(&globals.screenHeight, (const char*)globals_ + 212, 4);
	TASK = false;
	taskCommands = (MeshTaskCommand*)commands;
	draws = (MeshDraw*)draws_;
	meshlets = (Meshlet*)meshlets_;
	meshletData = meshletData_;
	meshletData16 = (uint16_t*)meshletData_;
	meshletData8 = (uint8_t*)meshletData_;
	vertices = (Vertex*)vertices_;
	clusterIndices = clusterIndices_;
	for (uint y = 0; y < cc4[2]; ++y)
		for (uint z = 0; z < cc4[3]; ++z)
			for (uint x = 0; x < cc4[1]; ++x)
			{
				gl_WorkGroupID.x = x;
				gl_WorkGroupID.y = y;
				gl_WorkGroupID.z = z;
				for (int run = 0; run < 2; ++run)
					for (uint l = 0; l < 64; ++l)
					{
						gl_LocalInvocationIndex = l;
						gl_LocalInvocationID.x = l;
						shader_main();
					}
				uint32_t index = x + y * 256 + z * CLUSTER_TILE;
				uint32_t out[4] = { 0, 0, 0, 0 };
				if (ref_outVertices || ref_outPrimitives || clusterIndices_[index] != ~0u)
				{
					uint32_t kept = 0;
					for (uint i = 0; i < ref_outPrimitives; ++i)
						if (!gl_MeshPrimitivesEXT[i].gl_CullPrimitiveEXT)
						{
							out[i >> 5] |= 1u << (i & 31);
							kept++;
						}
					out[3] = (ref_outPrimitives & 0xffu) | (ref_outVertices & 0xffu) << 8 | kept << 16;
					totals3[0] += 1;
					totals3[1] += ref_outPrimitives;
					totals3[2] += kept;
				}
				if (index < capacity)
					memcpy(masks4 + (size_t)index * 4, out, sizeof(out));
			}
}
#endif

#ifdef REF_MESHLET_TASK
/* vkCmdDrawMeshTasksIndirectEXT(dccb, 4) of meshlet.task.glsl: grid (count4[1], count4[2] = 64, 1), one workgroup of
 * TASK_WGSIZE = 64 invocations per task command (src/niagara.cpp:1660).  Per workgroup the payload's first
 * EmitMeshTasksEXT-count entries and that count are handed back. */
extern "C" void ref_meshlet_task(const void* cull, int late, void* commands, const uint32_t* count4, void* draws_, void* meshlets_, uint32_t* mvb,
                                 const RefPyramid* pyr, uint32_t* payloads, uint32_t* payloadCounts)
{
	memcpy(&globals.cullData, cull, sizeof(CullData));
	LATE = late != 0;
	taskCommands = (MeshTaskCommand*)commands;
	draws = (MeshDraw*)draws_;
	meshlets = (Meshlet*)meshlets_;
	meshletVisibility = mvb;
	depthPyramid = bind_pyramid(pyr);
	for (uint gx = 0; gx < count4[1]; ++gx)
		for (uint gy = 0; gy < count4[2]; ++gy)
		{
			ref_emitCount = 0;
			for (uint l = 0; l < 64; ++l)
			{
				gl_WorkGroupID.x = gx;
				gl_WorkGroupID.y = gy;
				gl_LocalInvocationID.x = l;
				shader_main();
			}
			const uint commandId = gx * 64 + gy;
			for (uint i = 0; i < ref_emitCount; ++i)
				payloads[(size_t)commandId * 64 + i] = payload.clusterIndices[i];
			payloadCounts[commandId] = ref_emitCount;
		}
}
#endif

/* ================= the shading end of the frame (built with -DREF_SHADING: typed images, oracle/glsl_shade_shim.h) =================
 *
 * Every binding's format is the reference host code's:
 *   depthTarget       VK_FORMAT_D32_SFLOAT                 src/niagara.cpp:631, :1326
 *   gbufferTargets[0] VK_FORMAT_R8G8B8A8_UNORM             src/niagara.cpp:634-637, :1325
 *   gbufferTargets[1] VK_FORMAT_A2B10G10R10_UNORM_PACK32   src/niagara.cpp:634-637, :1325
 *   shadowTarget, shadowblurTarget  VK_FORMAT_R8_UNORM     src/niagara.cpp:1328-1329
 *   bloomTarget and its mip views   VK_FORMAT_B10G11R11_UFLOAT_PACK32   src/niagara.cpp:1335-1337
 *   the output of final.comp.glsl   the swapchain's format (src/niagara.cpp:1197, :1864), VK_FORMAT_R8G8B8A8_UNORM where the surface leaves
 *                                   the choice (src/swapchain.cpp:54-55); a BGRA surface stores the same codes in another byte order
 * dispatch() rounds the grid up to whole 8x8 workgroups (src/niagara.cpp:213-225, src/shaders.h:71-74); every invocation of that grid runs. */
#ifdef REF_SHADING
template <typename F>
static void run_grid(uint32_t threadsX, uint32_t threadsY, F&& body)
{
	uint32_t gx = (threadsX + 7) / 8, gy = (threadsY + 7) / 8;
	for (uint32_t y = 0; y < gy * 8; ++y)
		for (uint32_t x = 0; x < gx * 8; ++x)
		{
			gl_GlobalInvocationID.x = x;
			gl_GlobalInvocationID.y = y;
			gl_LocalInvocationID.x = x & 7, gl_LocalInvocationID.y = y & 7;
			gl_WorkGroupID.x = x >> 3, gl_WorkGroupID.y = y >> 3;
			body();
		}
}
static texture2D bind_texture(const void* data, uint32_t w, uint32_t h, ImageFormat f)
{
	texture2D t = { data, w, h, f, 0 };
	return t;
}
static image2D bind_image(void* data, uint32_t w, uint32_t h, ImageFormat f, float* handed)
{
	image2D t = { data, w, h, f, (vec4*)handed };
	return t;
}
/* the shim's counters since the last call (glsl_shade_shim.h, shim_stats): the tests' input conditions */
extern "C" void REF_STATS(uint32_t out[7])
{
	memcpy(out, shim_stats, sizeof(shim_stats));
	memset(shim_stats, 0, sizeof(shim_stats));
}
#endif

#ifdef REF_SHADOWFILL
/* src/niagara.cpp:1822-1834: dispatch((width + 1) / 2, height) of shadowfill.comp.glsl, in place on shadowTarget */
extern "C" void ref_shadowfill(uint8_t* shadow, const float* depth, uint32_t w, uint32_t h, int checker, float* handed)
{
	imageSize = vec2((float)w, (float)h);
	checkerboard = checker;
	shadowImage = bind_image(shadow, w, h, FORMAT_R8_UNORM, handed);
	depthImage = bind_texture(depth, w, h, FORMAT_R32_SFLOAT);
	run_grid((w + 1) / 2, h, [] { shader_main(); });
}
#endif

#ifdef REF_SHADOWBLUR
/* src/niagara.cpp:1836-1850: dispatch(width, height) of shadowblur.comp.glsl; direction 1 in the first pass, 0 in the second */
extern "C" void ref_shadowblur(uint8_t* out, const uint8_t* shadow, const float* depth, uint32_t w, uint32_t h, float dir, float zn, float* handed)
{
	imageSize = vec2((float)w, (float)h);
	direction = dir;
	znear = zn;
	outImage = bind_image(out, w, h, FORMAT_R8_UNORM, handed);
	shadowImage = bind_texture(shadow, w, h, FORMAT_R8_UNORM);
	depthImage = bind_texture(depth, w, h, FORMAT_R32_SFLOAT);
	run_grid(w, h, [] { shader_main(); });
}
#endif

#ifdef REF_FINAL
/* src/niagara.cpp:1911-1925: dispatch(width, height) of final.comp.glsl.  sd: ShadeData as the host lays it out (src/niagara.cpp:280-290:
 * vec3, pad, vec3, int, mat4, vec2).  bloom: level 0 of the bloom target (the view bloomTarget.imageView starts there). */
extern "C" void ref_final(const float* sd, const uint32_t* g0, const uint32_t* g1, const float* depth, const uint8_t* shadow, const uint32_t* bloom,
                          uint32_t bw, uint32_t bh, uint32_t* color, uint32_t w, uint32_t h, float* handed)
{
	shadeData.cameraPosition = vec3(sd[0], sd[1], sd[2]);
	shadeData.sunDirection = vec3(sd[4], sd[5], sd[6]);
	memcpy(&shadeData.shadowsEnabled, sd + 7, 4);
	for (int c = 0; c < 4; ++c)
		shadeData.inverseViewProjection[c] = vec4(sd[8 + 4 * c], sd[9 + 4 * c], sd[10 + 4 * c], sd[11 + 4 * c]);
	shadeData.imageSize = vec2(sd[24], sd[25]);
	outImage = bind_image(color, w, h, FORMAT_R8G8B8A8_UNORM, handed);
	gbufferImage0 = bind_texture(g0, w, h, FORMAT_R8G8B8A8_UNORM);
	gbufferImage1 = bind_texture(g1, w, h, FORMAT_A2B10G10R10_UNORM_PACK32);
	depthImage = bind_texture(depth, w, h, FORMAT_R32_SFLOAT);
	shadowImage = shadow ? bind_texture(shadow, w, h, FORMAT_R8_UNORM) : bind_texture(0, 0, 0, FORMAT_R8_UNORM);
	bloomImage = bind_texture(bloom, bw, bh, FORMAT_B10G11R11_UFLOAT_PACK32);
	run_grid(w, h, [] { shader_main(); });
}

/* the helpers of src/shaders/math.h:51-109, one by one over arrays of n arguments */
extern "C" void ref_encode_oct(const float* v, uint32_t n, float* out)
{
	for (uint32_t i = 0; i < n; ++i)
	{
		vec2 r = encodeOct(vec3(v[3 * i], v[3 * i + 1], v[3 * i + 2]));
		out[2 * i] = r.x, out[2 * i + 1] = r.y;
	}
}
extern "C" void ref_decode_oct(const float* e, uint32_t n, float* out)
{
	for (uint32_t i = 0; i < n; ++i)
	{
		vec3 r = decodeOct(vec2(e[2 * i], e[2 * i + 1]));
		out[3 * i] = r.x, out[3 * i + 1] = r.y, out[3 * i + 2] = r.z;
	}
}
/* which: 0 tosrgb(vec3), 1 fromsrgb(vec3), 2 tonemap, 3 tosrgb(vec4), 4 fromsrgb(vec4) (the vec4 forms pass .w through); c, out: 3 or 4 floats each */
extern "C" void ref_colour(int which, const float* c, uint32_t n, float* out)
{
	for (uint32_t i = 0; i < n; ++i)
		if (which < 3)
		{
			vec3 a(c[3 * i], c[3 * i + 1], c[3 * i + 2]);
			vec3 r = which == 0 ? tosrgb(a) : which == 1 ? fromsrgb(a) : tonemap(a);
			out[3 * i] = r.x, out[3 * i + 1] = r.y, out[3 * i + 2] = r.z;
		}
		else
		{
			vec4 a(c[4 * i], c[4 * i + 1], c[4 * i + 2], c[4 * i + 3]);
			vec4 r = which == 3 ? tosrgb(a) : fromsrgb(a);
			out[4 * i] = r.x, out[4 * i + 1] = r.y, out[4 * i + 2] = r.z, out[4 * i + 3] = r.w;
		}
}
extern "C" void ref_gradient_noise(const float* uv, uint32_t n, float* out)
{
	for (uint32_t i = 0; i < n; ++i)
		out[i] = gradientNoise(vec2(uv[2 * i], uv[2 * i + 1]));
}
extern "C" void ref_unpack_tbn(const uint32_t* np, const uint32_t* tp, uint32_t n, float* normal3, float* tangent4)
{
	for (uint32_t i = 0; i < n; ++i)
	{
		vec3 nrm;
		vec4 tan;
		REF_NS::unpackTBN(np[i], tp[i], nrm, tan);
		normal3[3 * i] = nrm.x, normal3[3 * i + 1] = nrm.y, normal3[3 * i + 2] = nrm.z;
		tangent4[4 * i] = tan.x, tangent4[4 * i + 1] = tan.y, tangent4[4 * i + 2] = tan.z, tangent4[4 * i + 3] = tan.w;
	}
}
#endif

#ifdef REF_BLOOM
/* one dispatch of bloom.comp.glsl (QUALITY 1) as src/niagara.cpp:1882-1885 / :1897-1898 issue it: dispatch(levelWidth, levelHeight) with
 * imageSize = the target level's size.  srcIsGbuffer: the source is gbufferTargets[0] (pass 0), else a level of the bloom target.
 */
static void bloom_dispatch(int pass_, const uint32_t* src, uint32_t W, uint32_t H, int srcIsGbuffer, uint32_t* dst, uint32_t w, uint32_t h, float radius_,
                           float* handed)
{
	imageSize = vec2((float)w, (float)h);
	pass = pass_;
	radius = radius_;
	outImage = bind_image(dst, w, h, FORMAT_B10G11R11_UFLOAT_PACK32, handed);
	sourceImage = bind_texture(src, W, H, srcIsGbuffer ? FORMAT_R8G8B8A8_UNORM : FORMAT_B10G11R11_UFLOAT_PACK32);
	run_grid(w, h, [] { shader_main(); });
}
extern "C" void ref_bloom_pass(int pass_, const uint32_t* src, uint32_t W, uint32_t H, int srcIsGbuffer, uint32_t* dst, uint32_t w, uint32_t h,
                               float radius_, float* handed)
{
	bloom_dispatch(pass_, src, W, H, srcIsGbuffer, dst, w, h, radius_, handed);
}
/* the loop of src/niagara.cpp:1873-1901: pass 0 into level 0, pass 1 into levels 1 .. levels - 1, pass 2 into levels - 2 .. 0 with radius 2;
 * bloomWidth / bloomHeight / levels as src/niagara.cpp:1331-1333 computes them (handed in), levelOffset in texels of the one buffer */
extern "C" void ref_bloom(const uint32_t* g0, uint32_t W, uint32_t H, uint32_t* target, uint32_t bloomWidth, uint32_t bloomHeight, uint32_t bloomLevels,
                          const uint32_t* levelOffset)
{
	for (uint32_t i = 0; i < bloomLevels; ++i)
	{
		uint32_t levelWidth = bloomWidth >> i ? bloomWidth >> i : 1u, levelHeight = bloomHeight >> i ? bloomHeight >> i : 1u;
		uint32_t srcWidth = bloomWidth >> (i - 1) ? bloomWidth >> (i - 1) : 1u, srcHeight = bloomHeight >> (i - 1) ? bloomHeight >> (i - 1) : 1u;
		if (i == 0)
			bloom_dispatch(0, g0, W, H, 1, target + levelOffset[0], levelWidth, levelHeight, 0.f, 0);
		else
			bloom_dispatch(1, target + levelOffset[i - 1], srcWidth, srcHeight, 0, target + levelOffset[i], levelWidth, levelHeight, 0.f, 0);
	}
	for (int i = (int)bloomLevels - 2; i >= 0; --i)
	{
		uint32_t levelWidth = bloomWidth >> i ? bloomWidth >> i : 1u, levelHeight = bloomHeight >> i ? bloomHeight >> i : 1u;
		uint32_t srcWidth = bloomWidth >> (i + 1) ? bloomWidth >> (i + 1) : 1u, srcHeight = bloomHeight >> (i + 1) ? bloomHeight >> (i + 1) : 1u;
		bloom_dispatch(2, target + levelOffset[i + 1], srcWidth, srcHeight, 0, target + levelOffset[i], levelWidth, levelHeight, 2.0f, 0);
	}
}
#endif

#ifdef REF_MESH_FRAG
/* mesh.frag.glsl:55-95 once per fragment.  The inputs of :27-31 are one 64-byte record {vec2 uv, vec2 bary, vec3 normal, uint drawId,
 * vec4 tangent, vec3 wpos, uint materialIndex}; fragment i sits at pixel (i % width, i / width), gl_FragCoord.xy = pixel + 0.5.  A record with
 * drawId == ~0 has no fragment (outputs stay 0).  draws: 48-byte MeshDraw, materials: 64-byte Material (src/shaders/mesh.h:80-102).
 * texture(SAMP(id), uv) is the caller's: taps (optional, n x 4 x 4 floats) holds per fragment the texel of the albedo, normal, specular and
 * emissive slot; a slot whose texture id is > 0 is renumbered to slot + 1 so the shim can tell the four apart.
 * Outputs: the attachments packed by the shim's UNORM store in the formats of src/niagara.cpp:634-637, the discard flag, and (optional,
 * n x 8 floats) gbuffer[0] and gbuffer[1] as written. */
extern "C" void ref_mesh_frag(const void* records, uint32_t n, uint32_t width, const void* draws_, const void* materials_, uint32_t materialCount,
                              const float* taps, int post, uint32_t* gb0, uint32_t* gb1, uint8_t* discarded, float* written)
{
	struct Record
	{
		float uv[2], bary[2], normal[3];
		uint32_t drawId;
		float tangent[4], wpos[3];
		uint32_t materialIndex;
	};
	struct DrawIn
	{
		float position[3], scale, orientation[4];
		uint32_t meshIndex, meshletVisibilityOffset, postPass, materialIndex;
	};
	struct MaterialIn
	{
		uint32_t tex[4];
		float diffuse[4], specular[4], emissive[3];
		uint32_t padding;
	};
	const Record* rec = (const Record*)records;
	const DrawIn* din = (const DrawIn*)draws_;
	const MaterialIn* min_ = (const MaterialIn*)materials_;
	static MeshDraw oneDraw;
	static Material* table = 0;
	delete[] table;
	table = new Material[materialCount ? materialCount : 1];
	for (uint32_t m = 0; m < materialCount; ++m)
	{
		table[m].albedoTexture = min_[m].tex[0] > 0 ? 1u : 0u;
		table[m].normalTexture = min_[m].tex[1] > 0 ? 2u : 0u;
		table[m].specularTexture = min_[m].tex[2] > 0 ? 3u : 0u;
		table[m].emissiveTexture = min_[m].tex[3] > 0 ? 4u : 0u;
		table[m].diffuseFactor = vec4(min_[m].diffuse[0], min_[m].diffuse[1], min_[m].diffuse[2], min_[m].diffuse[3]);
		table[m].specularFactor = vec4(min_[m].specular[0], min_[m].specular[1], min_[m].specular[2], min_[m].specular[3]);
		table[m].emissiveFactor = vec3(min_[m].emissive[0], min_[m].emissive[1], min_[m].emissive[2]);
	}
	materials = table;
	draws = &oneDraw;
	POST = post;
	for (uint32_t i = 0; i < n; ++i)
	{
		gb0[i] = gb1[i] = 0;
		discarded[i] = 0;
		if (rec[i].drawId == ~0u)
			continue;
		const DrawIn& d = din[rec[i].drawId];
		oneDraw.materialIndex = d.materialIndex; /* :57-58 read nothing else of the draw */
		drawId = 0;
		uv = vec2(rec[i].uv[0], rec[i].uv[1]);
		normal = vec3(rec[i].normal[0], rec[i].normal[1], rec[i].normal[2]);
		tangent = vec4(rec[i].tangent[0], rec[i].tangent[1], rec[i].tangent[2], rec[i].tangent[3]);
		wpos = vec3(rec[i].wpos[0], rec[i].wpos[1], rec[i].wpos[2]);
		gl_FragCoord = vec4((float)(i % width) + 0.5f, (float)(i / width) + 0.5f, 0, 1);
		for (int s = 0; s < 4; ++s)
			shim_taps.texel[s + 1] = taps ? vec4(taps[(size_t)i * 16 + 4 * s], taps[(size_t)i * 16 + 4 * s + 1], taps[(size_t)i * 16 + 4 * s + 2],
			                                     taps[(size_t)i * 16 + 4 * s + 3])
			                              : vec4(0);
		ref_discard = false;
		gbuffer[0] = gbuffer[1] = vec4(0);
		shader_main();
		gb0[i] = shim_encode_word(gbuffer[0], FORMAT_R8G8B8A8_UNORM);
		gb1[i] = shim_encode_word(gbuffer[1], FORMAT_A2B10G10R10_UNORM_PACK32);
		discarded[i] = ref_discard;
		if (written)
		{
			float* o = written + (size_t)i * 8;
			o[0] = gbuffer[0].x, o[1] = gbuffer[0].y, o[2] = gbuffer[0].z, o[3] = gbuffer[0].w;
			o[4] = gbuffer[1].x, o[5] = gbuffer[1].y, o[6] = gbuffer[1].z, o[7] = gbuffer[1].w;
		}
	}
}
#endif

#ifdef REF_SHADOW
#include <vector>
/* src/niagara.cpp:1797-1817: dispatch(shadowWidthCB, height) of shadow.comp.glsl, shadowWidthCB = checkerboard ? (width + 1) / 2 : width, into
 * shadowTarget (R8_UNORM); QUALITY 0 is shadowlqPipeline, 1 shadowhqPipeline (:1803).  sd: the 96-byte ShadowData as the host lays it out (vec3,
 * float, mat4, vec2, int).  The bindings of :1808 are the caller's arrays in the C ABI's layouts (Mesh 208 bytes, MeshDraw 48, Vertex 16,
 * Material 64, texture descriptors of four words {offset, width, height, levels} over one buffer of decoded RGBA8 words, entry 0 reserved).
 * The acceleration structure is built here from the draws as glsl_rayquery_shim.h's model states (fillInstanceRT, src/scenert.cpp:504-518).
 * mask: w * h bytes, prefilled by the caller; texels no invocation stores to keep their byte.  Per texel an invocation stored to: handed (4
 * floats: the vec4 given to imageStore), rays (8 floats: origin, direction, tmin, tmax of its last rayQueryInitializeEXT) and info (6 words:
 * queries initialised, ray flags, opaque commits, non-opaque candidates, confirmed candidates, the committed instance or ~0).  samples: up to
 * sampleRoom x 8 floats {id, u, v, alpha, instance, primitive, bary.x, bary.y} of the textureLod calls, in order; *sampleCount is how many there were. */
extern "C" void ref_shadow(const float* sd, const float* depth, uint32_t w, uint32_t h, const void* meshes_, uint32_t meshCount, const uint32_t* indices_,
                           uint32_t indexCapacity, const void* vertices_, uint32_t vertexCapacity, const void* draws_, uint32_t drawCount, const void* materials_,
                           uint32_t materialCount, const uint32_t* descs, uint32_t textureCount, const uint32_t* texels, uint64_t texelWords, int quality,
                           uint8_t* mask, float* handed, float* rays, uint32_t* info, float* samples, uint64_t sampleRoom, uint64_t* sampleCount)
{
	static_assert(sizeof(Mesh) == 208 && sizeof(MeshDraw) == 48 && sizeof(Vertex) == 16, "the translated structs have the C ABI's layouts");
	struct MaterialIn
	{
		uint32_t tex[4];
		float diffuse[4], specular[4], emissive[3];
		uint32_t padding;
	};
	const MaterialIn* min_ = (const MaterialIn*)materials_;
	int cb;
	memcpy(&cb, sd + 22, 4);
	shadowData.sunDirection = vec3(sd[0], sd[1], sd[2]);
	shadowData.sunJitter = sd[3];
	for (int c = 0; c < 4; ++c)
		shadowData.inverseViewProjection[c] = vec4(sd[4 + 4 * c], sd[5 + 4 * c], sd[6 + 4 * c], sd[7 + 4 * c]);
	shadowData.imageSize = vec2(sd[20], sd[21]);
	shadowData.checkerboard = cb;
	QUALITY = quality;

	/* materials: one entry behind the table stands for every material index at or past it — "no texture" (the shader's own
	 * load there is out of bounds) */
	std::vector<Material> table(materialCount + 1u);
	for (uint32_t m = 0; m < materialCount; ++m)
	{
		table[m].albedoTexture = min_[m].tex[0], table[m].normalTexture = min_[m].tex[1];
		table[m].specularTexture = min_[m].tex[2], table[m].emissiveTexture = min_[m].tex[3];
	}
	table[materialCount].albedoTexture = 0;
	std::vector<MeshDraw> drawTable(drawCount ? drawCount : 1u);
	if (drawCount)
		memcpy(drawTable.data(), draws_, (size_t)drawCount * sizeof(MeshDraw));
	for (uint32_t i = 0; i < drawCount; ++i)
		if (drawTable[i].materialIndex >= materialCount)
			drawTable[i].materialIndex = materialCount;
	draws = drawTable.data();
	meshes = (Mesh*)meshes_;
	materials = table.data();
	vertices = (Vertex*)vertices_;
	indices = (uint*)indices_;

	/* textures: level 0 of every descriptor the set holds whole (DESIGN.md §4.18's descriptor check); the others are "no texture" */
	std::vector<ShimLevel0> levels(textureCount ? textureCount : 1u);
	for (uint32_t t = 0; t < textureCount; ++t)
	{
		const uint32_t offset = descs[4 * t], tw = descs[4 * t + 1], th = descs[4 * t + 2], tl = descs[4 * t + 3];
		uint64_t words = 0;
		bool ok = t != 0 && tw != 0 && th != 0 && tw <= 16384u && th <= 16384u && tl != 0 && tl <= 15u;
		for (uint32_t l = 0; ok && l < tl; ++l)
			words += (uint64_t)((tw >> l) ? (tw >> l) : 1u) * ((th >> l) ? (th >> l) : 1u);
		ok = ok && (uint64_t)offset + words <= texelWords;
		levels[t].texels = ok ? texels + offset : 0;
		levels[t].width = tw, levels[t].height = th;
	}
	shim_rq_textures = levels.data();
	shim_rq_texture_count = textureCount;
	shim_rq_samples.clear();

	/* the acceleration structure: the triangles of every mesh's lods[lodRT] once, an instance per draw */
	const Mesh* meshIn = (const Mesh*)meshes_;
	const Vertex* vertexIn = (const Vertex*)vertices_;
	std::vector<std::vector<nv::rt3>> corners(meshCount);
	std::vector<std::vector<uint8_t>> kept(meshCount);
	for (uint32_t m = 0; m < meshCount; ++m)
	{
		const Mesh& mesh = meshIn[m];
		if (mesh.lodRT >= 8u || mesh.lodRT >= mesh.lodCount)
			continue;
		const MeshLod& lod = mesh.lods[mesh.lodRT];
		const uint32_t count = lod.indexCount / 3u;
		corners[m].resize((size_t)count * 3u);
		kept[m].assign(count, 1);
		for (uint32_t t = 0; t < count; ++t)
			for (uint32_t k = 0; k < 3u; ++k)
			{
				const uint64_t at = (uint64_t)lod.indexOffset + 3ull * t + k;
				const uint64_t corner = at < indexCapacity ? (uint64_t)mesh.vertexOffset + indices_[at] : ~0ull;
				if (at >= indexCapacity || corner >= vertexCapacity)
				{
					kept[m][t] = 0;
					continue;
				}
				corners[m][3 * (size_t)t + k] = nv::rt3{ (float)vertexIn[corner].vx, (float)vertexIn[corner].vy, (float)vertexIn[corner].vz };
			}
	}
	std::vector<ShimRtInstance> instances(drawCount ? drawCount : 1u);
	const MeshDraw* drawIn = (const MeshDraw*)draws_;
	for (uint32_t i = 0; i < drawCount; ++i)
	{
		const MeshDraw& d = drawIn[i];
		ShimRtInstance& in = instances[i];
		in.position[0] = d.position.x, in.position[1] = d.position.y, in.position[2] = d.position.z;
		in.scale = d.scale;
		in.orientation[0] = d.orientation.x, in.orientation[1] = d.orientation.y, in.orientation[2] = d.orientation.z, in.orientation[3] = d.orientation.w;
		in.mask = d.postPass < 32u ? (1u << d.postPass) & 0xffu : 0u; /* src/scenert.cpp:515 */
		in.opaque = d.postPass == 0u;                                   /* :516 */
		bool finite = nv::rt_finite(d.scale);
		for (int k = 0; k < 3; ++k)
			finite = finite && nv::rt_finite(in.position[k]);
		for (int k = 0; k < 4; ++k)
			finite = finite && nv::rt_finite(in.orientation[k]);
		const bool geometry = d.postPass <= 1u /* :517 */ && d.meshIndex < meshCount && finite && d.scale > 0.0f && !kept[d.meshIndex < meshCount ? d.meshIndex : 0].empty();
		in.corners = geometry ? corners[d.meshIndex].data() : 0;
		in.kept = geometry ? kept[d.meshIndex].data() : 0;
		in.triangles = geometry ? (uint)kept[d.meshIndex].size() : 0u;
	}
	tlas.instances = instances.data();
	tlas.count = drawCount;

	outImage = bind_image(mask, w, h, FORMAT_R8_UNORM, handed);
	depthImage = bind_texture(depth, w, h, FORMAT_R32_SFLOAT);
	run_grid(cb ? (w + 1) / 2 : w, h, [&] {
		ShimRayLog log;
		memset(&log, 0, sizeof(log));
		log.committedInstance = ~0u;
		shim_rq_log = &log;
		shim_last_store = ivec2(-1, -1);
		shader_main();
		shim_rq_log = &shim_rq_scratch;
		if (!shim_inside(shim_last_store, w, h))
			return;
		const size_t at = (size_t)shim_last_store.y * w + (size_t)shim_last_store.x;
		memcpy(rays + at * 8, log.origin, 8 * sizeof(float));
		const uint32_t words[6] = { log.queries, log.flags, log.opaqueCommits, log.candidates, log.confirmed, log.committedInstance };
		memcpy(info + at * 6, words, sizeof(words));
	});
	*sampleCount = shim_rq_samples.size();
	for (size_t i = 0; i < shim_rq_samples.size() && i < sampleRoom; ++i)
	{
		const ShimSample& s = shim_rq_samples[i];
		float* o = samples + 8 * i;
		o[0] = (float)s.id, o[1] = s.u, o[2] = s.v, o[3] = s.alpha;
		o[4] = (float)s.instance, o[5] = (float)s.primitive, o[6] = s.baryX, o[7] = s.baryY;
	}
	shim_rq_textures = 0;
	shim_rq_texture_count = 0;
	tlas.instances = 0, tlas.count = 0;
}
#endif
