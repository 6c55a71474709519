// host.cpp — host-side helpers of the C ABI (no device work): the pieces of niagara's main() that prepare what the
// cull passes consume.  Plain C++; arithmetic is fp32 in the order written so that results are reproducible.
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/niagara_vis.h"
#include "animmath.h"

extern "C" {

// src/niagara.cpp:439-447 — largest power of two strictly below v (1 for v <= 2)
// n / d for a launch constant d: m = floor(2^39 / d) + 1 = 2^39 / d + e with 0 < e <= 1, so n m / 2^39 = n / d + n e / 2^39 and the
// floor is that of n / d while n e / 2^39 < 1 / d, i.e. for n < 2^39 / d; m fits 32 bits for d >= 256 (kernels: args.h)
uint32_t nv_division_magic(uint32_t d)
{
	return d >= 256u && d <= 8192u ? (uint32_t)((1ull << 39) / d) + 1u : 0u;
}

uint32_t nv_previous_pow2(uint32_t v)
{
	uint32_t r = 1;
	while (r * 2 < v)
		r *= 2;
	return r;
}

// src/resources.cpp:280-292
uint32_t nv_image_mip_levels(uint32_t width, uint32_t height)
{
	uint32_t levels = 1;
	while (width > 1 || height > 1)
	{
		++levels;
		width /= 2;
		height /= 2;
	}
	return levels;
}

// src/niagara.cpp:1340-1344 (+ linear mip offsets replacing the per-mip image views at :1346-1350)
int nv_pyramid_desc_init(NvPyramidDesc* desc, uint32_t depthWidth, uint32_t depthHeight)
{
	if (!desc || !depthWidth || !depthHeight)
		return NV_EINVAL;
	desc->width = nv_previous_pow2(depthWidth);
	desc->height = nv_previous_pow2(depthHeight);
	desc->levels = nv_image_mip_levels(desc->width, desc->height);
	if (desc->levels > NV_MAX_MIPS)
		return NV_EINVAL;
	uint32_t offset = 0;
	for (uint32_t i = 0; i < NV_MAX_MIPS; ++i)
	{
		desc->mipOffset[i] = offset;
		if (i < desc->levels)
		{
			uint32_t w = desc->width >> i, h = desc->height >> i;
			offset += (w ? w : 1) * (h ? h : 1);
		}
	}
	desc->totalTexels = offset;
	return NV_OK;
}

// src/niagara.cpp:1331-1333 (+ linear level offsets replacing the per-mip image views)
int nv_bloom_desc_init(NvBloomDesc* desc, uint32_t width, uint32_t height)
{
	if (!desc || !width || !height || width > 16384 || height > 16384)
		return NV_EINVAL;
	desc->width = (width + 1) / 2;
	desc->height = (height + 1) / 2;
	const uint32_t levels = nv_image_mip_levels(desc->width, desc->height);
	desc->levels = levels < NV_BLOOM_MAX_LEVELS ? levels : NV_BLOOM_MAX_LEVELS;
	uint32_t offset = 0;
	for (uint32_t i = 0; i < NV_BLOOM_MAX_LEVELS; ++i)
	{
		desc->levelOffset[i] = offset;
		if (i < desc->levels)
		{
			uint32_t w = desc->width >> i, h = desc->height >> i;
			offset += (w ? w : 1) * (h ? h : 1);
		}
	}
	desc->totalTexels = offset;
	return NV_OK;
}

// src/niagara.cpp:424-437 (perspectiveProjection, normalizePlane) and :1487-1516 (CullData).
// view = scale(1,1,-1) * inverse(translate(pos) * mat4_cast(q)); the inverse of a rigid transform is taken in
// closed form, [R^T | -(R^T t)] (glm is not vendored in the reference snapshot, so its cofactor inverse cannot be
// matched bit for bit; DESIGN.md lists this as a defined semantic).
int nv_build_cull_data(NvCullData* out, const float cameraPosition[3], const float cameraOrientation[4], float fovY,
                       float znear, float drawDistance, uint32_t viewportWidth, uint32_t viewportHeight,
                       uint32_t pyramidWidth, uint32_t pyramidHeight, uint32_t drawCount, int debugLodStep)
{
	if (!out || !cameraPosition || !cameraOrientation || !viewportWidth || !viewportHeight)
		return NV_EINVAL;
	memset(out, 0, sizeof(*out));

	const float x = cameraOrientation[0], y = cameraOrientation[1], z = cameraOrientation[2], w = cameraOrientation[3];
	const float xx = x * x, yy = y * y, zz = z * z;
	const float xz = x * z, xy = x * y, yz = y * z;
	const float wx = w * x, wy = w * y, wz = w * z;

	// rot[column][row]
	float rot[3][3];
	rot[0][0] = 1.0f - 2.0f * (yy + zz);
	rot[0][1] = 2.0f * (xy + wz);
	rot[0][2] = 2.0f * (xz - wy);
	rot[1][0] = 2.0f * (xy - wz);
	rot[1][1] = 1.0f - 2.0f * (xx + zz);
	rot[1][2] = 2.0f * (yz + wx);
	rot[2][0] = 2.0f * (xz + wy);
	rot[2][1] = 2.0f * (yz - wx);
	rot[2][2] = 1.0f - 2.0f * (xx + yy);

	float* view = out->view;
	for (int col = 0; col < 3; ++col)
		for (int row = 0; row < 3; ++row)
			view[4 * col + row] = rot[row][col]; // transpose
	for (int row = 0; row < 3; ++row)
	{
		float t = (rot[row][0] * cameraPosition[0] + rot[row][1] * cameraPosition[1]) + rot[row][2] * cameraPosition[2];
		view[12 + row] = -t;
	}
	view[15] = 1.0f;
	for (int col = 0; col < 4; ++col)
		view[4 * col + 2] = -view[4 * col + 2]; // scale(1,1,-1) on the left flips row 2

	const float f = 1.0f / tanf(fovY / 2.0f);
	const float aspect = (float)viewportWidth / (float)viewportHeight;
	out->P00 = f / aspect;
	out->P11 = f;
	out->znear = znear;
	out->zfar = drawDistance;

	// normalizePlane(row3 + row0) = (P00,0,1,0)/len, normalizePlane(row3 + row1) = (0,P11,1,0)/len
	const float lenX = sqrtf((out->P00 * out->P00 + 0.0f * 0.0f) + 1.0f * 1.0f);
	const float lenY = sqrtf((0.0f * 0.0f + out->P11 * out->P11) + 1.0f * 1.0f);
	out->frustum[0] = out->P00 / lenX;
	out->frustum[1] = 1.0f / lenX;
	out->frustum[2] = out->P11 / lenY;
	out->frustum[3] = 1.0f / lenY;

	out->lodTarget = (2.0f / out->P11) * (1.0f / (float)viewportHeight) * (float)(1 << debugLodStep);
	out->pyramidWidth = (float)pyramidWidth;
	out->pyramidHeight = (float)pyramidHeight;
	out->drawCount = drawCount;
	return NV_OK;
}

// src/niagara.cpp:1917-1922.  inverse(projection * view) in fp64 from the fp32 entries (the product's sums left to right, the inverse as adjugate /
// determinant from the 2 x 2 minors of the row pairs), rounded once to fp32.  A structural zero of the product stays an exact zero: with niagara's
// projection the w row of the result is (0, 0, 1 / znear, 0), so a sky pixel (depth 0) has wposh.w == 0 exactly, as in the shader.
static int inverse_view_projection(const NvGlobals* globals, float inverse[16])
{
	const float* P = globals->projection;
	const float* V = globals->cullData.view;
	double a[4][4]; // a[row][col] of projection * view (both column-major)
	for (int r = 0; r < 4; ++r)
		for (int c = 0; c < 4; ++c)
			a[r][c] = (((double)P[r] * V[4 * c] + (double)P[4 + r] * V[4 * c + 1]) + (double)P[8 + r] * V[4 * c + 2]) + (double)P[12 + r] * V[4 * c + 3];
	const double s0 = a[0][0] * a[1][1] - a[1][0] * a[0][1], s1 = a[0][0] * a[1][2] - a[1][0] * a[0][2], s2 = a[0][0] * a[1][3] - a[1][0] * a[0][3];
	const double s3 = a[0][1] * a[1][2] - a[1][1] * a[0][2], s4 = a[0][1] * a[1][3] - a[1][1] * a[0][3], s5 = a[0][2] * a[1][3] - a[1][2] * a[0][3];
	const double c5 = a[2][2] * a[3][3] - a[3][2] * a[2][3], c4 = a[2][1] * a[3][3] - a[3][1] * a[2][3], c3 = a[2][1] * a[3][2] - a[3][1] * a[2][2];
	const double c2 = a[2][0] * a[3][3] - a[3][0] * a[2][3], c1 = a[2][0] * a[3][2] - a[3][0] * a[2][2], c0 = a[2][0] * a[3][1] - a[3][0] * a[2][1];
	const double det = ((((s0 * c5 - s1 * c4) + s2 * c3) + s3 * c2) - s4 * c1) + s5 * c0;
	if (!(fabs(det) > 0.0) || !(fabs(det) < INFINITY))
		return NV_EINVAL;
	double b[4][4]; // the adjugate, b[row][col]
	b[0][0] = (a[1][1] * c5 - a[1][2] * c4) + a[1][3] * c3;
	b[0][1] = (-a[0][1] * c5 + a[0][2] * c4) - a[0][3] * c3;
	b[0][2] = (a[3][1] * s5 - a[3][2] * s4) + a[3][3] * s3;
	b[0][3] = (-a[2][1] * s5 + a[2][2] * s4) - a[2][3] * s3;
	b[1][0] = (-a[1][0] * c5 + a[1][2] * c2) - a[1][3] * c1;
	b[1][1] = (a[0][0] * c5 - a[0][2] * c2) + a[0][3] * c1;
	b[1][2] = (-a[3][0] * s5 + a[3][2] * s2) - a[3][3] * s1;
	b[1][3] = (a[2][0] * s5 - a[2][2] * s2) + a[2][3] * s1;
	b[2][0] = (a[1][0] * c4 - a[1][1] * c2) + a[1][3] * c0;
	b[2][1] = (-a[0][0] * c4 + a[0][1] * c2) - a[0][3] * c0;
	b[2][2] = (a[3][0] * s4 - a[3][1] * s2) + a[3][3] * s0;
	b[2][3] = (-a[2][0] * s4 + a[2][1] * s2) - a[2][3] * s0;
	b[3][0] = (-a[1][0] * c3 + a[1][1] * c1) - a[1][2] * c0;
	b[3][1] = (a[0][0] * c3 - a[0][1] * c1) + a[0][2] * c0;
	b[3][2] = (-a[3][0] * s3 + a[3][1] * s1) - a[3][2] * s0;
	b[3][3] = (a[2][0] * s3 - a[2][1] * s1) + a[2][2] * s0;
	for (int r = 0; r < 4; ++r)
		for (int c = 0; c < 4; ++c)
		{
			const double v = b[r][c] / det;
			if (!(fabs(v) < INFINITY))
				return NV_EINVAL;
			inverse[4 * c + r] = (float)v;
		}
	return NV_OK;
}

int nv_build_shade_data(NvShadeData* out, const NvGlobals* globals, const float cameraPosition[3], const float sunDirection[3], int shadowsEnabled,
                        uint32_t width, uint32_t height)
{
	if (!out || !globals || !cameraPosition || !sunDirection || !width || !height)
		return NV_EINVAL;
	float inverse[16];
	if (inverse_view_projection(globals, inverse) != NV_OK)
		return NV_EINVAL;
	memset(out, 0, sizeof(*out));
	memcpy(out->inverseViewProjection, inverse, sizeof(inverse));
	for (int k = 0; k < 3; ++k)
	{
		out->cameraPosition[k] = cameraPosition[k];
		out->sunDirection[k] = sunDirection[k];
	}
	out->shadowsEnabled = shadowsEnabled;
	out->imageSize[0] = (float)width;
	out->imageSize[1] = (float)height;
	return NV_OK;
}

// src/niagara.cpp:1810-1815: the same inverse as nv_build_shade_data's
int nv_build_shadow_data(NvShadowData* out, const NvGlobals* globals, const float sunDirection[3], float sunJitter, int checkerboard, uint32_t width,
                         uint32_t height)
{
	if (!out || !globals || !sunDirection || !width || !height)
		return NV_EINVAL;
	float inverse[16];
	if (inverse_view_projection(globals, inverse) != NV_OK)
		return NV_EINVAL;
	memset(out, 0, sizeof(*out));
	memcpy(out->inverseViewProjection, inverse, sizeof(inverse));
	for (int k = 0; k < 3; ++k)
		out->sunDirection[k] = sunDirection[k];
	out->sunJitter = sunJitter;
	out->imageSize[0] = (float)width;
	out->imageSize[1] = (float)height;
	out->checkerboard = checkerboard;
	return NV_OK;
}

// src/niagara.cpp:1002-1020
int nv_assign_visibility_offsets(NvMeshDraw* draws, uint32_t drawCount, const NvMesh* meshes, uint32_t meshCount,
                                 uint32_t* out_slots, uint32_t* out_postPassMask)
{
	if ((!draws && drawCount) || !meshes)
		return NV_EINVAL;
	uint32_t slots = 0, mask = 0;
	for (uint32_t i = 0; i < drawCount; ++i)
	{
		if (draws[i].meshIndex >= meshCount)
			return NV_EINVAL;
		const NvMesh& mesh = meshes[draws[i].meshIndex];
		draws[i].meshletVisibilityOffset = slots;
		uint32_t widest = 0;
		for (uint32_t l = 0; l < mesh.lodCount && l < NV_MAX_LODS; ++l)
			if (mesh.lods[l].meshletCount > widest)
				widest = mesh.lods[l].meshletCount;
		slots += widest;
		mask |= 1u << draws[i].postPass;
	}
	if (out_slots)
		*out_slots = slots;
	if (out_postPassMask)
		*out_postPassMask = mask;
	return NV_OK;
}

// the names of the triangles of indexed draws: the prefix of the draws' widest LODs, as the function above does for meshlets
int nv_assign_triangle_offsets(const NvMeshDraw* draws, uint32_t drawCount, const NvMesh* meshes, uint32_t meshCount, uint64_t* offsets)
{
	if ((!draws && drawCount) || (!meshes && meshCount) || !offsets)
		return NV_EINVAL;
	uint64_t at = 0;
	offsets[0] = 0;
	for (uint32_t i = 0; i < drawCount; ++i)
	{
		uint32_t widest = 0;
		if (draws[i].meshIndex < meshCount)
		{
			const NvMesh& mesh = meshes[draws[i].meshIndex];
			for (uint32_t l = 0; l < mesh.lodCount && l < NV_MAX_LODS; ++l)
				if (mesh.lods[l].indexCount / 3u > widest)
					widest = mesh.lods[l].indexCount / 3u;
		}
		at += widest;
		offsets[i + 1] = at;
	}
	return at > (1ull << 34) - 2ull ? NV_EINVAL : NV_OK;
}

namespace
{
// src/niagara.cpp:449-481
struct Pcg32
{
	uint64_t state, inc;
	uint32_t next()
	{
		uint64_t old = state;
		state = old * 6364136223846793005ULL + (inc | 1);
		uint32_t xs = (uint32_t)(((old >> 18u) ^ old) >> 27u);
		uint32_t rot = (uint32_t)(old >> 59u);
		return (xs >> rot) | (xs << ((32 - rot) & 31));
	}
	double unit() { return next() / double(1ull << 32); }
};
} // namespace

// src/niagara.cpp:969-998 (rngstate.state = 0x42, default inc); the three rand01() of the axis are drawn x, y, z
int nv_synth_draws(NvMeshDraw* draws, uint32_t drawCount, uint32_t meshCount, float sceneRadius)
{
	if ((!draws && drawCount) || !meshCount)
		return NV_EINVAL;
	Pcg32 rng = { 0x42, 0xda3e39cb94b95bdbULL };
	for (uint32_t i = 0; i < drawCount; ++i)
	{
		NvMeshDraw& d = draws[i];
		memset(&d, 0, sizeof(d));
		const uint32_t meshIndex = rng.next() % meshCount;
		for (int k = 0; k < 3; ++k)
			d.position[k] = float(rng.unit()) * sceneRadius * 2 - sceneRadius;
		d.scale = float(rng.unit()) + 1;
		d.scale *= 2;
		float ax = float(rng.unit()) * 2 - 1;
		float ay = float(rng.unit()) * 2 - 1;
		float az = float(rng.unit()) * 2 - 1;
		const float inv = 1.0f / sqrtf((ax * ax + ay * ay) + az * az);
		ax *= inv, ay *= inv, az *= inv;
		const float angle = (float(rng.unit()) * 90.f) * 0.01745329251994329576923690768489f;
		const float s = sinf(angle * 0.5f);
		d.orientation[0] = ax * s;
		d.orientation[1] = ay * s;
		d.orientation[2] = az * s;
		d.orientation[3] = cosf(angle * 0.5f);
		d.meshIndex = meshIndex;
	}
	return NV_OK;
}

// src/scene.cpp:207-220 with glm's component-wise forms: center += v; center /= float(n); radius = max(radius,
// distance(center, v)), distance = sqrt((dx*dx + dy*dy) + dz*dz).  Sequential on purpose: the sum's rounding is part of
// the result.
int nv_mesh_bounds(const float* positions, uint32_t vertexCount, float out_center[3], float* out_radius)
{
	if (!positions || !out_center || !out_radius || vertexCount == 0)
		return NV_EINVAL;
	float cx = 0.0f, cy = 0.0f, cz = 0.0f;
	for (uint32_t i = 0; i < vertexCount; ++i)
	{
		cx += positions[3 * i + 0];
		cy += positions[3 * i + 1];
		cz += positions[3 * i + 2];
	}
	const float n = (float)vertexCount;
	cx /= n;
	cy /= n;
	cz /= n;
	float radius = 0.0f;
	for (uint32_t i = 0; i < vertexCount; ++i)
	{
		const float dx = cx - positions[3 * i + 0], dy = cy - positions[3 * i + 1], dz = cz - positions[3 * i + 2];
		const float d = sqrtf((dx * dx + dy * dy) + dz * dz);
		radius = radius < d ? d : radius; // std::max(radius, d)
	}
	out_center[0] = cx;
	out_center[1] = cy;
	out_center[2] = cz;
	*out_radius = radius;
	return NV_OK;
}

// ---- scene cache (src/scenecache.cpp) ----
// SceneHeader, src/scenecache.cpp:16-55, as the reference's compiler lays it out (vec3 / quat are plain floats; the
// uint64_t makes the struct 8-aligned): 160 bytes.
namespace
{
struct SceneCacheHeader
{
	uint32_t magic, version;
	uint64_t hashMeta;
	uint32_t meshletMaxVertices, meshletMaxTriangles;
	uint8_t clrtMode, compressed, pad[2];
	uint32_t compressedVertexBytes, compressedIndexBytes, compressedMeshletDataBytes, compressedMeshletVtx0Bytes;
	uint32_t vertexCount, indexCount, meshletCount, meshletdataCount, meshletvtx0Count, meshCount;
	uint32_t materialCount, drawCount, texturePathCount, lightCount, animationCount, keyframeCount;
	uint32_t ommArrayDataSize, ommIndexDataSize, ommDescCount, ommStates;
	float cameraPosition[3], cameraOrientation[4], cameraFovY, cameraZnear;
	float sunDirection[3];
	uint32_t tail;
};
static_assert(sizeof(SceneCacheHeader) == 160, "SceneHeader layout (src/scenecache.cpp:16-55)");
static_assert(offsetof(SceneCacheHeader, vertexCount) == 44 && offsetof(SceneCacheHeader, cameraPosition) == 108, "SceneHeader offsets");

const uint32_t kSceneCacheMagic = 0x434E4353u; // 'SCNC', src/scenecache.cpp:12
const uint32_t kSceneCacheVersion = 7;         // src/scenecache.cpp:13
const uint64_t kVertexBytes = 16;              // Vertex, src/scene.h:60-66
const uint64_t kMaterialBytes = 64;            // Material, src/scene.h:25-37
} // namespace

int nv_scenecache_info(const char* path, NvSceneCacheInfo* out)
{
	if (!path || !out)
		return NV_EINVAL;
	FILE* f = fopen(path, "rb");
	if (!f)
		return NV_EIO;
	SceneCacheHeader h;
	const size_t got = fread(&h, 1, sizeof(h), f);
	uint64_t fileSize = 0;
	if (fseek(f, 0, SEEK_END) == 0)
		fileSize = (uint64_t)ftell(f);
	fclose(f);
	// src/scenecache.cpp:276-293 (the caller-dependent fields are handed back instead of compared)
	if (got < sizeof(h) || h.magic != kSceneCacheMagic || h.version != kSceneCacheVersion || h.meshletMaxVertices != NV_MESH_MAXVTX ||
	    h.meshletMaxTriangles != NV_MESH_MAXTRI)
		return NV_EFORMAT;

	memset(out, 0, sizeof(*out));
	out->version = h.version;
	out->compressed = h.compressed;
	out->clrtMode = h.clrtMode;
	out->ommStates = h.ommStates;
	out->hashMeta = h.hashMeta;
	out->meshletMaxVertices = h.meshletMaxVertices;
	out->meshletMaxTriangles = h.meshletMaxTriangles;
	out->vertexCount = h.vertexCount;
	out->indexCount = h.indexCount;
	out->meshletCount = h.meshletCount;
	out->meshletdataCount = h.meshletdataCount;
	out->meshletvtx0Count = h.meshletvtx0Count;
	out->meshCount = h.meshCount;
	out->materialCount = h.materialCount;
	out->drawCount = h.drawCount;
	out->texturePathCount = h.texturePathCount;
	out->lightCount = h.lightCount;
	out->animationCount = h.animationCount;
	out->keyframeCount = h.keyframeCount;
	memcpy(out->cameraPosition, h.cameraPosition, sizeof(h.cameraPosition));
	memcpy(out->cameraOrientation, h.cameraOrientation, sizeof(h.cameraOrientation));
	out->cameraFovY = h.cameraFovY;
	out->cameraZnear = h.cameraZnear;
	memcpy(out->sunDirection, h.sunDirection, sizeof(h.sunDirection));
	out->fileSize = fileSize;

	// section order of saveSceneCache, src/scenecache.cpp:163-186
	uint64_t off = sizeof(h);
	out->vertexOffset = off;
	out->vertexBytes = h.compressed ? h.compressedVertexBytes : (uint64_t)h.vertexCount * kVertexBytes;
	off += out->vertexBytes;
	out->indexOffset = off;
	out->indexBytes = h.compressed ? h.compressedIndexBytes : (uint64_t)h.indexCount * 4u;
	off += out->indexBytes;
	out->meshletOffset = off;
	off += (uint64_t)h.meshletCount * sizeof(NvMeshlet);
	out->meshletdataOffset = off;
	out->meshletdataBytes = h.compressed ? h.compressedMeshletDataBytes : (uint64_t)h.meshletdataCount * 4u;
	off += out->meshletdataBytes;
	off += h.compressed ? h.compressedMeshletVtx0Bytes : (uint64_t)h.meshletvtx0Count * 2u;
	out->meshOffset = off;
	off += (uint64_t)h.meshCount * sizeof(NvMesh);
	off += (uint64_t)h.materialCount * kMaterialBytes;
	out->drawOffset = off;
	off += (uint64_t)h.drawCount * sizeof(NvMeshDraw);
	if (off > fileSize)
		return NV_EFORMAT; // truncated
	return NV_OK;
}

int nv_scenecache_read(const char* path, const NvSceneCacheInfo* info, NvMesh* meshes, NvMeshlet* meshlets, NvMeshDraw* draws)
{
	if (!path || !info)
		return NV_EINVAL;
	FILE* f = fopen(path, "rb");
	if (!f)
		return NV_EIO;
	int rc = NV_OK;
	const struct
	{
		void* dst;
		uint64_t offset, bytes;
	} parts[3] = { { meshlets, info->meshletOffset, (uint64_t)info->meshletCount * sizeof(NvMeshlet) },
		           { meshes, info->meshOffset, (uint64_t)info->meshCount * sizeof(NvMesh) },
		           { draws, info->drawOffset, (uint64_t)info->drawCount * sizeof(NvMeshDraw) } };
	for (int i = 0; i < 3 && rc == NV_OK; ++i)
	{
		if (!parts[i].dst || !parts[i].bytes)
			continue;
		if (fseek(f, (long)parts[i].offset, SEEK_SET) != 0 || fread(parts[i].dst, 1, parts[i].bytes, f) != parts[i].bytes)
			rc = NV_EIO;
	}
	fclose(f);
	return rc;
}

// src/scenecache.cpp:183-186: Light, Animation and Keyframe records, raw, directly behind the draws
int nv_scenecache_animations(const char* path, const NvSceneCacheInfo* info, NvLight* lights, NvAnimation* animations, NvKeyframe* keyframes)
{
	if (!path || !info)
		return NV_EINVAL;
	FILE* f = fopen(path, "rb");
	if (!f)
		return NV_EIO;
	uint64_t fileSize = 0;
	if (fseek(f, 0, SEEK_END) == 0)
		fileSize = (uint64_t)ftell(f);
	struct
	{
		void* dst;
		uint64_t offset, bytes;
	} parts[3] = { { lights, 0, (uint64_t)info->lightCount * sizeof(NvLight) },
		           { animations, 0, (uint64_t)info->animationCount * sizeof(NvAnimation) },
		           { keyframes, 0, (uint64_t)info->keyframeCount * sizeof(NvKeyframe) } };
	uint64_t off = info->drawOffset + (uint64_t)info->drawCount * sizeof(NvMeshDraw);
	for (int i = 0; i < 3; ++i)
	{
		parts[i].offset = off;
		off += parts[i].bytes;
	}
	int rc = off > fileSize ? NV_EFORMAT : NV_OK; // truncated
	for (int i = 0; i < 3 && rc == NV_OK; ++i)
	{
		if (!parts[i].dst || !parts[i].bytes)
			continue;
		if (fseek(f, (long)parts[i].offset, SEEK_SET) != 0 || fread(parts[i].dst, 1, parts[i].bytes, f) != parts[i].bytes)
			rc = NV_EIO;
	}
	fclose(f);
	return rc;
}

// ---- keyframe animation (src/niagara.cpp:1368-1409; animmath.h is the text) ----
int nv_animation_validate_host(const NvAnimation* animations, uint32_t animationCount, uint32_t keyframeCount, uint32_t drawCount, uint32_t lightCount,
                               uint32_t* out_reason, uint32_t* out_index)
{
	uint32_t reason = NV_ANIM_OK, at = 0;
	if (!animations && animationCount)
		return NV_EINVAL;
	for (uint32_t i = 0; i < animationCount && reason == NV_ANIM_OK; ++i)
	{
		const NvAnimation& a = animations[i];
		if (a.keyframeCount == 0)
			reason = NV_ANIM_NO_KEYFRAMES;
		else if (a.keyframeCount > 0x7fffffffu || a.keyframeOffset > keyframeCount || a.keyframeCount > keyframeCount - a.keyframeOffset)
			reason = NV_ANIM_KEYFRAME_RANGE;
		else if (!(a.period > 0.0f) || !(a.period <= FLT_MAX) || !(fabsf(a.startTime) <= FLT_MAX))
			reason = NV_ANIM_PERIOD;
		else if (a.drawIndex >= 0 && (uint32_t)a.drawIndex >= drawCount)
			reason = NV_ANIM_DRAW_INDEX;
		else if (a.lightIndex >= 0 && (uint32_t)a.lightIndex >= lightCount)
			reason = NV_ANIM_LIGHT_INDEX;
		at = i;
	}
	// duplicates: the smallest animation index that repeats an earlier one's target (sorted by (target, animation))
	for (int pass = 0; pass < 2 && reason == NV_ANIM_OK; ++pass)
	{
		std::vector<uint64_t> keys;
		try
		{
			for (uint32_t i = 0; i < animationCount; ++i)
			{
				const int32_t target = pass ? animations[i].lightIndex : animations[i].drawIndex;
				if (target >= 0)
					keys.push_back((uint64_t)(uint32_t)target << 32 | i);
			}
		}
		catch (...)
		{
			return NV_ENOMEM;
		}
		std::sort(keys.begin(), keys.end());
		uint32_t first = 0xffffffffu;
		for (size_t k = 1; k < keys.size(); ++k)
			if (keys[k] >> 32 == keys[k - 1] >> 32 && (uint32_t)keys[k] < first)
				first = (uint32_t)keys[k];
		if (first != 0xffffffffu)
		{
			reason = pass ? NV_ANIM_DUPLICATE_LIGHT : NV_ANIM_DUPLICATE_DRAW;
			at = first;
		}
	}
	if (out_reason)
		*out_reason = reason;
	if (out_index)
		*out_index = reason == NV_ANIM_OK ? 0u : at;
	return reason == NV_ANIM_OK ? NV_OK : NV_EINVAL;
}

int nv_animation_phase_host(const NvAnimation* animations, const uint32_t* which, const double* times, uint64_t n, uint8_t* out_skipped, uint32_t* out_index0,
                            uint32_t* out_index1, float* out_t)
{
	if (n && (!animations || !which || !times || !out_skipped || !out_index0 || !out_index1 || !out_t))
		return NV_EINVAL;
	for (uint64_t i = 0; i < n; ++i)
	{
		const NvAnimation& a = animations[which[i]];
		if (!(fabs(times[i]) <= DBL_MAX) || a.keyframeCount == 0 || a.keyframeCount > 0x7fffffffu)
			return NV_EINVAL;
		nv::AnimPhase ph;
		out_skipped[i] = nv::anim_phase(times[i], a.startTime, a.period, a.keyframeCount, ph) ? 0 : 1;
		if (out_skipped[i])
			continue;
		out_index0[i] = ph.index0;
		out_index1[i] = ph.index1;
		out_t[i] = ph.t;
	}
	return NV_OK;
}

int nv_animate_draws_host(double time, const NvAnimation* animations, uint32_t animationCount, const NvKeyframe* keyframes, uint32_t keyframeCount,
                          NvMeshDraw* draws, uint32_t drawCount, NvLight* lights, uint32_t lightCount)
{
	if (!(fabs(time) <= DBL_MAX) || (animationCount && (!animations || !keyframes)))
		return NV_EINVAL;
	const int rc = nv_animation_validate_host(animations, animationCount, keyframeCount, drawCount, lightCount, nullptr, nullptr);
	if (rc != NV_OK)
		return rc;
	for (uint32_t i = 0; i < animationCount; ++i)
	{
		const NvAnimation& a = animations[i];
		nv::AnimPhase ph;
		if (!nv::anim_phase(time, a.startTime, a.period, a.keyframeCount, ph))
			continue;
		const NvKeyframe& k0 = keyframes[(size_t)a.keyframeOffset + ph.index0];
		const NvKeyframe& k1 = keyframes[(size_t)a.keyframeOffset + ph.index1];
		const float t = ph.t;
		const float px = nv::anim_mix(k0.translation[0], k1.translation[0], t), py = nv::anim_mix(k0.translation[1], k1.translation[1], t),
		            pz = nv::anim_mix(k0.translation[2], k1.translation[2], t);
		if (a.drawIndex >= 0 && draws)
		{
			NvMeshDraw& d = draws[a.drawIndex];
			const nv::AnimQuat q = nv::anim_slerp(nv::AnimQuat{ k0.rotation[0], k0.rotation[1], k0.rotation[2], k0.rotation[3] },
			                                      nv::AnimQuat{ k1.rotation[0], k1.rotation[1], k1.rotation[2], k1.rotation[3] }, t);
			d.position[0] = px;
			d.position[1] = py;
			d.position[2] = pz;
			d.scale = nv::anim_mix(k0.scale, k1.scale, t);
			d.orientation[0] = q.x;
			d.orientation[1] = q.y;
			d.orientation[2] = q.z;
			d.orientation[3] = q.w;
		}
		if (a.lightIndex >= 0 && lights)
		{
			NvLight& l = lights[a.lightIndex];
			l.position[0] = px;
			l.position[1] = py;
			l.position[2] = pz;
		}
	}
	return NV_OK;
}

// contiguous ranges, remainder spread over the first ranks
void nv_shard_range(uint64_t total, uint32_t rank, uint32_t world, uint64_t* begin, uint64_t* end)
{
	if (!world)
		world = 1;
	uint64_t base = total / world, rem = total % world;
	uint64_t b = base * rank + (rank < rem ? rank : rem);
	uint64_t e = b + base + (rank < rem ? 1 : 0);
	if (begin)
		*begin = b;
	if (end)
		*end = e;
}

} // extern "C"
