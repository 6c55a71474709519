/*
 * glsl_rayquery_shim.h — a CPU rayQueryEXT / accelerationStructureEXT and the material sampler's textureLod, for the translation of
 * shadow.comp.glsl (TEST INFRASTRUCTURE).  Included by glsl_shim.h behind glsl_shade_shim.h when a translation unit is built with -DREF_SHADOW
 * (oracle/Makefile).  With it every statement of shadow.comp.glsl runs on the CPU as the reference wrote it; what GL_EXT_ray_query leaves to
 * the implementation is modelled here.
 *
 * THE MODEL
 *
 * The acceleration structure is a list of instances in draw order; oracle/ref_runner.cpp (ref_shadow) builds it from the draw array as
 * fillInstanceRT (src/scenert.cpp:504-518) states:
 *   - one instance per draw, and the instance id is the draw index (the instance buffer is filled in draw order; InstanceIdEXT is that index);
 *   - mask = (1 << postPass) & 0xff (VkAccelerationStructureInstanceKHR::mask has 8 bits, :515); an instance takes part in a query iff
 *     mask & cullMask != 0, the cull mask being the 0xff of shadow.comp.glsl:81 / :89;
 *   - FORCE_OPAQUE iff postPass == 0 (:516);
 *   - geometry: the triangles of meshes[meshIndex].lods[lodRT] when postPass <= 1, none otherwise (:517: a null BLAS reference).
 * Where Vulkan leaves the outcome undefined the library defines it ("Casting instances" and "Triangles"), and the runner
 * follows: a draw with a non-finite position, orientation or scale, with scale <= 0, or with meshIndex >= meshCount has no geometry; a mesh with
 * lodRT >= 8 or lodRT >= lodCount has none; a triangle with an index position >= the index capacity or a corner >= the vertex capacity is left
 * out.  A ray with a non-finite origin or direction component meets nothing (§4.16, "Per invocation").
 *
 * rayQueryInitializeEXT records the ray and appends origin, direction, tmin, tmax and flags to the record of the running invocation
 * (shim_rq_log, set by the runner before every shader main()).
 *
 * rayQueryProceedEXT walks the instances in index order and the triangles of each in index order, from where the last call stopped.  For a
 * triangle the predicate accepts: an opaque instance commits the hit, and gl_RayFlagsTerminateOnFirstHitEXT ends the walk (false); a non-opaque
 * instance hands the triangle out as the candidate — instance id, primitive index, barycentrics — and returns true.  When the list is
 * exhausted, or after a commit under TerminateOnFirstHit, it returns false.  rayQueryConfirmIntersectionEXT commits the candidate.
 * rayQueryGetIntersectionTypeEXT(rq, true) is committed-triangle or none.  Both queries of the shader set TerminateOnFirstHit; closest-hit
 * ordering (shrinking tmax to a committed hit) is therefore not modelled, and a query without the flag aborts.
 * gl_RayFlagsForceOpacityMicromap2StateEXT has nothing to act on: there are no opacity micromaps in the model (the reference's are an option
 * of its scene build), so a non-opaque triangle stays a candidate under it.
 *
 * THE GEOMETRIC PREDICATE IS THE LIBRARY'S, NOT PINNED HERE.  Vulkan leaves the ray/triangle test to the implementation, and the library
 * defines its own: the object-space ray of an instance, the watertight test T with its fp64 branch, and the barycentrics
 * (V / det, W / det) as rt_hit_uv forms them.  They come from niagara_amd/csrc/rtmath.h and rtalpha.h (rt_object_ray, rt_ray_setup,
 * rt_triangle_uvw), as tools/rt_scene_check.cpp takes them on the host; T has its own tests.  This shim pins every statement AROUND T.
 *
 * textureLod(SAMP(id), uv, 0) is DESIGN.md §4.18's rule at lambda = 0, written once more over the decoded RGBA8 texels of level 0: REPEAT (the
 * fractional part of the coordinate), u = s size - 0.5, i0 = floor(u) and i0 + 1 wrapped into the level, weight u - floor(u), UNORM code / 255,
 * mix(x, y, a) = x (1 - a) + y a along x first, then y.  A non-finite coordinate gives index 0 and a NaN weight.  A texture id at or past the
 * table, or one whose chain does not lie in the set, is "no texture" (§4.19: alpha 1).  Every call is logged (id, uv, the alpha returned, and
 * the candidate it was made for: instance, primitive, barycentrics) so that the test can hold this sampler against nv_rt_alpha_sample_host,
 * and the uv against the restatement's interpolation, before it compares a mask.
 */
#pragma once

#include <stdlib.h>

#include <vector>

#include "../niagara_amd/csrc/rtalpha.h"

namespace glsl
{
namespace
{

/* ---- the acceleration structure */
struct ShimRtInstance
{
	float position[3], scale, orientation[4];
	uint mask;              /* (1 << postPass) & 0xff */
	bool opaque;            /* VK_GEOMETRY_INSTANCE_FORCE_OPAQUE_BIT_KHR */
	const nv::rt3* corners; /* 3 per triangle, object space; 0: no geometry */
	const uint8_t* kept;    /* per triangle: 0 = left out (an index or corner past the capacities) */
	uint triangles;
};
struct accelerationStructureEXT
{
	const ShimRtInstance* instances;
	uint count;
};

const uint gl_RayFlagsTerminateOnFirstHitEXT = 4u;           /* the values of GL_EXT_ray_query */
const uint gl_RayFlagsForceOpacityMicromap2StateEXT = 1024u; /* GL_EXT_opacity_micromap */
const uint gl_RayQueryCommittedIntersectionNoneEXT = 0u;
const uint gl_RayQueryCommittedIntersectionTriangleEXT = 1u;

/* what one invocation's queries did: the runner hands these back per invocation */
struct ShimRayLog
{
	float origin[3], dir[3], tmin, tmax;
	uint flags, queries;
	uint opaqueCommits, candidates, confirmed;
	uint committedInstance; /* ~0: none */
};
static ShimRayLog shim_rq_scratch;
static ShimRayLog* shim_rq_log = &shim_rq_scratch;

/* every textureLod call, in order (see the end of this file) */
struct ShimSample
{
	uint id;
	float u, v, alpha;
	int instance, primitive; /* the candidate the walk handed out last: the one this sample belongs to */
	float baryX, baryY;
};
static std::vector<ShimSample> shim_rq_samples;
static ShimSample shim_rq_candidate; /* instance, primitive and barycentrics of the last candidate */

struct rayQueryEXT
{
	accelerationStructureEXT as;
	uint flags, cullMask;
	nv::rt3 o, d;
	float tmin, tmax;
	bool finite;
	uint instance, triangle; /* where the walk continues */
	bool haveRay;            /* `ray` is that of `instance` */
	nv::RtRay ray;
	int candidateInstance, candidatePrimitive;
	vec2 candidateBary;
	bool committed, ended;
};

inline void rayQueryInitializeEXT(rayQueryEXT& rq, accelerationStructureEXT as, uint flags, uint cullMask, vec3 origin, float tmin, vec3 dir, float tmax)
{
	if (!(flags & gl_RayFlagsTerminateOnFirstHitEXT))
		abort(); /* closest-hit ordering is not modelled (see the top) */
	rq.as = as;
	rq.flags = flags, rq.cullMask = cullMask;
	rq.o = nv::rt3{ origin.x, origin.y, origin.z }, rq.d = nv::rt3{ dir.x, dir.y, dir.z };
	rq.tmin = tmin, rq.tmax = tmax;
	rq.finite = nv::rt_finite(origin.x) && nv::rt_finite(origin.y) && nv::rt_finite(origin.z) && nv::rt_finite(dir.x) && nv::rt_finite(dir.y) && nv::rt_finite(dir.z);
	rq.instance = rq.triangle = 0;
	rq.haveRay = rq.committed = rq.ended = false;
	rq.candidateInstance = rq.candidatePrimitive = -1;
	ShimRayLog* l = shim_rq_log;
	l->origin[0] = origin.x, l->origin[1] = origin.y, l->origin[2] = origin.z;
	l->dir[0] = dir.x, l->dir[1] = dir.y, l->dir[2] = dir.z;
	l->tmin = tmin, l->tmax = tmax, l->flags = flags;
	l->queries++;
}

inline bool rayQueryProceedEXT(rayQueryEXT& rq)
{
	if (rq.ended || !rq.finite) /* a non-finite ray meets nothing */
		return false;
	for (; rq.instance < rq.as.count; rq.instance++, rq.triangle = 0, rq.haveRay = false)
	{
		const ShimRtInstance& in = rq.as.instances[rq.instance];
		if (!(in.mask & rq.cullMask & 0xffu) || !in.corners)
			continue;
		if (!rq.haveRay)
		{
			nv::rt3 o2, d2;
			nv::rt_object_ray(rq.o, rq.d, in.position, in.orientation, in.scale, &o2, &d2);
			rq.ray = nv::rt_ray_setup(o2, d2);
			rq.haveRay = true;
		}
		while (rq.triangle < in.triangles)
		{
			const uint t = rq.triangle++;
			nv::RtHit hit;
			if (!in.kept[t] || !nv::rt_triangle_uvw(rq.ray, in.corners[3 * t], in.corners[3 * t + 1], in.corners[3 * t + 2], rq.tmin, rq.tmax, &hit))
				continue;
			if (in.opaque)
			{
				rq.committed = true;
				shim_rq_log->opaqueCommits++;
				shim_rq_log->committedInstance = rq.instance;
				rq.ended = true; /* TerminateOnFirstHit */
				return false;
			}
			rq.candidateInstance = (int)rq.instance, rq.candidatePrimitive = (int)t;
			rq.candidateBary = vec2(hit.V / hit.det, hit.W / hit.det); /* rt_hit_uv's b1, b2 */
			shim_rq_log->candidates++;
			shim_rq_candidate.instance = rq.candidateInstance, shim_rq_candidate.primitive = rq.candidatePrimitive;
			shim_rq_candidate.baryX = rq.candidateBary.x, shim_rq_candidate.baryY = rq.candidateBary.y;
			return true;
		}
	}
	rq.ended = true;
	return false;
}

inline void rayQueryConfirmIntersectionEXT(rayQueryEXT& rq)
{
	rq.committed = true;
	rq.ended = true; /* TerminateOnFirstHit */
	shim_rq_log->confirmed++;
	shim_rq_log->committedInstance = (uint)rq.candidateInstance;
}

inline uint rayQueryGetIntersectionTypeEXT(const rayQueryEXT& rq, bool committed)
{
	if (!committed)
		abort(); /* the shader asks for the committed intersection only */
	return rq.committed ? gl_RayQueryCommittedIntersectionTriangleEXT : gl_RayQueryCommittedIntersectionNoneEXT;
}
/* the shader reads these of the candidate (committed = false) only */
inline int rayQueryGetIntersectionInstanceIdEXT(const rayQueryEXT& rq, bool) { return rq.candidateInstance; }
inline int rayQueryGetIntersectionPrimitiveIndexEXT(const rayQueryEXT& rq, bool) { return rq.candidatePrimitive; }
inline vec2 rayQueryGetIntersectionBarycentricsEXT(const rayQueryEXT& rq, bool) { return rq.candidateBary; }

/* ---- textureLod over the material set (level 0 of every texture, decoded RGBA8; R in bits 0-7, alpha in bits 24-31) */
struct ShimLevel0
{
	const uint32_t* texels; /* 0: "no texture" */
	uint width, height;
};
static const ShimLevel0* shim_rq_textures;
static uint shim_rq_texture_count;

inline void shim_repeat_axis(float x, uint size, size_t i[2], float* weight)
{
	float s = x - floorf(x);
	float u = s * (float)size - 0.5f;
	float fl = floorf(u);
	long long at = fl == fl && fabsf(fl) < 1e18f ? (long long)fl : 0;
	*weight = u - fl;
	i[0] = (size_t)(((at % (long long)size) + (long long)size) % (long long)size);
	i[1] = (size_t)((((at + 1) % (long long)size) + (long long)size) % (long long)size);
}
inline float shim_mix2(float t00, float t01, float t10, float t11, float a, float b) { return mix(mix(t00, t01, a), mix(t10, t11, a), b); }

inline vec4 textureLod(sampler2D s, vec2 uv, float lod)
{
	if (lod != 0.0f)
		abort(); /* level 0 only */
	vec4 out(1.0f);
	const uint id = s.t.id;
	if (id < shim_rq_texture_count && shim_rq_textures[id].texels)
	{
		const ShimLevel0& t = shim_rq_textures[id];
		size_t xi[2], yi[2];
		float a, b;
		shim_repeat_axis(uv.x, t.width, xi, &a);
		shim_repeat_axis(uv.y, t.height, yi, &b);
		vec4 t00 = shim_decode(t.texels, FORMAT_R8G8B8A8_UNORM, yi[0] * t.width + xi[0]), t01 = shim_decode(t.texels, FORMAT_R8G8B8A8_UNORM, yi[0] * t.width + xi[1]);
		vec4 t10 = shim_decode(t.texels, FORMAT_R8G8B8A8_UNORM, yi[1] * t.width + xi[0]), t11 = shim_decode(t.texels, FORMAT_R8G8B8A8_UNORM, yi[1] * t.width + xi[1]);
		out = vec4(shim_mix2(t00.x, t01.x, t10.x, t11.x, a, b), shim_mix2(t00.y, t01.y, t10.y, t11.y, a, b), shim_mix2(t00.z, t01.z, t10.z, t11.z, a, b),
		           shim_mix2(t00.w, t01.w, t10.w, t11.w, a, b));
	}
	ShimSample rec = shim_rq_candidate;
	rec.id = id, rec.u = uv.x, rec.v = uv.y, rec.alpha = out.w;
	shim_rq_samples.push_back(rec);
	return out;
}

} // namespace
} // namespace glsl
