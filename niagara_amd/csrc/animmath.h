// animmath.h — the arithmetic of the keyframe animation (src/niagara.cpp:1368-1409) in ONE place that compiles for the
// device (hipcc) and for the host (g++): animate.hip's kernel and host.cpp's nv_animate_draws_host run the same text, so the order of the
// operations is written once and the branch a sample takes is the same on both sides by construction.  Nothing else includes it;
// tests/animate_ref.c restates it independently.
//
// Build with -ffp-contract=off: every fp32 operation is one IEEE operation in the order written.  fp64 division, fmod and floor are exact or
// correctly rounded on both sides, so the keyframe pair and t agree bit for bit; sinf / acosf are the libraries' (the only difference).
#pragma once

#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NV_ANIM __host__ __device__ inline __attribute__((always_inline))
#else
#define NV_ANIM static inline
#endif

namespace nv
{

struct AnimPhase
{
	uint32_t index0, index1;
	float t;
};

struct AnimQuat // (x, y, z, w): NvMeshDraw.orientation's order
{
	float x, y, z, w;
};

// src/niagara.cpp:1368-1378.  false = the animation is skipped at `time` (:1370; an index that is not finite is skipped too: the reference
// leaves int(NaN) undefined).  keyframeCount is in [1, 2^31) (the validator)
NV_ANIM bool anim_phase(double time, float startTime, float period, uint32_t keyframeCount, AnimPhase& out)
{
	double index = (time - double(startTime)) / double(period);
	if (!(index >= 0.0) || !(index <= DBL_MAX))
		return false;
	index = fmod(index, double(keyframeCount));
	const uint32_t index0 = uint32_t(int32_t(index)) % keyframeCount;
	out.index0 = index0;
	out.index1 = (index0 + 1u) % keyframeCount;
	out.t = float(index - floor(index));
	return true;
}

// glm::mix: x * (1 - a) + y * a
NV_ANIM float anim_mix(float x, float y, float a)
{
	const float b = 1.0f - a;
	const float p = x * b;
	const float q = y * a;
	return p + q;
}

// glm::slerp(x, y, a) (glm/ext/quaternion_common.inl): the dot as glm's compute_dot<qua> sums it, (w w + x x) + (y y + z z)
NV_ANIM AnimQuat anim_slerp(AnimQuat x, AnimQuat y, float a)
{
	AnimQuat z = y;
	float cosTheta = (x.w * y.w + x.x * y.x) + (x.y * y.y + x.z * y.z);
	if (cosTheta < 0.0f)
	{
		z.x = -y.x;
		z.y = -y.y;
		z.z = -y.z;
		z.w = -y.w;
		cosTheta = -cosTheta;
	}
	AnimQuat o;
	if (cosTheta > 1.0f - FLT_EPSILON)
	{
		o.x = anim_mix(x.x, z.x, a);
		o.y = anim_mix(x.y, z.y, a);
		o.z = anim_mix(x.z, z.z, a);
		o.w = anim_mix(x.w, z.w, a);
		return o;
	}
	const float angle = acosf(cosTheta);
	const float s0 = sinf((1.0f - a) * angle);
	const float s1 = sinf(a * angle);
	const float d = sinf(angle);
	o.x = (s0 * x.x + s1 * z.x) / d;
	o.y = (s0 * x.y + s1 * z.y) / d;
	o.z = (s0 * x.z + s1 * z.z) / d;
	o.w = (s0 * x.w + s1 * z.w) / d;
	return o;
}

} // namespace nv
