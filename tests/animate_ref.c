/* animate_ref.c — an independent restatement of niagara's keyframe animation loop (src/niagara.cpp:1366-1410) with glm::mix and glm::slerp
 * written out from glm's published definitions (glm/detail/func_common.inl, glm/ext/quaternion_common.inl, glm/detail/type_quat.inl).  Test
 * infrastructure: it shares no text with niagara_amd/csrc/animmath.h.
 *
 * Builds twice.  Default (REAL = float): the bits nv_animate_draws_host must write, sinf / acosf being this machine's libm.  -DREAL=double:
 * the reference value of the trigonometric branch.  In that build the time statements, the quaternion dot and with it the two decisions
 * (negate y, linear or trigonometric) stay fp32 — they are pinned bit for bit by the fp32 build — and what follows the dot (acos, the three
 * sines, the products, the sum, the division; mix) is evaluated in double from the fp32 inputs. */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifndef REAL
#define REAL float
#endif

typedef struct
{
	int32_t drawIndex, lightIndex;
	float startTime, period;
	uint32_t keyframeOffset, keyframeCount;
} Animation;

typedef struct
{
	float translation[3];
	float scale;
	float rotation[4]; /* x, y, z, w */
} Keyframe;

typedef struct
{
	float position[3];
	float scale;
	float orientation[4]; /* x, y, z, w */
	uint32_t meshIndex, meshletVisibilityOffset, postPass, materialIndex;
} MeshDraw;

typedef struct
{
	float position[3];
	float range;
	float color[3];
	float intensity;
} Light;

typedef struct
{
	REAL w, x, y, z;
} quat;

int ar_real_bytes(void) { return (int)sizeof(REAL); }

static REAL r_sin(REAL v) { return sizeof(REAL) == 4 ? (REAL)sinf((float)v) : (REAL)sin((double)v); }
static REAL r_acos(REAL v) { return sizeof(REAL) == 4 ? (REAL)acosf((float)v) : (REAL)acos((double)v); }

/* glm::mix(x, y, a) for floating a: x * (1 - a) + y * a */
static REAL mix(REAL x, REAL y, REAL a) { return x * ((REAL)1 - a) + y * a; }

/* glm::dot(qua, qua): compute_dot<qua>: tmp(a.w b.w, a.x b.x, a.y b.y, a.z b.z); (tmp.x + tmp.y) + (tmp.z + tmp.w) — always in fp32 here */
static float qdot32(const float* a, const float* b)
{
	const float tw = a[3] * b[3], tx = a[0] * b[0], ty = a[1] * b[1], tz = a[2] * b[2];
	return (tw + tx) + (ty + tz);
}

/* glm::slerp(x, y, a); flags: bit 0 = the trigonometric branch, bit 1 = y was negated */
static quat slerp(const float* xf, const float* yf, float af, unsigned* flags)
{
	const quat x = { (REAL)xf[3], (REAL)xf[0], (REAL)xf[1], (REAL)xf[2] };
	const quat y = { (REAL)yf[3], (REAL)yf[0], (REAL)yf[1], (REAL)yf[2] };
	const REAL a = (REAL)af;
	quat z = y;
	float cosTheta = qdot32(xf, yf);
	*flags = 0;
	/* "If cosTheta < 0, the interpolation will take the long way around the sphere.  To fix this, one quat must be negated." */
	if (cosTheta < 0.0f)
	{
		z.w = -y.w;
		z.x = -y.x;
		z.y = -y.y;
		z.z = -y.z;
		cosTheta = -cosTheta;
		*flags |= 2u;
	}
	if (cosTheta > 1.0f - FLT_EPSILON)
	{
		quat o = { mix(x.w, z.w, a), mix(x.x, z.x, a), mix(x.y, z.y, a), mix(x.z, z.z, a) };
		return o;
	}
	else
	{
		*flags |= 1u;
		const REAL angle = r_acos((REAL)cosTheta);
		const REAL s0 = r_sin(((REAL)1 - a) * angle), s1 = r_sin(a * angle), s = r_sin(angle);
		/* (s0 * x + s1 * z) / s: qua * scalar, qua + qua and qua / scalar are component-wise */
		quat o = { (s0 * x.w + s1 * z.w) / s, (s0 * x.x + s1 * z.x) / s, (s0 * x.y + s1 * z.y) / s, (s0 * x.z + s1 * z.z) / s };
		return o;
	}
}

/* src/niagara.cpp:1368-1378; returns 0 when the animation is skipped (:1370) */
static int phase(const Animation* an, double time, int* index0, int* index1, double* t)
{
	double index = (time - an->startTime) / an->period;
	if (index < 0)
		return 0;
	index = fmod(index, (double)an->keyframeCount);
	*index0 = (int)((unsigned)(int)index % an->keyframeCount);
	*index1 = (int)((unsigned)(*index0 + 1) % an->keyframeCount);
	*t = index - floor(index);
	return 1;
}

/* one sample per (animation which[i], time times[i]): out8 = position xyz, scale, orientation xyzw, in REAL widened to double */
void ar_eval(const Animation* anims, const Keyframe* keys, const uint32_t* which, const double* times, uint64_t n, uint8_t* skipped, uint32_t* i0,
             uint32_t* i1, float* tf, double* out8, uint8_t* flags)
{
	for (uint64_t i = 0; i < n; ++i)
	{
		const Animation* an = anims + which[i];
		int index0 = 0, index1 = 0;
		double t = 0;
		skipped[i] = !phase(an, times[i], &index0, &index1, &t);
		if (skipped[i])
			continue;
		const Keyframe* k0 = keys + an->keyframeOffset + index0;
		const Keyframe* k1 = keys + an->keyframeOffset + index1;
		const float ft = (float)t;
		unsigned f = 0;
		const quat q = slerp(k0->rotation, k1->rotation, ft, &f);
		i0[i] = (uint32_t)index0;
		i1[i] = (uint32_t)index1;
		tf[i] = ft;
		flags[i] = (uint8_t)f;
		double* o = out8 + 8 * i;
		for (int c = 0; c < 3; ++c)
			o[c] = (double)mix((REAL)k0->translation[c], (REAL)k1->translation[c], (REAL)ft);
		o[3] = (double)mix((REAL)k0->scale, (REAL)k1->scale, (REAL)ft);
		o[4] = (double)q.x;
		o[5] = (double)q.y;
		o[6] = (double)q.z;
		o[7] = (double)q.w;
	}
}

/* the loop itself, in array order (of two animations with one target the last one wins, as in the reference); draws / lights may be NULL */
void ar_apply(double time, const Animation* anims, uint32_t count, const Keyframe* keys, MeshDraw* draws, Light* lights)
{
	for (uint32_t i = 0; i < count; ++i)
	{
		const Animation* an = anims + i;
		int index0, index1;
		double t;
		if (!phase(an, time, &index0, &index1, &t))
			continue;
		const Keyframe* k0 = keys + an->keyframeOffset + index0;
		const Keyframe* k1 = keys + an->keyframeOffset + index1;
		const float ft = (float)t;
		if (an->drawIndex >= 0 && draws)
		{
			MeshDraw* d = draws + an->drawIndex;
			unsigned f;
			const quat q = slerp(k0->rotation, k1->rotation, ft, &f);
			for (int c = 0; c < 3; ++c)
				d->position[c] = (float)mix((REAL)k0->translation[c], (REAL)k1->translation[c], (REAL)ft);
			d->scale = (float)mix((REAL)k0->scale, (REAL)k1->scale, (REAL)ft);
			d->orientation[0] = (float)q.x;
			d->orientation[1] = (float)q.y;
			d->orientation[2] = (float)q.z;
			d->orientation[3] = (float)q.w;
		}
		if (an->lightIndex >= 0 && lights)
		{
			Light* l = lights + an->lightIndex;
			for (int c = 0; c < 3; ++c)
				l->position[c] = (float)mix((REAL)k0->translation[c], (REAL)k1->translation[c], (REAL)ft);
		}
	}
}
