// rtmath.h — the arithmetic of the ray-traced shadow pass in ONE place that compiles for the device (hipcc) and for the
// host (g++): the ray of an invocation, the object-space ray of an instance, the watertight triangle test T, the box test and the skip-link
// traversal of the scene blob rtbuild.cpp writes.  shadowtrace.hip's kernel and nv_rt_scene_trace_host run the same text.
//
// Build with -ffp-contract=off.  T and the ray set-up are the RESULT: every fp32 operation is one IEEE operation in the order written, and
// tests/shadow_ref.c restates them without a BVH.  The box test is an acceleration: its arithmetic is free, its obligation is never to
// reject a node whose subtree holds a triangle T accepts for the ray (the margins are derived in DESIGN.md §4.16 and named RT_* below).
#pragma once

#include <stdint.h>

#include "../../include/niagara_vis.h"

#if defined(__HIPCC__)
#define NV_RT __host__ __device__ inline __attribute__((always_inline))
#else
#define NV_RT static inline
#endif

namespace nv
{

struct rt3
{
	float x, y, z;
};

// what the alpha test of rtalpha.h reads besides the blob: the caller's buffers, every index checked against its count before the load.  Here,
// not there: it is a field of the alpha trace's kernel arguments (args.h), which do not need the test's text.  SET is the residency of the
// texture set, texmath.h's TxDecoded or TxBlocks (only named here: a translation unit that instantiates this has included texmath.h)
struct TxDecoded;
struct TxBlocks;
template <typename SET>
struct RtAlphaInputs
{
	typedef SET Set;
	const NvMeshDraw* draws;
	const NvMaterial* materials;
	const typename SET::Desc* textures; // == NvTextureDesc / NvTextureBlockDesc; entry 0 is "no texture"
	const typename SET::Unit* data;     // the decoded texels / the DDS payloads, 16-byte aligned
	uint64_t extent;                    // texelWords / units16
	uint32_t drawCount, materialCount, textureCount;
};

struct __attribute__((aligned(16))) RtF4 // one 16-byte load
{
	float x, y, z, w;
};

// ---- the blob (offsets in bytes from its start, every section 16-byte aligned; no pointers)
constexpr uint32_t RT_MAGIC = 0x5452564eu; // "NVRT"
constexpr uint32_t RT_VERSION = 1u;
constexpr uint32_t RT_LEAF_MAX = 4u;          // triangles per BLAS leaf at most (a TLAS leaf holds one instance)
constexpr uint32_t RT_LEAF_SHIFT = 29u;       // leaf word = count << 29 | first; 0 = inner node
constexpr uint32_t RT_LEAF_FIRST = (1u << RT_LEAF_SHIFT) - 1u;

struct RtHeader // 64 bytes
{
	uint32_t magic, version, bytes, meshCount; // meshCount = entries of the BLAS table (one per mesh; nodeCount 0 = no triangles)
	uint32_t tlasNodes, instances, blasNodes, triangles;
	uint32_t tableOff, tlasOff, instOff, blasOff;
	uint32_t triOff;
	float padOrigin; // the TLAS boxes' ray-dependent padding per unit of max |origin component| (RT_PAD_K u times the worst instance's factor)
	uint32_t drawCount, flags; // flags: RT_FLAG_* (0 in nv_rt_scene_build's blob)
};
struct RtBlas // 32 bytes = two RtF4
{
	uint32_t nodeFirst, nodeCount, triFirst, triCount; // nodes and triangles of this BLAS; a node's skip and a leaf's first are relative to them
	float maxAbs;    // the largest |coordinate| of its vertices
	float maxExtent; // the largest extent of one triangle's box along an axis
	uint32_t reserved[2];
};
struct RtNode // 32 bytes = two RtF4: {lo, skip} {hi, leaf}
{
	float lo[3];
	uint32_t skip;
	float hi[3];
	uint32_t leaf;
};
struct RtInstance // 64 bytes: {position, scale} {orientation} {drawId, postPass, blas, 0} {0}
{
	float position[3], scale, orientation[4];
	uint32_t drawId, postPass, blas, reserved[5];
};
// a triangle is three RtF4 {v.x, v.y, v.z, w}, in leaf order; w is 0, or with RT_FLAG_TEXCOORDS the BITS tu | tv << 16 of the corner's fp16 texcoord
// (never a number: rtalpha.h reads them with rt_bits)
constexpr uint32_t RT_FLAG_TEXCOORDS = 1u; // nv_rt_scene_build_textured wrote the blob
constexpr uint32_t RT_FLAGS_KNOWN = RT_FLAG_TEXCOORDS;

// ---- margins of the box test
constexpr float RT_U = 5.9604644775390625e-8f; // 2^-24
constexpr float RT_PAD_K = 32.0f;              // eps = RT_PAD_K u (max|o'| + max|vertex coordinate|): the analysis needs 14 u
constexpr float RT_TINY = 1e-37f;              // a slab distance of exactly 0 moves outward by this: 0 x inf cannot arise
constexpr float RT_T_UP = 1.00000095367431640625f; // 1 + 2^-20: rounds the widened t range outward

NV_RT uint32_t rt_bits(float f)
{
	uint32_t u;
	__builtin_memcpy(&u, &f, 4);
	return u;
}
NV_RT bool rt_finite(float f) { return (rt_bits(f) & 0x7f800000u) != 0x7f800000u; }
NV_RT float rt_max3abs(rt3 v)
{
	const float a = __builtin_fabsf(v.x), b = __builtin_fabsf(v.y), c = __builtin_fabsf(v.z);
	const float m = a < b ? b : a;
	return m < c ? c : m;
}

// ---- the ray of an invocation (shadow.comp.glsl:125-150)

// final.comp.glsl:52-54 / shadow.comp.glsl:133-135: wposh = inverseViewProjection * (cx, cy, depth, 1), wpos = wposh.xyz / wposh.w;
// m column-major, the sums left to right.  shade_final_kernel and the shadow trace share it.
NV_RT rt3 rt_unproject(const float* m, float cx, float cy, float depth)
{
	const float hx = ((m[0] * cx + m[4] * cy) + m[8] * depth) + m[12] * 1.0f;
	const float hy = ((m[1] * cx + m[5] * cy) + m[9] * depth) + m[13] * 1.0f;
	const float hz = ((m[2] * cx + m[6] * cy) + m[10] * depth) + m[14] * 1.0f;
	const float hw = ((m[3] * cx + m[7] * cy) + m[11] * depth) + m[15] * 1.0f;
	return rt3{ hx / hw, hy / hw, hz / hw };
}

// math.h:99-102 gradientNoise(vec2(x, y))
NV_RT float rt_gradient_noise(float x, float y)
{
	const float inner = x * 0.06711056f + y * 0.00583715f;
	const float f0 = inner - __builtin_floorf(inner);
	const float n1 = 52.9829189f * f0;
	return n1 - __builtin_floorf(n1);
}

NV_RT rt3 rt_normalize(rt3 v)
{
	const float l = __builtin_sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z);
	return rt3{ v.x / l, v.y / l, v.z / l };
}

// origin and direction of the pixel (px, py) whose depth texel is `depth`
NV_RT void rt_pixel_ray(const float* sun, float sunJitter, const float* inverseViewProjection, const float* imageSize, uint32_t px, uint32_t py,
                        float depth, rt3* origin, rt3* dir)
{
	const float uvx = ((float)px + 0.5f) / imageSize[0], uvy = ((float)py + 0.5f) / imageSize[1];
	*origin = rt_unproject(inverseViewProjection, uvx * 2.0f - 1.0f, 1.0f - uvy * 2.0f, depth);
	rt3 d = { sun[0], sun[1], sun[2] };
	d.x = d.x + (rt_gradient_noise((float)px, (float)py) * 2.0f - 1.0f) * sunJitter;
	d.z = d.z + (rt_gradient_noise((float)py, (float)px) * 2.0f - 1.0f) * sunJitter;
	*dir = rt_normalize(d);
}

// ---- the object-space ray of an instance: o' = rotateQuat(o - position, conj(q)) / scale, d' = rotateQuat(d, conj(q)) / scale (t is kept)

NV_RT rt3 rt_cross(rt3 a, rt3 b) { return rt3{ a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y }; }

// math.h:46-49 with cullmath.h's operation order: v + 2 cross(q, cross(q, v) + w v)
NV_RT rt3 rt_rotate_quat(rt3 v, rt3 q, float qw)
{
	rt3 t = rt_cross(q, v);
	t.x = t.x + qw * v.x;
	t.y = t.y + qw * v.y;
	t.z = t.z + qw * v.z;
	const rt3 u = rt_cross(q, t);
	return rt3{ v.x + 2.0f * u.x, v.y + 2.0f * u.y, v.z + 2.0f * u.z };
}

NV_RT void rt_object_ray(rt3 o, rt3 d, const float* position, const float* orientation, float scale, rt3* o2, rt3* d2)
{
	const rt3 c = { -orientation[0], -orientation[1], -orientation[2] };
	const rt3 rel = { o.x - position[0], o.y - position[1], o.z - position[2] };
	const rt3 ro = rt_rotate_quat(rel, c, orientation[3]), rd = rt_rotate_quat(d, c, orientation[3]);
	*o2 = rt3{ ro.x / scale, ro.y / scale, ro.z / scale };
	*d2 = rt3{ rd.x / scale, rd.y / scale, rd.z / scale };
}

// ---- the triangle test T (Woop, Benthin, Wald: Watertight Ray/Triangle Intersection, JCGT 2013)

NV_RT float rt_sel(float x, float y, float z, int k) { return k == 0 ? x : (k == 1 ? y : z); }

struct RtRay
{
	int kx, ky, kz;
	float ox, oy, oz; // the origin's kx, ky, kz components
	float Sx, Sy, Sz;
};

NV_RT RtRay rt_ray_setup(rt3 o, rt3 d)
{
	RtRay r;
	const float ax = __builtin_fabsf(d.x), ay = __builtin_fabsf(d.y), az = __builtin_fabsf(d.z);
	int kz = 0;
	float m = ax;
	if (ay > m)
	{
		kz = 1;
		m = ay;
	}
	if (az > m)
		kz = 2;
	int kx = kz == 2 ? 0 : kz + 1;
	int ky = kx == 2 ? 0 : kx + 1;
	const float dz = rt_sel(d.x, d.y, d.z, kz);
	if (dz < 0.0f)
	{
		const int s = kx;
		kx = ky;
		ky = s;
	}
	r.kx = kx, r.ky = ky, r.kz = kz;
	r.ox = rt_sel(o.x, o.y, o.z, kx), r.oy = rt_sel(o.x, o.y, o.z, ky), r.oz = rt_sel(o.x, o.y, o.z, kz);
	r.Sx = rt_sel(d.x, d.y, d.z, kx) / dz;
	r.Sy = rt_sel(d.x, d.y, d.z, ky) / dz;
	r.Sz = 1.0f / dz;
	return r;
}

NV_RT bool rt_triangle(const RtRay& r, rt3 v0, rt3 v1, rt3 v2, float tmin, float tmax)
{
	const float Akx = rt_sel(v0.x, v0.y, v0.z, r.kx) - r.ox, Aky = rt_sel(v0.x, v0.y, v0.z, r.ky) - r.oy, Akz = rt_sel(v0.x, v0.y, v0.z, r.kz) - r.oz;
	const float Bkx = rt_sel(v1.x, v1.y, v1.z, r.kx) - r.ox, Bky = rt_sel(v1.x, v1.y, v1.z, r.ky) - r.oy, Bkz = rt_sel(v1.x, v1.y, v1.z, r.kz) - r.oz;
	const float Ckx = rt_sel(v2.x, v2.y, v2.z, r.kx) - r.ox, Cky = rt_sel(v2.x, v2.y, v2.z, r.ky) - r.oy, Ckz = rt_sel(v2.x, v2.y, v2.z, r.kz) - r.oz;
	const float Ax = Akx - r.Sx * Akz, Ay = Aky - r.Sy * Akz;
	const float Bx = Bkx - r.Sx * Bkz, By = Bky - r.Sy * Bkz;
	const float Cx = Ckx - r.Sx * Ckz, Cy = Cky - r.Sy * Ckz;
	float U = Cx * By - Cy * Bx;
	float V = Ax * Cy - Ay * Cx;
	float W = Bx * Ay - By * Ax;
	if (U == 0.0f || V == 0.0f || W == 0.0f)
	{
		U = (float)((double)Cx * (double)By - (double)Cy * (double)Bx);
		V = (float)((double)Ax * (double)Cy - (double)Ay * (double)Cx);
		W = (float)((double)Bx * (double)Ay - (double)By * (double)Ax);
	}
	if ((U < 0.0f || V < 0.0f || W < 0.0f) && (U > 0.0f || V > 0.0f || W > 0.0f))
		return false;
	const float det = (U + V) + W;
	if (det == 0.0f)
		return false;
	const float T = (U * (r.Sz * Akz) + V * (r.Sz * Bkz)) + W * (r.Sz * Ckz);
	const float t = T / det;
	return t > tmin && t < tmax; // a NaN is a miss
}

// ---- the box test: slabs of the box widened by `pad`, NaN-safe; [tlo, thi] = the ray's range, already widened (or -inf, +inf)

struct RtSlab
{
	float ox, oy, oz, ix, iy, iz;
};

NV_RT RtSlab rt_slab_setup(rt3 o, rt3 d) { return RtSlab{ o.x, o.y, o.z, 1.0f / d.x, 1.0f / d.y, 1.0f / d.z }; }

NV_RT void rt_slab_axis(float lo, float hi, float pad, float o, float inv, float* tn, float* tf)
{
	float a = (lo - pad) - o, b = (hi + pad) - o;
	a = a == 0.0f ? -RT_TINY : a; // the origin on a slab plane is inside the slab, also with inv = +-inf (a zero direction component)
	b = b == 0.0f ? RT_TINY : b;
	const float t1 = a * inv, t2 = b * inv;
	*tn = __builtin_fminf(t1, t2); // fminf / fmaxf drop a NaN: no constraint from it
	*tf = __builtin_fmaxf(t1, t2);
}

NV_RT bool rt_box(const RtSlab& s, float pad, RtF4 lo, RtF4 hi, float tlo, float thi)
{
	float nx, fx, ny, fy, nz, fz;
	rt_slab_axis(lo.x, hi.x, pad, s.ox, s.ix, &nx, &fx);
	rt_slab_axis(lo.y, hi.y, pad, s.oy, s.iy, &ny, &fy);
	rt_slab_axis(lo.z, hi.z, pad, s.oz, s.iz, &nz, &fz);
	const float tn = __builtin_fmaxf(__builtin_fmaxf(nx, ny), nz), tf = __builtin_fminf(__builtin_fminf(fx, fy), fz);
	return !(tn > tf) && !(tn > thi) && !(tf < tlo); // written so that a NaN keeps the node
}

// ---- the traversal: depth-first preorder with skip links on both levels; the visited index strictly increases, no stack.
// maxPostPass = quality: instances with postPass above it do not cast.  The blob has passed nv_rt_scene_validate.
NV_RT bool rt_occluded(const unsigned char* blob, rt3 o, rt3 d, float tmin, float tmax, uint32_t maxPostPass)
{
	if (!(rt_finite(o.x) && rt_finite(o.y) && rt_finite(o.z) && rt_finite(d.x) && rt_finite(d.y) && rt_finite(d.z)))
		return false;
	const RtHeader* h = reinterpret_cast<const RtHeader*>(blob);
	const RtF4* tlas = reinterpret_cast<const RtF4*>(blob + h->tlasOff);
	const RtF4* inst = reinterpret_cast<const RtF4*>(blob + h->instOff);
	const RtF4* table = reinterpret_cast<const RtF4*>(blob + h->tableOff);
	const RtF4* blasNodes = reinterpret_cast<const RtF4*>(blob + h->blasOff);
	const RtF4* tris = reinterpret_cast<const RtF4*>(blob + h->triOff);
	const uint32_t tlasCount = h->tlasNodes;
	const float inf = __builtin_inff();
	const RtSlab sw = rt_slab_setup(o, d);
	const float padW = h->padOrigin * rt_max3abs(o);
	for (uint32_t i = 0; i < tlasCount;)
	{
		const RtF4 lo = tlas[2u * i], hi = tlas[2u * i + 1u];
		const uint32_t skip = rt_bits(lo.w), leaf = rt_bits(hi.w);
		if (!rt_box(sw, padW, lo, hi, -inf, inf)) // the line, not the segment: see DESIGN.md §4.16
		{
			i = skip;
			continue;
		}
		if (leaf == 0u)
		{
			++i;
			continue;
		}
		i = skip;
		const uint32_t at = (leaf & RT_LEAF_FIRST) * 4u;
		const RtF4 i0 = inst[at], i1 = inst[at + 1u], i2 = inst[at + 2u];
		if (rt_bits(i2.y) > maxPostPass)
			continue;
		const float position[3] = { i0.x, i0.y, i0.z }, orientation[4] = { i1.x, i1.y, i1.z, i1.w };
		rt3 o2, d2;
		rt_object_ray(o, d, position, orientation, i0.w, &o2, &d2);
		const RtRay ray = rt_ray_setup(o2, d2);
		const RtF4 b0 = table[2u * rt_bits(i2.z)], b1 = table[2u * rt_bits(i2.z) + 1u];
		const uint32_t nodeFirst = rt_bits(b0.x), nodeCount = rt_bits(b0.y), triFirst = rt_bits(b0.z);
		// the margins of this (ray, instance): eps widens every box, tau widens the ray's range; where they are not finite nothing is culled
		const float eps = RT_PAD_K * RT_U * (rt_max3abs(o2) + b1.x);
		const float tau = ((b1.y + 2.0f * eps) / rt_max3abs(d2)) * RT_T_UP;
		const bool cull = eps < inf && tau < inf; // false on NaN
		const float tlo = tmin - tau, thi = tmax + tau;
		const RtSlab so = rt_slab_setup(o2, d2);
		const RtF4* nodes = blasNodes + 2u * (size_t)nodeFirst;
		const RtF4* tri = tris + 3u * (size_t)triFirst;
		for (uint32_t j = 0; j < nodeCount;)
		{
			const RtF4 nlo = nodes[2u * j], nhi = nodes[2u * j + 1u];
			const uint32_t nskip = rt_bits(nlo.w), nleaf = rt_bits(nhi.w);
			if (cull && !rt_box(so, eps, nlo, nhi, tlo, thi))
			{
				j = nskip;
				continue;
			}
			if (nleaf == 0u)
			{
				++j;
				continue;
			}
			j = nskip;
			const uint32_t first = nleaf & RT_LEAF_FIRST, count = nleaf >> RT_LEAF_SHIFT;
			for (uint32_t k = 0; k < count; ++k)
			{
				const RtF4 v0 = tri[3u * (first + k)], v1 = tri[3u * (first + k) + 1u], v2 = tri[3u * (first + k) + 2u];
				if (rt_triangle(ray, rt3{ v0.x, v0.y, v0.z }, rt3{ v1.x, v1.y, v1.z }, rt3{ v2.x, v2.y, v2.z }, tmin, tmax))
					return true;
			}
		}
	}
	return false;
}

} // namespace nv
