// rtalpha.h — the alpha-tested traversal of the ray-traced shadow pass in ONE place that compiles for the device (hipcc) and
// for the host (g++): shadowTraceTransparent of shadow.comp.glsl:86-123.  The triangle test that hands back its U, V, W and det, the albedo
// texture of an instance, and rt_occluded_alpha, rtmath.h's rt_occluded with the confirming loop.  The texture set is asked through its residency
// type (texmath.h: TxDecoded or TxBlocks, RtAlphaInputs<SET>::Set), whose alpha_lod0 holds the four alpha taps of textureLod(..., 0).w.
// shadowtrace_alpha.hip's kernels and nv_rt_scene_trace_host_textured_rays run the same text; tests/shadow_alpha_ref.c restates it without a BVH.
//
// Build with -ffp-contract=off.  rtmath.h's rt_triangle and rt_occluded are not touched: nv_shadow_trace's kernels keep their code.
#pragma once

#include "../../include/niagara_vis.h"
#include "rtmath.h"
#ifndef NV_TX_SAMPLER_ONLY
#define NV_TX_SAMPLER_ONLY // the sampler half of texmath.h: no decode tables in this translation unit
#endif
#include "texmath.h"

namespace nv
{

// the fp16 of the low 16 bits, exact (rtbuild.cpp's half_to_float)
NV_RT float rt_half(uint32_t h)
{
	const uint32_t s = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 1023u;
	if (e == 0u)
	{
		const float v = (float)m * 5.9604644775390625e-8f;
		return s ? -v : v;
	}
	const uint32_t bits = s | (e == 31u ? 0x7f800000u | m << 13 : (e + 112u) << 23 | m << 13);
	float v;
	__builtin_memcpy(&v, &bits, 4);
	return v;
}

// T (rtmath.h rt_triangle, the same operations in the same order) that also hands back U, V, W — after the fp64 fallback where T took it —
// and det of an accepted triangle
struct RtHit
{
	float U, V, W, det;
};

NV_RT bool rt_triangle_uvw(const RtRay& r, rt3 v0, rt3 v1, rt3 v2, float tmin, float tmax, RtHit* hit)
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
	hit->U = U, hit->V = V, hit->W = W, hit->det = det;
	return t > tmin && t < tmax; // a NaN is a miss
}

// The albedo texture the alpha test of draw `drawId` samples (shadow.comp.glsl:108-117): false = alpha is 1.  A draw, material or texture
// index out of range, texture 0 (:116) and a descriptor the set refuses (SET::ok: its chain does not lie inside the set's buffer) are all
// "no texture": nothing is loaded through an index that was not checked.
template <typename SET>
NV_RT bool rt_albedo_desc(const RtAlphaInputs<SET>& in, uint32_t drawId, typename SET::Desc* desc)
{
	if (drawId >= in.drawCount)
		return false;
	const uint32_t material = in.draws[drawId].materialIndex;
	if (material >= in.materialCount)
		return false;
	const uint32_t tex = in.materials[material].albedoTexture;
	if (tex == 0u || tex >= in.textureCount)
		return false;
	*desc = in.textures[tex];
	return SET::ok(*desc, in.extent);
}

// uv of an accepted triangle at the hit (shadow.comp.glsl:110-116); w0, w1, w2: the corners' packed texcoord bits tu | tv << 16
struct RtUv
{
	float u, v;
};
NV_RT RtUv rt_hit_uv(const RtHit& hit, uint32_t w0, uint32_t w1, uint32_t w2)
{
	const float b1 = hit.V / hit.det, b2 = hit.W / hit.det;
	const float b0 = (1.0f - b1) - b2;
	const float u = (rt_half(w0 & 0xffffu) * b0 + rt_half(w1 & 0xffffu) * b1) + rt_half(w2 & 0xffffu) * b2;
	const float v = (rt_half(w0 >> 16) * b0 + rt_half(w1 >> 16) * b1) + rt_half(w2 >> 16) * b2;
	return RtUv{ u, v };
}

// rt_occluded(..., 1) whose hits are CONFIRMED: a triangle of a postPass == 0 instance always (FORCE_OPAQUE, src/scenert.cpp:516), one of a
// postPass == 1 instance when its alpha is >= 0.5 (a NaN does not confirm).  The instance's texture is resolved once, where its BLAS is
// entered; an instance without one confirms unconditionally and leaves at its first accepted triangle, as rt_occluded does.  The result is an OR
// over the accepted triangles: it does not depend on the order of the walk.  The blob has passed nv_rt_scene_validate and carries
// RT_FLAG_TEXCOORDS.  One text for both residencies of the texture set.
template <typename SET>
NV_RT bool rt_occluded_alpha(const unsigned char* blob, const RtAlphaInputs<SET>& in, rt3 o, rt3 d, float tmin, float tmax)
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
		if (!rt_box(sw, padW, lo, hi, -inf, inf))
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
		const uint32_t postPass = rt_bits(i2.y);
		if (postPass > 1u)
			continue;
		typename SET::Desc tex = SET::none();
		const bool tested = postPass == 1u && rt_albedo_desc(in, rt_bits(i2.x), &tex);
		const float position[3] = { i0.x, i0.y, i0.z }, orientation[4] = { i1.x, i1.y, i1.z, i1.w };
		rt3 o2, d2;
		rt_object_ray(o, d, position, orientation, i0.w, &o2, &d2);
		const RtRay ray = rt_ray_setup(o2, d2);
		const RtF4 b0 = table[2u * rt_bits(i2.z)], b1 = table[2u * rt_bits(i2.z) + 1u];
		const uint32_t nodeFirst = rt_bits(b0.x), nodeCount = rt_bits(b0.y), triFirst = rt_bits(b0.z);
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
				RtHit hit;
				if (!rt_triangle_uvw(ray, rt3{ v0.x, v0.y, v0.z }, rt3{ v1.x, v1.y, v1.z }, rt3{ v2.x, v2.y, v2.z }, tmin, tmax, &hit))
					continue;
				if (!tested)
					return true;
				const RtUv at = rt_hit_uv(hit, rt_bits(v0.w), rt_bits(v1.w), rt_bits(v2.w));
				if (SET::alpha_lod0(in.data, tex, at.u, at.v) >= 0.5f) // :117-118; a NaN does not confirm
					return true;
			}
		}
	}
	return false;
}

} // namespace nv
