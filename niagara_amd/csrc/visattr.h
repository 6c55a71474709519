// visattr.h — the attribute pass of the visibility buffer as ONE text for its entry points: visattr.hip
// instantiates visibility_attributes_kernel<RUNS> (nv_visibility_attributes: the fragment stage from the material's factors) and
// visattr_tex.hip and visattr_blocks.hip visibility_attributes_kernel<true, true, VisAttrSetArgs<SET>> (nv_visibility_attributes_textured,
// nv_visibility_attributes_blocks: the complete fragment stage over a texture set of residency SET, texmath.h's TxDecoded or TxBlocks, §4.21);
// the argument structs are args.h's.  Run detection, set-up, barycentrics and varyings are shared; TEX only adds statements under
// `if constexpr (TEX)`, so the untextured kernels keep their instruction streams.
#pragma once
#include "raster.h"
#include "launch.h"
#include "fragalpha.h" // the corner's clip x, y, w and uv, the barycentrics, the texture read: shared with the alpha-tested raster (§4.20)

namespace nv
{

constexpr int VA_THREADS = 256;

// one corner of the triangle after the vertex stage: fragalpha.h's clip x, y, w and packed uv, plus what the other varyings need
struct VaCorner : FaCorner
{
	f3 n;             // rotateQuat(normal)
	f3 t;             // rotateQuat(tangent.xyz)
	float tw;         // tangent.w
	f3 w;             // wpos
};

struct VaSetup
{
	VaCorner a, b, c;
	uint32_t ok;            // 0: the record is invalid
	uint32_t materialIndex; // draw.materialIndex
};

// normalize(v) = v / sqrt((x x + y y) + z z) per component
NV_DEV f3 va_normalize(f3 v)
{
	const float l = __builtin_sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z);
	return f3{ v.x / l, v.y / l, v.z / l };
}

// math.h:60-67
NV_DEV f3 va_decode_oct(float ex, float ey)
{
	f3 v = { ex, ey, (1.0f - __builtin_fabsf(ex)) - __builtin_fabsf(ey) };
	const float t = gl_max(-v.z, 0.0f);
	v.x = v.x + (v.x >= 0.0f ? -t : t);
	v.y = v.y + (v.y >= 0.0f ? -t : t);
	return va_normalize(v);
}

// meshlet.mesh.glsl:129-140 for one vertex record under the draw {d0 = position.xyz, scale; d1 = orientation}
NV_DEV VaCorner va_vertex(const NvGlobals& g, uint4 v, float4 d0, float4 d1)
{
	VaCorner o;
	const f3 q = { d1.x, d1.y, d1.z };
	// math.h:104-109 unpackTBN
	const f3 normal = { (float)(int32_t)(v.z & 1023u) / 511.0f - 1.0f, (float)(int32_t)(v.z >> 10 & 1023u) / 511.0f - 1.0f,
		                (float)(int32_t)(v.z >> 20 & 1023u) / 511.0f - 1.0f };
	const uint32_t tp = v.y >> 16;
	const f3 tangent = va_decode_oct((float)(int32_t)(tp & 255u) / 127.0f - 1.0f, (float)(int32_t)(tp >> 8 & 255u) / 127.0f - 1.0f);
	o.tw = (v.z & (1u << 30)) != 0u ? -1.0f : 1.0f;
	o.n = rotate_quat(normal, q, d1.w);
	o.t = rotate_quat(tangent, q, d1.w);
	o.uv = v.w;
	// wpos: the statements rd_clip_position starts with (the compiler evaluates them once)
	const f3 position = { half_bits_to_float(v.x & 0xffffu), half_bits_to_float(v.x >> 16), half_bits_to_float(v.y & 0xffffu) };
	const f3 rot = rotate_quat(position, q, d1.w);
	o.w = f3{ rot.x * d0.w + d0.x, rot.y * d0.w + d0.y, rot.z * d0.w + d0.z };
	float clip[4];
	rd_clip_position(g, make_uint2(v.x, v.y), q, d1.w, d0.w, d0.x, d0.y, d0.z, clip);
	o.cx = clip[0], o.cy = clip[1], o.cw = clip[3];
	return o;
}

// The validation and the set-up of the triangle a record names (drawId != ~0).  Every load is behind the check that keeps it inside the
// caller's buffers; s.ok = 0 when a check fails (the corners then are left as they are: nothing reads them).
NV_DEV void va_setup(const VisAttrArgs& a, uint4 r, VaSetup& s)
{
	s.ok = 0u;
	if (r.x >= a.drawCount || r.y >= a.meshletCount)
		return;
	const uint32_t* mw = reinterpret_cast<const uint32_t*>(a.meshlets + r.y);
	const uint32_t dataOffset = mw[3], baseVertex = mw[4], counts = mw[5];
	const uint32_t vcRaw = counts & 0xffu, tcRaw = counts >> 8 & 0xffu;
	const bool shortRefs = (counts >> 16 & 0xffu) == 1u;
	const uint32_t ve = vcRaw < 64u ? vcRaw : 64u, te = tcRaw < 96u ? tcRaw : 96u;
	if (r.z >= te)
		return;
	// meshlet.mesh.glsl:116,170 in 64 bits: nothing wraps
	const unsigned long long indexOffset = (unsigned long long)dataOffset + (shortRefs ? (vcRaw + 1u) / 2u : vcRaw);
	const unsigned long long o = indexOffset * 4ull + r.z * 3u;
	const unsigned long long dataBytes = (unsigned long long)a.dataWords * 4ull;
	if (o + 3ull > dataBytes)
		return;
	const uint8_t* data8 = reinterpret_cast<const uint8_t*>(a.meshletData);
	const uint32_t ia = data8[o], ib = data8[o + 1], ic = data8[o + 2];
	if (ia >= ve || ib >= ve || ic >= ve)
		return;
	// meshlet.mesh.glsl:127: the three vertex references (ia, ib, ic < 64: the last one read is the largest position)
	const uint32_t im = ia > ib ? (ia > ic ? ia : ic) : (ib > ic ? ib : ic);
	const unsigned long long last = shortRefs ? ((unsigned long long)dataOffset * 2ull + im) * 2ull + 2ull : ((unsigned long long)dataOffset + im) * 4ull + 4ull;
	if (last > dataBytes)
		return;
	const uint16_t* data16 = reinterpret_cast<const uint16_t*>(a.meshletData);
	const unsigned long long ra = shortRefs ? data16[(unsigned long long)dataOffset * 2ull + ia] : a.meshletData[(unsigned long long)dataOffset + ia];
	const unsigned long long rb = shortRefs ? data16[(unsigned long long)dataOffset * 2ull + ib] : a.meshletData[(unsigned long long)dataOffset + ib];
	const unsigned long long rc = shortRefs ? data16[(unsigned long long)dataOffset * 2ull + ic] : a.meshletData[(unsigned long long)dataOffset + ic];
	const unsigned long long va = ra + baseVertex, vb = rb + baseVertex, vc = rc + baseVertex;
	if (va >= a.vertexCount || vb >= a.vertexCount || vc >= a.vertexCount)
		return;
	const float4* dp = reinterpret_cast<const float4*>(a.draws + r.x);
	const float4 d0 = dp[0], d1 = dp[1];
	const uint32_t materialIndex = reinterpret_cast<const uint32_t*>(dp + 2)[3];
	if (a.materials && materialIndex >= a.materialCount)
		return;
	const uint4* vp = reinterpret_cast<const uint4*>(a.vertices);
	const uint4 v0 = vp[va], v1 = vp[vb], v2 = vp[vc];
	s.a = va_vertex(a.globals, v0, d0, d1);
	s.b = va_vertex(a.globals, v1, d0, d1);
	s.c = va_vertex(a.globals, v2, d0, d1);
	s.materialIndex = materialIndex;
	s.ok = 1u;
}

NV_DEV uint32_t va_from(uint32_t v, uint32_t lane) { return (uint32_t)__shfl((int)v, (int)lane, 64); }
NV_DEV float va_from(float v, uint32_t lane) { return __uint_as_float(va_from(__float_as_uint(v), lane)); }
NV_DEV f3 va_from(f3 v, uint32_t lane) { return f3{ va_from(v.x, lane), va_from(v.y, lane), va_from(v.z, lane) }; }
NV_DEV void va_from(VaCorner& c, uint32_t lane)
{
	c.cx = va_from(c.cx, lane), c.cy = va_from(c.cy, lane), c.cw = va_from(c.cw, lane);
	c.uv = va_from(c.uv, lane);
	c.n = va_from(c.n, lane), c.t = va_from(c.t, lane), c.tw = va_from(c.tw, lane), c.w = va_from(c.w, lane);
}

NV_DEV float va_fract(float x) { return x - __builtin_floorf(x); }

// UNORM pack of one channel: clamp to [0, 1] with NaN -> 0, scale, round half to even
NV_DEV uint32_t va_unorm(float x, float scale)
{
	float v = x > 0.0f ? x : 0.0f;
	v = v < 1.0f ? v : 1.0f;
	return (uint32_t)__builtin_rintf(v * scale);
}

// ARGS = VisAttrArgs (TEX = false) or VisAttrSetArgs<SET> (TEX = true)
template <bool RUNS, bool TEX = false, typename ARGS = VisAttrArgs>
__global__ __launch_bounds__(VA_THREADS) void visibility_attributes_kernel(ARGS a)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t stride = gridDim.x * VA_THREADS;
	uint32_t shaded = 0, invalid = 0, degenerate = 0, textured = 0; // per lane

	// `base` is the wave's first pixel: the loop is uniform over the wave, so the DPP moves, the ballot and the permutes see all 64 lanes
	for (uint32_t base = blockIdx.x * VA_THREADS + wave * 64u; base < a.n; base += stride)
	{
		const uint32_t i = base + lane;
		const bool in = i < a.n;
		const va_u4 word = __builtin_nontemporal_load(a.records + (in ? i : base));
		const uint4 r = make_uint4(in ? word.x : ~0u, word.y, word.z, word.w);
		const bool named = r.x != ~0u;

		VaSetup s;
		s.ok = 0u, s.materialIndex = 0u;
		s.a = VaCorner{ FaCorner{ 0.0f, 0.0f, 0.0f, 0u }, f3{ 0.0f, 0.0f, 0.0f }, f3{ 0.0f, 0.0f, 0.0f }, 0.0f, f3{ 0.0f, 0.0f, 0.0f } };
		s.b = s.a, s.c = s.a;
		if (RUNS)
		{
			// (the moves are statements of their own: see visresolve.hip)
			const uint32_t p0 = wave_shift_up1_u32(r.x), p1 = wave_shift_up1_u32(r.y), p2 = wave_shift_up1_u32(r.z);
			const bool start = lane == 0u || p0 != r.x || p1 != r.y || p2 != r.z;
			const uint64_t starts = __ballot(start);
			if (start && named)
				va_setup(a, r, s);
			// the start of this lane's run: the highest starting lane at or below it (lane 0 always starts one)
			const uint32_t from = 63u - (uint32_t)__builtin_clzll(starts & (~0ull >> (63u - lane)));
			va_from(s.a, from), va_from(s.b, from), va_from(s.c, from);
			s.ok = va_from(s.ok, from), s.materialIndex = va_from(s.materialIndex, from);
		}
		else if (named)
			va_setup(a, r, s);

		const bool ok = named && s.ok != 0u;
		invalid += named && !ok ? 1u : 0u;
		shaded += ok ? 1u : 0u;
		uint4 o0 = make_uint4(0u, 0u, 0u, 0u), o1 = make_uint4(0u, 0u, 0u, ~0u), o2 = o0, o3 = o0;
		uint32_t g0 = 0u, g1 = 0u;
		if (ok)
		{
			// ---- homogeneous barycentrics at the pixel centre (row 0 at the top)
			const uint32_t py = i / a.width, px = i - py * a.width;
			const float fx = (float)px + 0.5f, fy = (float)py + 0.5f;
			// (written out, not fa_bary(): through the function the compiler orders the untextured kernels' instructions differently, and they keep theirs)
			const float nx = (fx / a.fw) * 2.0f - 1.0f, ny = 1.0f - (fy / a.fh) * 2.0f;
			const float d0x = s.a.cx - nx * s.a.cw, d0y = s.a.cy - ny * s.a.cw;
			const float d1x = s.b.cx - nx * s.b.cw, d1y = s.b.cy - ny * s.b.cw;
			const float d2x = s.c.cx - nx * s.c.cw, d2y = s.c.cy - ny * s.c.cw;
			const float b0 = d1x * d2y - d1y * d2x, b1 = d2x * d0y - d2y * d0x, b2 = d0x * d1y - d0y * d1x;
			const float sum = (b0 + b1) + b2;
			float l0 = b0 / sum, l1 = b1 / sum, l2 = b2 / sum;
			const bool degen = sum == 0.0f || !va_finite(l0) || !va_finite(l1) || !va_finite(l2);
			l0 = degen ? 1.0f : l0, l1 = degen ? 0.0f : l1, l2 = degen ? 0.0f : l2;
			degenerate += degen ? 1u : 0u;

			// ---- the varyings
			const float u = va_mix(l0, l1, l2, half_bits_to_float(s.a.uv & 0xffffu), half_bits_to_float(s.b.uv & 0xffffu), half_bits_to_float(s.c.uv & 0xffffu));
			const float v = va_mix(l0, l1, l2, half_bits_to_float(s.a.uv >> 16), half_bits_to_float(s.b.uv >> 16), half_bits_to_float(s.c.uv >> 16));
			const f3 n = { va_mix(l0, l1, l2, s.a.n.x, s.b.n.x, s.c.n.x), va_mix(l0, l1, l2, s.a.n.y, s.b.n.y, s.c.n.y), va_mix(l0, l1, l2, s.a.n.z, s.b.n.z, s.c.n.z) };
			const f3 t = { va_mix(l0, l1, l2, s.a.t.x, s.b.t.x, s.c.t.x), va_mix(l0, l1, l2, s.a.t.y, s.b.t.y, s.c.t.y), va_mix(l0, l1, l2, s.a.t.z, s.b.t.z, s.c.t.z) };
			const float tw = va_mix(l0, l1, l2, s.a.tw, s.b.tw, s.c.tw);
			const f3 w = { va_mix(l0, l1, l2, s.a.w.x, s.b.w.x, s.c.w.x), va_mix(l0, l1, l2, s.a.w.y, s.b.w.y, s.c.w.y), va_mix(l0, l1, l2, s.a.w.z, s.b.w.z, s.c.w.z) };
			o0 = make_uint4(__float_as_uint(u), __float_as_uint(v), __float_as_uint(l1), __float_as_uint(l2));
			o1 = make_uint4(__float_as_uint(n.x), __float_as_uint(n.y), __float_as_uint(n.z), r.x);
			o2 = make_uint4(__float_as_uint(t.x), __float_as_uint(t.y), __float_as_uint(t.z), __float_as_uint(tw));
			o3 = make_uint4(__float_as_uint(w.x), __float_as_uint(w.y), __float_as_uint(w.z), s.materialIndex);

			// ---- the fragment stage, mesh.frag.glsl:57-89 (TEX: with the texture terms, §4.18)
			if (a.materials)
			{
				const uint4* mp = reinterpret_cast<const uint4*>(a.materials + s.materialIndex);
				const uint4 tex = mp[0];
				const float4 diffuse = *reinterpret_cast<const float4*>(mp + 1), specular = *reinterpret_cast<const float4*>(mp + 2);
				const float4 emissive = *reinterpret_cast<const float4*>(mp + 3); // .w: padding
				float4 albedo = diffuse;
				f3 nmap = { 0.0f, 0.0f, 1.0f }, em = { emissive.x, emissive.y, emissive.z };
				float gloss = specular.w; // specgloss.a: all that reaches the G-buffer of it
				if constexpr (TEX)
				{
					// ---- uv's derivatives per pixel step: the same set-up at the centres of (px + 1, py) and (px, py + 1); nothing is loaded there
					float dudx, dvdx, dudy, dvdy;
					fa_uv_steps(s.a, s.b, s.c, px, py, fx, fy, a.fw, a.fh, u, v, dudx, dvdx, dudy, dvdy);
					// :62-76, one texture after the other (8 taps each): the taps of one are consumed before the next one's are issued
					bool missing = false;
					TxF4 c;
					if (tex.x != 0u)
					{
						if (ARGS::Set::texture(a.tx, tex.x, u, v, dudx, dvdx, dudy, dvdy, c))
							albedo = make_float4(albedo.x * __builtin_powf(c.x, 2.2f), albedo.y * __builtin_powf(c.y, 2.2f), albedo.z * __builtin_powf(c.z, 2.2f), fa_alpha(albedo.w, c.w));
						else
							missing = true;
					}
					if (tex.y != 0u)
					{
						if (ARGS::Set::texture(a.tx, tex.y, u, v, dudx, dvdx, dudy, dvdy, c))
							nmap = f3{ c.x * 2.0f - 1.0f, c.y * 2.0f - 1.0f, c.z * 2.0f - 1.0f };
						else
							missing = true;
					}
					if (tex.z != 0u)
					{
						if (ARGS::Set::texture(a.tx, tex.z, u, v, dudx, dvdx, dudy, dvdy, c))
							gloss = gloss * c.w; // fromsrgb(vec4) leaves .a as it is
						else
							missing = true;
					}
					if (tex.w != 0u)
					{
						if (ARGS::Set::texture(a.tx, tex.w, u, v, dudx, dvdx, dudy, dvdy, c))
							em = f3{ em.x * __builtin_powf(c.x, 2.2f), em.y * __builtin_powf(c.y, 2.2f), em.z * __builtin_powf(c.z, 2.2f) };
						else
							missing = true;
					}
					textured += missing ? 1u : 0u;
				}
				else
					textured += (tex.x | tex.y | tex.z | tex.w) != 0u ? 1u : 0u;
				// math.h:99-102 gradientNoise(gl_FragCoord.xy)
				const float noise = va_fract(52.9829189f * va_fract(fx * 0.06711056f + fy * 0.00583715f));
				const float deband = noise * 2.0f - 1.0f;
				// :78-80; without a normal map nmap = (0, 0, 1), the multiplications by zero included
				const f3 bt = cross3(n, t);
				const f3 bitangent = { bt.x * tw, bt.y * tw, bt.z * tw };
				const f3 nrm = va_normalize(f3{ (nmap.x * t.x + nmap.y * bitangent.x) + nmap.z * n.x, (nmap.x * t.y + nmap.y * bitangent.y) + nmap.z * n.y,
					                            (nmap.x * t.z + nmap.y * bitangent.z) + nmap.z * n.z });
				// :82
				const float emissivef = ((em.x * 0.3f + em.y * 0.6f) + em.z * 0.1f) / (((albedo.x * 0.3f + albedo.y * 0.6f) + albedo.z * 0.1f) + 1e-3f);
				// :85 tosrgb (math.h:74-77) and log2: the two functions that are not correctly rounded
				const float gamma = 1.0f / 2.2f;
				const float c0 = __builtin_powf(albedo.x, gamma), c1 = __builtin_powf(albedo.y, gamma), c2 = __builtin_powf(albedo.z, gamma);
				const float c3 = __builtin_log2f(1.0f + emissivef) / 5.0f;
				g0 = va_unorm(c0, 255.0f) | va_unorm(c1, 255.0f) << 8 | va_unorm(c2, 255.0f) << 16 | va_unorm(c3, 255.0f) << 24;
				// :86 encodeOct (math.h:52-58)
				const float inv = 1.0f / ((__builtin_fabsf(nrm.x) + __builtin_fabsf(nrm.y)) + __builtin_fabsf(nrm.z));
				const float ox = nrm.x * inv, oy = nrm.y * inv;
				const float sx = nrm.x >= 0.0f ? 1.0f : -1.0f, sy = nrm.y >= 0.0f ? 1.0f : -1.0f;
				const float ex = nrm.z <= 0.0f ? (1.0f - __builtin_fabsf(oy)) * sx : ox;
				const float ey = nrm.z <= 0.0f ? (1.0f - __builtin_fabsf(ox)) * sy : oy;
				const float band = deband * (0.5f / 1023.0f);
				const float e0 = (ex * 0.5f + 0.5f) + band, e1 = (ey * 0.5f + 0.5f) + band;
				g1 = va_unorm(e0, 1023.0f) | va_unorm(e1, 1023.0f) << 10 | va_unorm(gloss, 1023.0f) << 20 | va_unorm(0.0f, 3.0f) << 30;
			}
		}
		if (in)
		{
			if (a.attributes)
			{
				uint4* out = a.attributes + (size_t)i * 4u;
				out[0] = o0, out[1] = o1, out[2] = o2, out[3] = o3;
			}
			if (a.gbuffer0)
				a.gbuffer0[i] = g0;
			if (a.gbuffer1)
				a.gbuffer1[i] = g1;
		}
	}

	if (!a.totals)
		return;
	__shared__ uint32_t s_tot[VA_THREADS / 64][4];
	const uint32_t w0 = wave_sum_u32(shaded), w1 = wave_sum_u32(invalid), w2 = wave_sum_u32(degenerate), w3 = wave_sum_u32(textured);
	if (lane == 0u)
	{
		s_tot[wave][0] = w0;
		s_tot[wave][1] = w1;
		s_tot[wave][2] = w2;
		s_tot[wave][3] = w3;
	}
	__syncthreads();
	if (threadIdx.x < 4u)
	{
		unsigned long long t = 0;
#pragma unroll
		for (int k = 0; k < VA_THREADS / 64; ++k)
			t += s_tot[k][threadIdx.x];
		if (t)
			atomicAdd(a.totals + threadIdx.x, t);
	}
}

// the fields every launcher derives from the image size, and their grid
inline uint32_t va_complete(VisAttrArgs& a, uint32_t height, uint32_t maxBlocks)
{
	a.n = a.width * height;
	a.fw = (float)a.width;
	a.fh = (float)height;
	return capped_grid(a.n, VA_THREADS, maxBlocks);
}

// the launch of the textured pass over either residency of the set
template <typename ARGS>
int launch_visibility_attributes_set(hipStream_t stream, ARGS a, uint32_t height, uint32_t maxBlocks)
{
	const uint32_t grid = va_complete(a, height, maxBlocks);
	hipLaunchKernelGGL((visibility_attributes_kernel<true, true, ARGS>), dim3(grid), dim3(VA_THREADS), 0, stream, a);
	return (int)hipGetLastError();
}

} // namespace nv
