/*
 * glsl_shade_shim.h — what the reference's SHADING shaders need beyond glsl_shim.h (TEST INFRASTRUCTURE).  Included by glsl_shim.h when a
 * translation unit is built with -DREF_SHADING (shadowfill, shadowblur, final, bloom, mesh.frag; oracle/Makefile), in place of the cull
 * shaders' single-channel images and MIN sampler.
 *
 * As there, only what GLSL and Vulkan leave to the implementation lives here, and every such piece follows the rule DESIGN.md documents for
 * it (the paragraph is named at the spot).  Everything else is component-wise fp32, one IEEE operation per operator, left to right.
 */
#pragma once

namespace glsl
{
/* Everything below has internal linkage: these names (texture2D, image2D, texture(), ...) mean something else in the cull translation
 * units of the same library, and the counters are per translation unit. */
namespace
{
using glsl::abs;
using glsl::dot;
using glsl::exp2;
using glsl::log2;
using glsl::max;
using glsl::min;

/* ---- integer vectors (shadowblur.comp.glsl:34-46, math.h:106-107): component-wise int32 arithmetic; GLSL's is C++'s */
struct ivec3
{
	int x, y, z;
	ivec3(int x_, int y_, int z_) : x(x_), y(y_), z(z_) {}
	explicit ivec3(int s) : x(s), y(s), z(s) {}
	explicit ivec3(uint s) : x((int)s), y((int)s), z((int)s) {}
};
inline ivec2 operator+(ivec2 a, ivec2 b) { return ivec2(a.x + b.x, a.y + b.y); }
inline ivec2 operator-(ivec2 a) { return ivec2(-a.x, -a.y); }
inline ivec2 operator&(ivec2 a, ivec2 b) { return ivec2(a.x & b.x, a.y & b.y); }
inline ivec2 operator>>(ivec2 a, ivec2 b) { return ivec2(a.x >> b.x, a.y >> b.y); }
inline ivec3 operator&(ivec3 a, ivec3 b) { return ivec3(a.x & b.x, a.y & b.y, a.z & b.z); }
inline ivec3 operator>>(ivec3 a, ivec3 b) { return ivec3(a.x >> b.x, a.y >> b.y, a.z >> b.z); }
/* int op float: the integer operand converts to float first (GLSL 4.60 §4.1.10), then one fp32 division per component */
inline vec2 operator/(ivec2 a, float s) { return vec2((float)a.x / s, (float)a.y / s); }
inline vec3 operator/(ivec3 a, float s) { return vec3((float)a.x / s, (float)a.y / s, (float)a.z / s); }

/* ---- float vectors: the operators the shading shaders use, component-wise */
inline vec2 operator+(vec2 a, float s) { return vec2(a.x + s, a.y + s); }
inline vec2 operator-(vec2 a, float s) { return vec2(a.x - s, a.y - s); }
inline vec2 operator-(float s, vec2 a) { return vec2(s - a.x, s - a.y); }
inline vec2 operator/(float s, vec2 a) { return vec2(s / a.x, s / a.y); }

inline vec3 operator+(vec3 a, float s) { return vec3(a.x + s, a.y + s, a.z + s); }
inline vec3 operator-(vec3 a, float s) { return vec3(a.x - s, a.y - s, a.z - s); }
inline vec3 operator*(vec3 a, vec3 b) { return vec3(a.x * b.x, a.y * b.y, a.z * b.z); }
inline vec3 operator/(vec3 a, vec3 b) { return vec3(a.x / b.x, a.y / b.y, a.z / b.z); }
inline vec3 operator/(vec3 a, float s) { return vec3(a.x / s, a.y / s, a.z / s); }
inline vec3& operator+=(vec3& a, float s)
{
	a.x += s, a.y += s, a.z += s;
	return a;
}
inline vec3& operator*=(vec3& a, vec3 b)
{
	a.x *= b.x, a.y *= b.y, a.z *= b.z;
	return a;
}

inline vec4 operator-(vec4 a) { return vec4(-a.x, -a.y, -a.z, -a.w); }
inline vec4 operator-(vec4 a, float s) { return vec4(a.x - s, a.y - s, a.z - s, a.w - s); }
inline vec4& operator*=(vec4& a, vec4 b)
{
	a.x *= b.x, a.y *= b.y, a.z *= b.z, a.w *= b.w;
	return a;
}

/* the lvalue swizzles: `v.xy += ...` (math.h:65) and `tangent.xyz = ...` (math.h:107), rewritten by the translator to lv_xy(v) / lv_xyz(v) */
struct xy_lvalue
{
	float &x, &y;
	void operator+=(vec2 b) { x += b.x, y += b.y; }
};
struct xyz_lvalue
{
	float &x, &y, &z;
	void operator=(vec3 b) { x = b.x, y = b.y, z = b.z; }
};
inline xy_lvalue lv_xy(vec3& v) { return xy_lvalue{ v.x, v.y }; }
inline xyz_lvalue lv_xyz(vec4& v) { return xyz_lvalue{ v.x, v.y, v.z }; }

/* ---- built-ins on vectors: component-wise; pow / exp2 / log2 are libm's fp32 functions */
inline float pow(float x, float y) { return powf(x, y); }
inline vec3 pow(vec3 a, vec3 b) { return vec3(powf(a.x, b.x), powf(a.y, b.y), powf(a.z, b.z)); }
inline vec3 exp2(vec3 a) { return vec3(exp2f(a.x), exp2f(a.y), exp2f(a.z)); }
inline vec4 exp2(vec4 a) { return vec4(exp2f(a.x), exp2f(a.y), exp2f(a.z), exp2f(a.w)); }
inline vec3 log2(vec3 a) { return vec3(log2f(a.x), log2f(a.y), log2f(a.z)); }
inline vec2 abs(vec2 a) { return vec2(fabsf(a.x), fabsf(a.y)); }
inline vec3 abs(vec3 a) { return vec3(fabsf(a.x), fabsf(a.y), fabsf(a.z)); }
inline vec4 abs(vec4 a) { return vec4(fabsf(a.x), fabsf(a.y), fabsf(a.z), fabsf(a.w)); }
/* max / min: DESIGN.md §4.14, first bullet of the rule set — a < b ? b : a and b < a ? b : a, arguments in the shader's order */
inline vec3 max(vec3 a, vec3 b) { return vec3(max(a.x, b.x), max(a.y, b.y), max(a.z, b.z)); }
inline vec3 min(vec3 a, vec3 b) { return vec3(min(a.x, b.x), min(a.y, b.y), min(a.z, b.z)); }
inline float dot(vec2 a, vec2 b) { return a.x * b.x + a.y * b.y; }
inline float dot(vec4 a, vec4 b) { return ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w; }
/* normalize: DESIGN.md §4.13 — v / sqrt((x x + y y) + z z), one division per component (no reciprocal, no rsqrt) */
inline vec3 normalize(vec3 v)
{
	float l = sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z);
	return vec3(v.x / l, v.y / l, v.z / l);
}
/* mix: DESIGN.md §4.14, second bullet — mix(x, y, a) = x (1 - a) + y a */
inline float mix(float x, float y, float a) { return x * (1.0f - a) + y * a; }

/* ---- typed images.  The format of every binding is set by the runner from the reference's host code (oracle/ref_runner.cpp) ---- */
enum ImageFormat
{
	FORMAT_R32_SFLOAT,              /* depth: D32_SFLOAT read through texelFetch */
	FORMAT_R8_UNORM,
	FORMAT_R8G8B8A8_UNORM,          /* R in bits 0-7 */
	FORMAT_A2B10G10R10_UNORM_PACK32, /* R in bits 0-9, G 10-19, B 20-29, A 30-31 */
	FORMAT_B10G11R11_UFLOAT_PACK32  /* R in bits 0-10, G 11-21, B 22-31 */
};

struct texture2D
{
	const void* data;
	uint width, height;
	ImageFormat format;
	uint id; /* a material texture: the slot whose texel the caller supplies (see sampler2D) */
};
struct image2D
{
	void* data;
	uint width, height;
	ImageFormat format;
	vec4* handed; /* optional, width * height: the unconverted value each imageStore was handed */
};
/* what the tests' input conditions read: [0] fetches and loads outside the image, [1] stores outside it, [2] those of them with p.x == width
 * inside the rows (shadowfill's odd width), [3..6] texture() taps clamped at the left, right, top, bottom edge; reset by the runner */
static uint shim_stats[7];
struct sampler
{
};

/* UNORM fetch: DESIGN.md §4.14, third bullet — (float)code / (float)(2^bits - 1), one division */
inline float shim_unorm_fetch(uint code, uint top) { return (float)code / (float)top; }
/* UNORM store: DESIGN.md §4.13 — clamp to [0, 1] with NaN -> 0, times 2^bits - 1, round half to even */
inline uint shim_unorm_store(float x, uint top)
{
	float v = x > 0.0f ? x : 0.0f;
	v = v < 1.0f ? v : 1.0f;
	return (uint)rintf(v * (float)top);
}
/* UFLOAT decode: DESIGN.md §4.15, first bullet — exact; denormals decode to their values, exponent 31 is inf / NaN */
inline float shim_ufloat_fetch(uint code, int mbits)
{
	uint e = code >> mbits, m = code & ((1u << mbits) - 1u);
	if (e == 31u)
		return m ? NAN : INFINITY;
	if (e == 0u)
		return ldexpf((float)m, -14 - mbits);
	return ldexpf((float)(m | 1u << mbits), (int)e - 15 - mbits);
}
/* UFLOAT store: DESIGN.md §4.15, second bullet — NaN -> exponent 31 with the top mantissa bit; any other value with the sign bit set -> 0;
 * +inf -> inf; a finite value above the largest finite code -> that code; everything else rounds toward zero */
inline uint shim_ufloat_store(float x, int mbits)
{
	uint bits;
	memcpy(&bits, &x, 4);
	if (x != x)
		return 31u << mbits | 1u << (mbits - 1);
	if (bits >> 31)
		return 0u;
	if (bits == 0x7f800000u)
		return 31u << mbits;
	if (x >= 65536.0f)
		return (31u << mbits) - 1u;
	int e = (int)(bits >> 23) - 127;
	if (e >= -14)
		return (uint)(e + 15) << mbits | (bits & 0x7fffffu) >> (23 - mbits);
	if (e < -14 - mbits)
		return 0u;
	/* a denormal code: floor(x 2^(14 + mbits)); the shift drops the bits below it */
	return ((bits & 0x7fffffu) | 0x800000u) >> (23 - mbits + (-14 - e));
}

inline vec4 shim_decode(const void* data, ImageFormat format, size_t at)
{
	switch (format)
	{
	case FORMAT_R32_SFLOAT: return vec4(((const float*)data)[at], 0, 0, 1);
	case FORMAT_R8_UNORM: return vec4(shim_unorm_fetch(((const uint8_t*)data)[at], 255u), 0, 0, 1);
	case FORMAT_R8G8B8A8_UNORM: {
		uint w = ((const uint*)data)[at];
		return vec4(shim_unorm_fetch(w & 255u, 255u), shim_unorm_fetch(w >> 8 & 255u, 255u), shim_unorm_fetch(w >> 16 & 255u, 255u),
		            shim_unorm_fetch(w >> 24, 255u));
	}
	case FORMAT_A2B10G10R10_UNORM_PACK32: {
		uint w = ((const uint*)data)[at];
		return vec4(shim_unorm_fetch(w & 1023u, 1023u), shim_unorm_fetch(w >> 10 & 1023u, 1023u), shim_unorm_fetch(w >> 20 & 1023u, 1023u),
		            shim_unorm_fetch(w >> 30, 3u));
	}
	case FORMAT_B10G11R11_UFLOAT_PACK32: {
		uint w = ((const uint*)data)[at];
		return vec4(shim_ufloat_fetch(w & 2047u, 6), shim_ufloat_fetch(w >> 11 & 2047u, 6), shim_ufloat_fetch(w >> 22, 5), 1);
	}
	}
	return vec4(0);
}

inline uint shim_encode_word(vec4 v, ImageFormat format)
{
	switch (format)
	{
	case FORMAT_R8G8B8A8_UNORM:
		return shim_unorm_store(v.x, 255u) | shim_unorm_store(v.y, 255u) << 8 | shim_unorm_store(v.z, 255u) << 16 | shim_unorm_store(v.w, 255u) << 24;
	case FORMAT_A2B10G10R10_UNORM_PACK32:
		return shim_unorm_store(v.x, 1023u) | shim_unorm_store(v.y, 1023u) << 10 | shim_unorm_store(v.z, 1023u) << 20 | shim_unorm_store(v.w, 3u) << 30;
	case FORMAT_B10G11R11_UFLOAT_PACK32: return shim_ufloat_store(v.x, 6) | shim_ufloat_store(v.y, 6) << 11 | shim_ufloat_store(v.z, 5) << 22;
	default: return 0;
	}
}

/* out of range: DESIGN.md §4.14, fourth bullet — a fetch outside the image returns 0, a store outside it is dropped */
inline bool shim_inside(ivec2 p, uint w, uint h) { return p.x >= 0 && p.y >= 0 && (uint)p.x < w && (uint)p.y < h; }
inline vec4 texelFetch(texture2D t, ivec2 p, int)
{
	shim_stats[0] += !shim_inside(p, t.width, t.height);
	return shim_inside(p, t.width, t.height) ? shim_decode(t.data, t.format, (size_t)p.y * t.width + (size_t)p.x) : vec4(0);
}
inline vec4 imageLoad(image2D t, ivec2 p)
{
	shim_stats[0] += !shim_inside(p, t.width, t.height);
	return shim_inside(p, t.width, t.height) ? shim_decode(t.data, t.format, (size_t)p.y * t.width + (size_t)p.x) : vec4(0);
}
static ivec2 shim_last_store; /* where the running invocation's last imageStore went, inside the image or not (ref_shadow files its log there) */
inline void imageStore(image2D t, ivec2 p, vec4 v)
{
	shim_last_store = p;
	if (!shim_inside(p, t.width, t.height))
	{
		shim_stats[1]++;
		shim_stats[2] += p.x == (int)t.width && p.y >= 0 && (uint)p.y < t.height;
		return;
	}
	size_t at = (size_t)p.y * t.width + (size_t)p.x;
	if (t.handed)
		t.handed[at] = v;
	if (t.format == FORMAT_R8_UNORM)
		((uint8_t*)t.data)[at] = (uint8_t)shim_unorm_store(v.x, 255u);
	else
		((uint*)t.data)[at] = shim_encode_word(v, t.format);
}

/* ---- texture() ---- */
struct ShimMaterialTaps
{
	vec4 texel[5];   /* texel[id] is what texture(SAMP(id), uv) returns for this fragment */
	uint sampled[5]; /* how often each id was sampled */
};
static ShimMaterialTaps shim_taps;

struct sampler2D
{
	texture2D t;
	sampler2D(texture2D t_, sampler) : t(t_) {}
};
inline uint nonuniformEXT(uint id) { return id; }
/* textures[]: the material sampler is fixed function and pinned elsewhere (tests/test_textures_cpu.py); an element only carries its id */
struct ShimTextureTable
{
	texture2D operator[](uint id) const
	{
		texture2D t = { 0, 0, 0, FORMAT_R8G8B8A8_UNORM, id };
		return t;
	}
};

/* filterSampler: DESIGN.md §4.15, third bullet — linear, clamp to edge, level 0 of the bound view, fp32 weights:
 * u = uv.x W - 0.5, i0 = floor(u), a = u - i0, i1 = i0 + 1, both clamped to [0, W - 1] as floats; per channel
 * (t00 (1 - a) + t10 a) (1 - b) + (t01 (1 - a) + t11 a) b */
inline void shim_filter_axis(float uv, uint size, size_t i[2], float* alpha)
{
	float u = uv * (float)size - 0.5f;
	float f0 = floorf(u), f1 = f0 + 1.0f, top = (float)size - 1.0f;
	*alpha = u - f0;
	f0 = f0 < 0.0f ? 0.0f : f0 > top ? top : f0;
	f1 = f1 < 0.0f ? 0.0f : f1 > top ? top : f1;
	i[0] = f0 == f0 ? (size_t)f0 : 0;
	i[1] = f1 == f1 ? (size_t)f1 : 0;
}
inline float shim_blend(float t00, float t10, float t01, float t11, float a, float b)
{
	return (t00 * (1.0f - a) + t10 * a) * (1.0f - b) + (t01 * (1.0f - a) + t11 * a) * b;
}
inline vec4 texture(sampler2D s, vec2 uv)
{
	if (s.t.data == 0)
	{
		shim_taps.sampled[s.t.id < 5u ? s.t.id : 0u]++;
		return shim_taps.texel[s.t.id < 5u ? s.t.id : 0u];
	}
	size_t xi[2], yi[2];
	float a, b;
	shim_filter_axis(uv.x, s.t.width, xi, &a);
	shim_filter_axis(uv.y, s.t.height, yi, &b);
	float ux = uv.x * (float)s.t.width - 0.5f, uy = uv.y * (float)s.t.height - 0.5f;
	shim_stats[3] += floorf(ux) < 0.0f;
	shim_stats[4] += floorf(ux) + 1.0f > (float)s.t.width - 1.0f;
	shim_stats[5] += floorf(uy) < 0.0f;
	shim_stats[6] += floorf(uy) + 1.0f > (float)s.t.height - 1.0f;
	vec4 t00 = shim_decode(s.t.data, s.t.format, yi[0] * s.t.width + xi[0]), t10 = shim_decode(s.t.data, s.t.format, yi[0] * s.t.width + xi[1]);
	vec4 t01 = shim_decode(s.t.data, s.t.format, yi[1] * s.t.width + xi[0]), t11 = shim_decode(s.t.data, s.t.format, yi[1] * s.t.width + xi[1]);
	return vec4(shim_blend(t00.x, t10.x, t01.x, t11.x, a, b), shim_blend(t00.y, t10.y, t01.y, t11.y, a, b), shim_blend(t00.z, t10.z, t01.z, t11.z, a, b),
	            shim_blend(t00.w, t10.w, t01.w, t11.w, a, b));
}

} // namespace
} // namespace glsl
