/* shade_ref.c — CPU restatement of nv_shadow_fill, nv_shadow_blur and nv_shade_final (include/niagara_vis.h), one pixel at
 * a time.
 *
 * Test infrastructure: compiled by tests/shade_ref.py with raster_ref.py's flags, twice: as it stands (REAL = float: every statement one IEEE
 * fp32 operation, the bits the HIP kernels must write up to pow / exp2) and with -DREAL=double (the same statements in fp64 from the same
 * inputs and the same fp32 constants: the yardstick of the accuracy check).  Written from the rule set of §4.14; every function names the
 * shader lines it restates.
 *
 * Conventions: images are linear, row 0 at the top.  A fetch outside the image returns 0, a store outside it is dropped.  max(a, b) =
 * a < b ? b : a, min(a, b) = b < a ? b : a, arguments in the shader's order.  mat4 * vec4 and dot associate left to right. */
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <tgmath.h>

#ifndef REAL
#define REAL float
#endif
#define K(x) ((REAL)(x)) /* a constant of the shaders: the fp32 value in both builds */

/* src/niagara.cpp:280-290 */
typedef struct
{
	float cameraPosition[3], pad0, sunDirection[3];
	int32_t shadowsEnabled;
	float inverseViewProjection[16], imageSize[2], pad1[2];
} ShadeData;

int sr_real_bytes(void) { return (int)sizeof(REAL); }

/* The accuracy experiment of tests/test_shade_cpu.py: every result of pow and of exp2 with a non-integer argument is moved by sr_ulps fp32
 * ULPs (mode 1: up, 2: down, 3: up or down by a fixed pseudo-random sequence) before it is used.  Only the fp32 build moves anything. */
static int sr_mode, sr_ulps;
static uint32_t sr_lcg;
void sr_set_perturb(int mode, int ulps) { sr_mode = mode, sr_ulps = ulps, sr_lcg = 12345u; }

static REAL sr_libm(REAL v)
{
	if (sizeof(REAL) != sizeof(float) || sr_mode == 0 || !(v > K(0.0f)) || !(v < (REAL)INFINITY))
		return v;
	int step = sr_ulps;
	if (sr_mode == 2)
		step = -step;
	if (sr_mode == 3)
	{
		sr_lcg = sr_lcg * 1664525u + 1013904223u;
		step = (sr_lcg >> 16 & 1u) ? step : -step;
	}
	float f = (float)v;
	uint32_t b;
	memcpy(&b, &f, 4);
	int32_t moved = (int32_t)b + step; /* (a denormal result stays at or above zero, the largest float finite) */
	b = (uint32_t)(moved < 0 ? 0 : moved > 0x7f7fffff ? 0x7f7fffff : moved);
	memcpy(&f, &b, 4);
	return (REAL)f;
}
static REAL sr_pow(REAL x, REAL y) { return sr_libm(pow(x, y)); }
static REAL sr_exp2(REAL x) { return sr_libm(exp2(x)); }

static REAL gl_max(REAL a, REAL b) { return a < b ? b : a; }
static REAL gl_min(REAL a, REAL b) { return b < a ? b : a; }

/* UNORM store, DESIGN.md §4.13: clamp to [0, 1] with NaN -> 0, times 2^bits - 1, round half to even */
static uint32_t sr_unorm8(REAL x)
{
	REAL v = x > K(0.0f) ? x : K(0.0f);
	v = v < K(1.0f) ? v : K(1.0f);
	return (uint32_t)rint(v * K(255.0f));
}

/* texelFetch of an R32F image: 0 outside */
static REAL sr_depth(const float* img, uint32_t w, uint32_t h, int64_t x, int64_t y)
{
	return x < 0 || y < 0 || x >= (int64_t)w || y >= (int64_t)h ? K(0.0f) : (REAL)img[(size_t)y * w + (size_t)x];
}

/* texelFetch / imageLoad of an R8_UNORM image: code / 255, 0 outside */
static REAL sr_r8(const uint8_t* img, uint32_t w, uint32_t h, int64_t x, int64_t y)
{
	return x < 0 || y < 0 || x >= (int64_t)w || y >= (int64_t)h ? K(0.0f) : (REAL)img[(size_t)y * w + (size_t)x] / K(255.0f);
}

/* shadowfill.comp.glsl:17-46 over (w + 1) / 2 x h invocations, in place (an invocation reads texels of the other parity only, so the order of
 * the invocations does not matter).  value (optional, w * h): what is handed to the store, for the written texels. */
void sr_shadow_fill(uint8_t* shadow, const float* depth, uint32_t w, uint32_t h, int checkerboard, REAL* value)
{
	static const int off[4][2] = { { -1, 0 }, { +1, 0 }, { 0, -1 }, { 0, +1 } }; /* :27-39 */
	for (uint32_t gy = 0; gy < h; ++gy)
		for (uint32_t gx = 0; gx < (w + 1u) / 2u; ++gx)
		{
			int64_t px = (int64_t)gx * 2, py = gy; /* :19-23 */
			px += ~((int32_t)gy ^ checkerboard) & 1;
			REAL d = sr_depth(depth, w, h, px, py); /* :25 */
			REAL wgt[4], sh[4];
			for (int k = 0; k < 4; ++k)
			{
				REAL dk = sr_depth(depth, w, h, px + off[k][0], py + off[k][1]);
				sh[k] = sr_r8(shadow, w, h, px + off[k][0], py + off[k][1]);
				wgt[k] = sr_exp2(-fabs(dk / d - K(1.0f)) * K(20.0f)); /* :41 */
			}
			/* :43 */
			REAL num = ((wgt[0] * sh[0] + wgt[1] * sh[1]) + wgt[2] * sh[2]) + wgt[3] * sh[3];
			REAL den = ((wgt[0] * K(1.0f) + wgt[1] * K(1.0f)) + wgt[2] * K(1.0f)) + wgt[3] * K(1.0f);
			REAL s = num / (den + K(1e-2f));
			if (px < (int64_t)w) /* :45, a store outside the image is dropped */
			{
				shadow[(size_t)py * w + (size_t)px] = (uint8_t)sr_unorm8(s);
				if (value)
					value[(size_t)py * w + (size_t)px] = s;
			}
		}
}

/* shadowblur.comp.glsl:48: exp2(-i * i / 50) in the shader's integer arithmetic, i = 1..10 */
void sr_gw(float out[10])
{
	for (int i = 1; i <= 10; ++i)
		out[i - 1] = (float)exp2((REAL)(-i * i / 50));
}

/* shadowblur.comp.glsl:24-64 with BLUR 1; direction 1 = horizontal, 0 = vertical (:34: offsetMask = -ivec2(direction, 1 - direction)) */
void sr_shadow_blur(uint8_t* out, const uint8_t* shadowImage, const float* depthImage, uint32_t w, uint32_t h, int direction, float znearf, REAL* value)
{
	const int mx = direction ? 1 : 0, my = direction ? 0 : 1;
	const REAL znear = znearf;
	for (uint32_t y = 0; y < h; ++y)
		for (uint32_t x = 0; x < w; ++x)
		{
			REAL shadow = sr_r8(shadowImage, w, h, x, y), accumw = K(1.0f); /* :29-30 */
			REAL depth = znear / sr_depth(depthImage, w, h, x, y);         /* :32 */
			for (int sign = -1; sign <= 1; sign += 2)
			{
				REAL dnext = znear / sr_depth(depthImage, w, h, (int64_t)x + sign * mx, (int64_t)y + sign * my); /* :40-41 */
				REAL dgrad = fabs(depth - dnext) < K(0.1f) ? dnext - depth : K(0.0f);                             /* :42 */
				for (int i = 1; i <= 10; ++i)
				{
					int64_t ox = (int64_t)x + i * sign * mx, oy = (int64_t)y + i * sign * my; /* :46 */
					REAL gw = exp2((REAL)(-i * i / 50));                                      /* :48, an integer argument: exact */
					REAL dv = znear / sr_depth(depthImage, w, h, ox, oy);                     /* :49 */
					REAL dw = sr_exp2(-fabs(dv - (depth + dgrad * (REAL)i)) * K(100.0f));     /* :50 */
					REAL fw = gw * dw;                                                        /* :51 */
					shadow = shadow + sr_r8(shadowImage, w, h, ox, oy) * fw;                  /* :53 */
					accumw = accumw + fw;                                                     /* :54 */
				}
			}
			shadow = shadow / accumw; /* :58 */
			out[(size_t)y * w + x] = (uint8_t)sr_unorm8(shadow);
			if (value)
				value[(size_t)y * w + x] = shadow;
		}
}

/* normalize(v), DESIGN.md §4.13 */
static void sr_normalize(REAL v[3])
{
	REAL l = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
	v[0] = v[0] / l, v[1] = v[1] / l, v[2] = v[2] / l;
}

/* src/shaders/math.h:60-67 decodeOct */
static void sr_decode_oct(REAL ex, REAL ey, REAL v[3])
{
	v[0] = ex, v[1] = ey, v[2] = (K(1.0f) - fabs(ex)) - fabs(ey);
	REAL t = gl_max(-v[2], K(0.0f));
	v[0] = v[0] + (v[0] >= K(0.0f) ? -t : t);
	v[1] = v[1] + (v[1] >= K(0.0f) ? -t : t);
	sr_normalize(v);
}

/* src/shaders/math.h:91-95 tonemap, one component */
static REAL sr_tonemap(REAL c)
{
	REAL x = gl_max(K(0.0f), c - K(0.004f));
	return (x * (K(6.2f) * x + K(0.5f))) / (x * (K(6.2f) * x + K(1.7f)) + K(0.06f));
}

/* src/shaders/math.h:99-102 gradientNoise, fract(x) = x - floor(x) */
static REAL sr_gradient_noise(REAL x, REAL y)
{
	REAL inner = x * K(0.06711056f) + y * K(0.00583715f);
	REAL f = inner - floor(inner);
	REAL n = K(52.9829189f) * f;
	return n - floor(n);
}

/* thin exported wrappers over the static helpers above, for tests/test_shading_vs_ref.py (arrays of n arguments) */
void sr_x_decode_oct(const REAL* e, uint32_t n, REAL* out3)
{
	for (uint32_t i = 0; i < n; ++i)
		sr_decode_oct(e[2 * (size_t)i], e[2 * (size_t)i + 1], out3 + 3 * (size_t)i);
}
void sr_x_tonemap(const REAL* c, uint32_t n, REAL* out)
{
	for (uint32_t i = 0; i < n; ++i)
		out[i] = sr_tonemap(c[i]);
}
void sr_x_gradient_noise(const REAL* xy, uint32_t n, REAL* out)
{
	for (uint32_t i = 0; i < n; ++i)
		out[i] = sr_gradient_noise(xy[2 * (size_t)i], xy[2 * (size_t)i + 1]);
}
/* fromsrgb as :46 of final.comp.glsl is restated below (:210 here) */
void sr_x_fromsrgb(const REAL* c, uint32_t n, REAL* out)
{
	for (uint32_t i = 0; i < n; ++i)
		out[i] = sr_pow(c[i], K(2.2f));
}

/* final.comp.glsl:37-80 with an all-zero bloom image.  shadow may be NULL unless sd->shadowsEnabled == 1.  value (optional, w * h * 4):
 * tonemap(outputColor).rgb and the deband term deband * (0.5 / 255) per pixel, before they are added and stored. */
void sr_shade_final(const ShadeData* sd, const uint32_t* gbuffer0, const uint32_t* gbuffer1, const float* depthImage, const uint8_t* shadowImage,
                    uint32_t* color, uint32_t w, uint32_t h, REAL* value)
{
	const float* m = sd->inverseViewProjection;
	const REAL sun[3] = { sd->sunDirection[0], sd->sunDirection[1], sd->sunDirection[2] };
	for (uint32_t py = 0; py < h; ++py)
		for (uint32_t px = 0; px < w; ++px)
		{
			const size_t at = (size_t)py * w + px;
			/* :40 */
			REAL uvx = ((REAL)px + K(0.5f)) / (REAL)sd->imageSize[0], uvy = ((REAL)py + K(0.5f)) / (REAL)sd->imageSize[1];
			/* :42-44 UNORM fetch */
			uint32_t a0 = gbuffer0[at], a1 = gbuffer1[at];
			REAL g0[4], g1[3];
			for (int k = 0; k < 4; ++k)
				g0[k] = (REAL)(a0 >> (8 * k) & 255u) / K(255.0f);
			for (int k = 0; k < 3; ++k)
				g1[k] = (REAL)(a1 >> (10 * k) & 1023u) / K(1023.0f);
			REAL depth = depthImage[at];
			/* :46-48 */
			REAL albedo[3], emissive[3], normal[3];
			for (int k = 0; k < 3; ++k)
				albedo[k] = sr_pow(g0[k], K(2.2f));
			REAL e = sr_exp2(g0[3] * K(5.0f)) - K(1.0f);
			for (int k = 0; k < 3; ++k)
				emissive[k] = albedo[k] * e;
			sr_decode_oct(g1[0] * K(2.0f) - K(1.0f), g1[1] * K(2.0f) - K(1.0f), normal);
			/* :50 */
			REAL ndotl = gl_max((normal[0] * sun[0] + normal[1] * sun[1]) + normal[2] * sun[2], K(0.0f));
			/* :52-54 */
			REAL clip[4] = { uvx * K(2.0f) - K(1.0f), K(1.0f) - uvy * K(2.0f), depth, K(1.0f) }, wposh[4], view[3], halfv[3];
			for (int r = 0; r < 4; ++r)
				wposh[r] = (((REAL)m[r] * clip[0] + (REAL)m[4 + r] * clip[1]) + (REAL)m[8 + r] * clip[2]) + (REAL)m[12 + r] * clip[3];
			/* :56-58 */
			for (int k = 0; k < 3; ++k)
				view[k] = (REAL)sd->cameraPosition[k] - wposh[k] / wposh[3];
			sr_normalize(view);
			for (int k = 0; k < 3; ++k)
				halfv[k] = view[k] + sun[k];
			sr_normalize(halfv);
			REAL ndoth = gl_max((normal[0] * halfv[0] + normal[1] * halfv[1]) + normal[2] * halfv[2], K(0.0f));
			REAL gloss = g1[2];
			/* :62, mix(1, 64, g) = 1 (1 - g) + 64 g */
			REAL specular = sr_pow(ndoth, K(1.0f) * (K(1.0f) - gloss) + K(64.0f) * gloss) * gloss;
			/* :64-66 */
			REAL shadow = K(1.0f);
			if (sd->shadowsEnabled == 1)
				shadow = (REAL)shadowImage[at] / K(255.0f);
			/* :73-76 */
			REAL lit = (ndotl * gl_min(shadow + K(0.05f), K(1.0f))) * K(2.5f) + K(0.07f);
			REAL spec = (specular * shadow) * K(2.5f);
			REAL bloom = K(0.0f) * K(0.1f);
			/* :78-79 */
			REAL band = (sr_gradient_noise((REAL)px, (REAL)py) * K(2.0f) - K(1.0f)) * (K(0.5f) / K(255.0f));
			uint32_t word = 255u << 24;
			for (int k = 0; k < 3; ++k)
			{
				REAL o = ((albedo[k] * lit + spec) + emissive[k]) + bloom;
				REAL t = sr_tonemap(o);
				word |= sr_unorm8(t + band) << (8 * k);
				if (value)
					value[at * 4 + k] = t;
			}
			if (value)
				value[at * 4 + 3] = band;
			color[at] = word;
		}
}
