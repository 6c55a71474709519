/* bloom_ref.c — CPU restatement of nv_bloom_extract, nv_bloom_downsample, nv_bloom_upsample and nv_shade_final_bloom (include/niagara_vis.h,
 * DESIGN.md §4.15), one texel at a time.
 *
 * Test infrastructure: compiled by tests/bloom_ref.py with raster_ref.py's flags, twice, as shade_ref.c is: as it stands (REAL = float: every
 * statement one IEEE fp32 operation, the bits the HIP kernels must write up to pow / exp2) and with -DREAL=double (the same statements in fp64
 * from the same inputs and the same fp32 constants).  It includes shade_ref.c for the helpers of final.comp.glsl (pow / exp2 with their
 * perturbation, decodeOct, tonemap, gradientNoise, the UNORM store) and restates final.comp.glsl:37-80 once more, this time with :76.
 *
 * The UFLOAT store works on the value (frexp, floor), not on the float's bits as niagara_amd/csrc/bloommath.h does: two statements of one rule. */
#include "shade_ref.c"

/* ---- VK_FORMAT_B10G11R11_UFLOAT_PACK32: R bits 0-10 and G bits 11-21 with 6 mantissa bits, B bits 22-31 with 5; exponent 5 bits, bias 15 */

static REAL br_decode(uint32_t code, int mbits)
{
	uint32_t e = code >> mbits, m = code & ((1u << mbits) - 1u);
	if (e == 0u) /* a denormal: its value */
		return (REAL)ldexp((double)m, -14 - mbits);
	if (e == 31u)
		return m ? (REAL)NAN : (REAL)INFINITY;
	return (REAL)ldexp(1.0 + ldexp((double)m, -mbits), (int)e - 15);
}

/* the store: NaN -> exponent 31 and the top mantissa bit; else the sign bit -> 0; +inf -> inf; finite above the largest finite code -> that
 * code; else toward zero (every REAL is a double exactly, so the arithmetic below is exact) */
static uint32_t br_encode(REAL value, int mbits)
{
	double d = (double)value;
	if (d != d)
		return 31u << mbits | 1u << (mbits - 1);
	if (signbit(d))
		return 0u;
	if (isinf(d))
		return 31u << mbits;
	if (d >= 65536.0)
		return (31u << mbits) - 1u;
	if (d >= ldexp(1.0, -14))
	{
		int ex;
		double fr = frexp(d, &ex); /* d = fr 2^ex, 0.5 <= fr < 1 */
		uint32_t mant = (uint32_t)floor((fr * 2.0 - 1.0) * (double)(1u << mbits));
		return (uint32_t)(ex - 1 + 15) << mbits | mant;
	}
	return (uint32_t)floor(ldexp(d, 14 + mbits));
}

void br_decode_array(const uint32_t* codes, uint32_t n, int mbits, REAL* out)
{
	for (uint32_t i = 0; i < n; ++i)
		out[i] = br_decode(codes[i], mbits);
}

void br_encode_array(const REAL* values, uint32_t n, int mbits, uint32_t* out)
{
	for (uint32_t i = 0; i < n; ++i)
		out[i] = br_encode(values[i], mbits);
}

static void br_unpack(uint32_t word, REAL rgb[3])
{
	rgb[0] = br_decode(word & 2047u, 6), rgb[1] = br_decode(word >> 11 & 2047u, 6), rgb[2] = br_decode(word >> 22, 5);
}

static uint32_t br_pack(const REAL rgb[3]) { return br_encode(rgb[0], 6) | br_encode(rgb[1], 6) << 11 | br_encode(rgb[2], 5) << 22; }

/* ---- texture() with filterSampler: linear, clamp to edge, level 0 of the bound view */

typedef struct
{
	int64_t i0, i1;
	REAL alpha;
} Axis;

static Axis br_axis(REAL uv, uint32_t size)
{
	REAL u = uv * (REAL)size - K(0.5f);
	REAL f0 = floor(u), f1 = f0 + K(1.0f), top = (REAL)size - K(1.0f);
	Axis a;
	a.alpha = u - f0;
	a.i0 = (int64_t)(f0 < K(0.0f) ? K(0.0f) : f0 > top ? top : f0);
	a.i1 = (int64_t)(f1 < K(0.0f) ? K(0.0f) : f1 > top ? top : f1);
	return a;
}

static REAL br_lerp2(REAL t00, REAL t10, REAL t01, REAL t11, REAL a, REAL b)
{
	return (t00 * (K(1.0f) - a) + t10 * a) * (K(1.0f) - b) + (t01 * (K(1.0f) - a) + t11 * a) * b;
}

/* texture(sampler2D(image, filterSampler), (u, v)).rgb of a UFLOAT level */
static void br_texture(const uint32_t* img, uint32_t w, uint32_t h, REAL u, REAL v, REAL out[3])
{
	Axis ax = br_axis(u, w), ay = br_axis(v, h);
	REAL t00[3], t10[3], t01[3], t11[3];
	br_unpack(img[(size_t)ay.i0 * w + (size_t)ax.i0], t00), br_unpack(img[(size_t)ay.i0 * w + (size_t)ax.i1], t10);
	br_unpack(img[(size_t)ay.i1 * w + (size_t)ax.i0], t01), br_unpack(img[(size_t)ay.i1 * w + (size_t)ax.i1], t11);
	for (int k = 0; k < 3; ++k)
		out[k] = br_lerp2(t00[k], t10[k], t01[k], t11[k], ax.alpha, ay.alpha);
}

/* the same of an R8G8B8A8_UNORM image, filtered on the stored codes: rgba */
static void br_texture_unorm8(const uint32_t* img, uint32_t w, uint32_t h, REAL u, REAL v, REAL out[4])
{
	Axis ax = br_axis(u, w), ay = br_axis(v, h);
	uint32_t w00 = img[(size_t)ay.i0 * w + (size_t)ax.i0], w10 = img[(size_t)ay.i0 * w + (size_t)ax.i1];
	uint32_t w01 = img[(size_t)ay.i1 * w + (size_t)ax.i0], w11 = img[(size_t)ay.i1 * w + (size_t)ax.i1];
	for (int k = 0; k < 4; ++k)
		out[k] = br_lerp2((REAL)(w00 >> (8 * k) & 255u) / K(255.0f), (REAL)(w10 >> (8 * k) & 255u) / K(255.0f), (REAL)(w01 >> (8 * k) & 255u) / K(255.0f),
		                  (REAL)(w11 >> (8 * k) & 255u) / K(255.0f), ax.alpha, ay.alpha);
}

/* ---- bloom.comp.glsl */

/* :29-46, pass 0: gbuffer0 (W x H) into level 0 (w x h).  value (optional, w * h * 3, here and in passes 1 and 2): what is handed to the store */
void br_extract(const uint32_t* gbuffer0, uint32_t W, uint32_t H, uint32_t* out, uint32_t w, uint32_t h, REAL* value)
{
	static const float off[4][2] = { { -0.25f, -0.25f }, { +0.25f, -0.25f }, { -0.25f, +0.25f }, { +0.25f, +0.25f } }; /* :33-36 */
	REAL tx = K(1.0f) / (REAL)w, ty = K(1.0f) / (REAL)h;                                                               /* :27 */
	for (uint32_t y = 0; y < h; ++y)
		for (uint32_t x = 0; x < w; ++x)
		{
			REAL uvx = ((REAL)x + K(0.5f)) / (REAL)w, uvy = ((REAL)y + K(0.5f)) / (REAL)h; /* :26 */
			REAL e[4][3];
			for (int s = 0; s < 4; ++s)
			{
				REAL t[4];
				br_texture_unorm8(gbuffer0, W, H, uvx + tx * K(off[s][0]), uvy + ty * K(off[s][1]), t);
				REAL scale = sr_exp2(t[3] * K(5.0f)) - K(1.0f); /* :38 */
				for (int k = 0; k < 3; ++k)
					e[s][k] = sr_pow(t[k], K(2.2f)) * scale;
			}
			REAL result[3];
			for (int k = 0; k < 3; ++k)
				result[k] = (((e[0][k] + e[1][k]) + e[2][k]) + e[3][k]) * K(0.25f); /* :43 */
			out[(size_t)y * w + x] = br_pack(result);
			if (value)
				memcpy(value + ((size_t)y * w + x) * 3, result, sizeof(result));
		}
}

/* :47-77, pass 1 with QUALITY 1: src (W x H) into dst (w x h) */
void br_downsample(const uint32_t* src, uint32_t W, uint32_t H, uint32_t* dst, uint32_t w, uint32_t h, REAL* value)
{
	/* :54-66: the offsets in texels of dst and the weights as the shader writes them */
	static const float tap[13][2] = { { 0, 0 }, { +0.5f, +0.5f }, { +0.5f, -0.5f }, { -0.5f, +0.5f }, { -0.5f, -0.5f }, { +1, +1 }, { +1, -1 },
		                              { -1, +1 }, { -1, -1 },       { +1, 0 },        { -1, 0 },        { 0, +1 },        { 0, -1 } };
	const REAL weight[13] = { K(0.125f),        K(0.5f) / K(4.0f),   K(0.5f) / K(4.0f),   K(0.5f) / K(4.0f),   K(0.5f) / K(4.0f),
		                      K(0.125f) / K(4.0f), K(0.125f) / K(4.0f), K(0.125f) / K(4.0f), K(0.125f) / K(4.0f), K(0.125f) / K(2.0f),
		                      K(0.125f) / K(2.0f), K(0.125f) / K(2.0f), K(0.125f) / K(2.0f) };
	REAL tx = K(1.0f) / (REAL)w, ty = K(1.0f) / (REAL)h;
	for (uint32_t y = 0; y < h; ++y)
		for (uint32_t x = 0; x < w; ++x)
		{
			REAL uvx = ((REAL)x + K(0.5f)) / (REAL)w, uvy = ((REAL)y + K(0.5f)) / (REAL)h;
			REAL result[3] = { K(0.0f), K(0.0f), K(0.0f) }; /* :50 */
			for (int s = 0; s < 13; ++s)
			{
				REAL t[3];
				/* :54 samples uv itself; uv + texelSize * 0 is the same value */
				br_texture(src, W, H, s ? uvx + tx * K(tap[s][0]) : uvx, s ? uvy + ty * K(tap[s][1]) : uvy, t);
				for (int k = 0; k < 3; ++k)
					result[k] = result[k] + t[k] * weight[s];
			}
			dst[(size_t)y * w + x] = br_pack(result);
			if (value)
				memcpy(value + ((size_t)y * w + x) * 3, result, sizeof(result));
		}
}

/* :78-107, pass 2 with QUALITY 1: src (W x H) added to dst (w x h) in place; an invocation touches its own texel of dst only */
void br_upsample(const uint32_t* src, uint32_t W, uint32_t H, uint32_t* dst, uint32_t w, uint32_t h, float radiusf, REAL* value)
{
	static const float tap[9][2] = { { 0, 0 }, { +1, 0 }, { -1, 0 }, { 0, +1 }, { 0, -1 }, { +1, +1 }, { +1, -1 }, { -1, +1 }, { -1, -1 } }; /* :85-93 */
	const REAL weight[9] = { K(4.0f) / K(16.0f), K(2.0f) / K(16.0f), K(2.0f) / K(16.0f), K(2.0f) / K(16.0f), K(2.0f) / K(16.0f),
		                     K(1.0f) / K(16.0f), K(1.0f) / K(16.0f), K(1.0f) / K(16.0f), K(1.0f) / K(16.0f) };
	REAL radius = radiusf;
	REAL rx = (K(1.0f) / (REAL)w) * radius, ry = (K(1.0f) / (REAL)h) * radius; /* texelSize * radius, left to right */
	for (uint32_t y = 0; y < h; ++y)
		for (uint32_t x = 0; x < w; ++x)
		{
			REAL uvx = ((REAL)x + K(0.5f)) / (REAL)w, uvy = ((REAL)y + K(0.5f)) / (REAL)h;
			REAL result[3];
			br_unpack(dst[(size_t)y * w + x], result); /* :81 */
			for (int s = 0; s < 9; ++s)
			{
				REAL t[3];
				br_texture(src, W, H, s ? uvx + rx * K(tap[s][0]) : uvx, s ? uvy + ry * K(tap[s][1]) : uvy, t);
				for (int k = 0; k < 3; ++k)
					result[k] = result[k] + t[k] * weight[s];
			}
			dst[(size_t)y * w + x] = br_pack(result);
			if (value)
				memcpy(value + ((size_t)y * w + x) * 3, result, sizeof(result));
		}
}

/* ---- final.comp.glsl:37-80 with the bloom term: bloom is level 0 (bw x bh) of the bloom target.  The statements are sr_shade_final's except
 * :76.  value (optional, w * h * 4) as there. */
void br_shade_final_bloom(const ShadeData* sd, const uint32_t* gbuffer0, const uint32_t* gbuffer1, const float* depthImage, const uint8_t* shadowImage,
                          const uint32_t* bloomImage, uint32_t bw, uint32_t bh, uint32_t* color, uint32_t w, uint32_t h, REAL* value)
{
	const float* m = sd->inverseViewProjection;
	const REAL sun[3] = { sd->sunDirection[0], sd->sunDirection[1], sd->sunDirection[2] };
	for (uint32_t py = 0; py < h; ++py)
		for (uint32_t px = 0; px < w; ++px)
		{
			const size_t at = (size_t)py * w + px;
			REAL uvx = ((REAL)px + K(0.5f)) / (REAL)sd->imageSize[0], uvy = ((REAL)py + K(0.5f)) / (REAL)sd->imageSize[1]; /* :40 */
			uint32_t a0 = gbuffer0[at], a1 = gbuffer1[at];
			REAL g0[4], g1[3];
			for (int k = 0; k < 4; ++k)
				g0[k] = (REAL)(a0 >> (8 * k) & 255u) / K(255.0f);
			for (int k = 0; k < 3; ++k)
				g1[k] = (REAL)(a1 >> (10 * k) & 1023u) / K(1023.0f);
			REAL depth = depthImage[at];
			REAL albedo[3], emissive[3], normal[3]; /* :46-48 */
			for (int k = 0; k < 3; ++k)
				albedo[k] = sr_pow(g0[k], K(2.2f));
			REAL e = sr_exp2(g0[3] * K(5.0f)) - K(1.0f);
			for (int k = 0; k < 3; ++k)
				emissive[k] = albedo[k] * e;
			sr_decode_oct(g1[0] * K(2.0f) - K(1.0f), g1[1] * K(2.0f) - K(1.0f), normal);
			REAL ndotl = gl_max((normal[0] * sun[0] + normal[1] * sun[1]) + normal[2] * sun[2], K(0.0f)); /* :50 */
			REAL clip[4] = { uvx * K(2.0f) - K(1.0f), K(1.0f) - uvy * K(2.0f), depth, K(1.0f) }, wposh[4], view[3], halfv[3]; /* :52-54 */
			for (int r = 0; r < 4; ++r)
				wposh[r] = (((REAL)m[r] * clip[0] + (REAL)m[4 + r] * clip[1]) + (REAL)m[8 + r] * clip[2]) + (REAL)m[12 + r] * clip[3];
			for (int k = 0; k < 3; ++k) /* :56-58 */
				view[k] = (REAL)sd->cameraPosition[k] - wposh[k] / wposh[3];
			sr_normalize(view);
			for (int k = 0; k < 3; ++k)
				halfv[k] = view[k] + sun[k];
			sr_normalize(halfv);
			REAL ndoth = gl_max((normal[0] * halfv[0] + normal[1] * halfv[1]) + normal[2] * halfv[2], K(0.0f));
			REAL gloss = g1[2];
			REAL specular = sr_pow(ndoth, K(1.0f) * (K(1.0f) - gloss) + K(64.0f) * gloss) * gloss; /* :62 */
			REAL shadow = K(1.0f);                                                                /* :64-66 */
			if (sd->shadowsEnabled == 1)
				shadow = (REAL)shadowImage[at] / K(255.0f);
			REAL lit = (ndotl * gl_min(shadow + K(0.05f), K(1.0f))) * K(2.5f) + K(0.07f); /* :73-75 */
			REAL spec = (specular * shadow) * K(2.5f);
			REAL bloom[3]; /* :76 */
			br_texture(bloomImage, bw, bh, uvx, uvy, bloom);
			REAL band = (sr_gradient_noise((REAL)px, (REAL)py) * K(2.0f) - K(1.0f)) * (K(0.5f) / K(255.0f)); /* :78-79 */
			uint32_t word = 255u << 24;
			for (int k = 0; k < 3; ++k)
			{
				REAL o = ((albedo[k] * lit + spec) + emissive[k]) + bloom[k] * K(0.1f);
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
