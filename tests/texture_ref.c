/* texture_ref.c — CPU restatement of the material textures: the BC1 / BC2 / BC3 / BC7 decode, `textureSampler` as a
 * software sampler, the analytic level of detail and nv_visibility_attributes_textured, one pixel at a time.
 *
 * Test infrastructure, written from the format specification (Khronos Data Format 1.3 §§18-20: S3TC and BPTC) and DESIGN.md §4.18's rule
 * set, NOT from niagara_amd/csrc/texmath.h: the decode here reads a block as a sequential bit stream into plain arrays, expands 5/6-bit
 * colours by rounded division and computes the BC7 weights by their defining formula; texmath.h addresses bits by position and uses
 * packed literals.  Both are held to tests/golden/textures/bc_blocks.npz.  Compiled by tests/texture_ref.py twice: as fp32
 * (the bits the kernels must write) and with -DREAL=double (the yardstick).  visattr_ref.c is included, unedited, for the triangle set-up,
 * the vertex stage and the packing of §4.13. */
#include "visattr_ref.c"

/* ---- block decode.  out: 16 texels RGBA8, R in the low byte, row-major */
typedef struct
{
	const uint8_t* p;
	int at;
} BitReader;

static uint32_t rd(BitReader* b, int n)
{
	uint32_t v = 0;
	for (int k = 0; k < n; ++k, ++b->at)
		v |= (uint32_t)(b->p[b->at >> 3] >> (b->at & 7) & 1u) << k;
	return v;
}

static uint32_t div_round(uint32_t x, uint32_t d) { return (2u * x + d) / (2u * d); } /* round(x / d), halves up */

/* S3TC colour block: endpoints RGB565; c0 > c1 (or BC2 / BC3): thirds, else half and transparent black.  Interpolated in 5/6 bits, then
 * scaled to 8 bits: round(x 255 / (31 k)) and round(x 255 / (63 k)) for an interpolant summed over k weights */
static void tr_colour_block(const uint8_t* blk, int opaque, uint32_t out[16])
{
	uint32_t c[2] = { blk[0] | (uint32_t)blk[1] << 8, blk[2] | (uint32_t)blk[3] << 8 }, pal[4];
	uint32_t e[2][3];
	for (int k = 0; k < 2; ++k)
		e[k][0] = c[k] >> 11 & 31u, e[k][1] = c[k] >> 5 & 63u, e[k][2] = c[k] & 31u;
	const uint32_t top[3] = { 31u, 63u, 31u };
	int four = c[0] > c[1] || opaque;
	for (int i = 0; i < 4; ++i)
	{
		uint32_t w0, w1; /* weights of e[0], e[1] */
		if (i < 2)
			w0 = i == 0, w1 = i == 1;
		else if (four)
			w0 = i == 2 ? 2 : 1, w1 = 3 - w0;
		else
			w0 = w1 = 1;
		pal[i] = 0xff000000u;
		for (int ch = 0; ch < 3; ++ch)
			pal[i] |= div_round((w0 * e[0][ch] + w1 * e[1][ch]) * 255u, top[ch] * (w0 + w1)) << (8 * ch);
		if (i == 3 && !four)
			pal[i] = 0;
	}
	for (int t = 0; t < 16; ++t)
		out[t] = pal[blk[4 + t / 4] >> (2 * (t % 4)) & 3u];
}

static void tr_bc3_alpha(const uint8_t* blk, uint32_t a[16])
{
	uint32_t pal[8] = { blk[0], blk[1] };
	if (pal[0] > pal[1])
		for (uint32_t i = 1; i < 7; ++i)
			pal[i + 1] = ((7 - i) * pal[0] + i * pal[1]) / 7;
	else
	{
		for (uint32_t i = 1; i < 5; ++i)
			pal[i + 1] = ((5 - i) * pal[0] + i * pal[1]) / 5;
		pal[6] = 0, pal[7] = 255;
	}
	uint64_t bits = 0;
	for (int k = 0; k < 6; ++k)
		bits |= (uint64_t)blk[2 + k] << (8 * k);
	for (int t = 0; t < 16; ++t)
		a[t] = pal[bits >> (3 * t) & 7u];
}

/* BPTC partitions: the subset of each texel, texel 0 first; anchors (fix-up indices) of the second / third subset */
static const char* const P2[64] = {
	"0011001100110011", "0001000100010001", "0111011101110111", "0001001100110111", "0000000100010011", "0011011101111111", "0001001101111111", "0000000100110111",
	"0000000000010011", "0011011111111111", "0000000101111111", "0000000000010111", "0001011111111111", "0000000011111111", "0000111111111111", "0000000000001111",
	"0000100011101111", "0111000100000000", "0000000010001110", "0111001100010000", "0011000100000000", "0000100011001110", "0000000010001100", "0111001100110001",
	"0011000100010000", "0000100010001100", "0110011001100110", "0011011001101100", "0001011111101000", "0000111111110000", "0111000110001110", "0011100110011100",
	"0101010101010101", "0000111100001111", "0101101001011010", "0011001111001100", "0011110000111100", "0101010110101010", "0110100101101001", "0101101010100101",
	"0111001111001110", "0001001111001000", "0011001001001100", "0011101111011100", "0110100110010110", "0011110011000011", "0110011010011001", "0000011001100000",
	"0100111001000000", "0010011100100000", "0000001001110010", "0000010011100100", "0110110010010011", "0011011011001001", "0110001110011100", "0011100111000110",
	"0110110011001001", "0110001100111001", "0111111010000001", "0001100011100111", "0000111100110011", "0011001111110000", "0010001011101110", "0100010001110111",
};
static const char* const P3[64] = {
	"0011001102212222", "0001001122112221", "0000200122112211", "0222002200110111", "0000000011221122", "0011001100220022", "0022002211111111", "0011001122112211",
	"0000000011112222", "0000111111112222", "0000111122222222", "0012001200120012", "0112011201120112", "0122012201220122", "0011011211221222", "0011200122002220",
	"0001001101121122", "0111001120012200", "0000112211221122", "0022002200221111", "0111011102220222", "0001000122212221", "0000001101220122", "0000110022102210",
	"0122012200110000", "0012001211222222", "0110122112210110", "0000011012211221", "0022110211020022", "0110011020022222", "0011012201220011", "0000200022112221",
	"0000000211221222", "0222002200120011", "0011001200220222", "0120012001200120", "0000111122220000", "0120120120120120", "0120201212010120", "0011220011220011",
	"0011112222000011", "0101010122222222", "0000000021212121", "0022112200221122", "0022001100220011", "0220122102201221", "0101222222220101", "0000212121212121",
	"0101010101012222", "0222011102220111", "0002111200021112", "0000211221122112", "0222011101110222", "0002111211120002", "0110011001102222", "0000000021122112",
	"0110011022222222", "0022001100110022", "0022112211220022", "0000000000002112", "0002000100020001", "0222122202221222", "0101222222222222", "0111201122012220",
};
static const uint8_t A2[64] = { 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 2, 8, 2, 2, 8, 8, 15, 2, 8, 2, 2, 8, 8, 2, 2,
	                            15, 15, 6, 8, 2, 8, 15, 15, 2, 8, 2, 2, 2, 15, 15, 6, 6, 2, 6, 8, 15, 15, 2, 2, 15, 15, 15, 15, 15, 2, 2, 15 };
static const uint8_t A3a[64] = { 3, 3, 15, 15, 8, 3, 15, 15, 8, 8, 6, 6, 6, 5, 3, 3, 3, 3, 8, 15, 3, 3, 6, 10, 5, 8, 8, 6, 8, 5, 15, 15,
	                             8, 15, 3, 5, 6, 10, 8, 15, 15, 3, 15, 5, 15, 15, 15, 15, 3, 15, 5, 5, 5, 8, 5, 10, 5, 10, 8, 13, 15, 12, 3, 3 };
static const uint8_t A3b[64] = { 15, 8, 8, 3, 15, 15, 3, 8, 15, 15, 15, 15, 15, 15, 15, 8, 15, 8, 15, 3, 15, 8, 15, 8, 3, 15, 6, 10, 15, 15, 10, 8,
	                             15, 3, 15, 10, 10, 8, 9, 10, 6, 15, 8, 15, 3, 6, 6, 8, 15, 3, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 3, 15, 15, 8 };

static uint32_t bptc_weight(int bits, uint32_t i) { return div_round(64u * i, (1u << bits) - 1u); }
static uint32_t bptc_mix(uint32_t a, uint32_t b, uint32_t w) { return (a * (64u - w) + b * w + 32u) >> 6; }

static void tr_bc7_block(const uint8_t* blk, uint32_t out[16])
{
	/* per mode: subsets, partition bits, rotation bits, index selection bit, colour bits, alpha bits, endpoint p-bits, shared p-bits, index
	 * bits, secondary index bits (the format's table) */
	static const int NS[8] = { 3, 2, 3, 2, 1, 1, 1, 2 }, PB[8] = { 4, 6, 6, 6, 0, 0, 0, 6 }, RB[8] = { 0, 0, 0, 0, 2, 2, 0, 0 }, ISB[8] = { 0, 0, 0, 0, 1, 0, 0, 0 };
	static const int CB[8] = { 4, 6, 5, 7, 5, 7, 7, 5 }, AB[8] = { 0, 0, 0, 0, 6, 8, 7, 5 }, EPB[8] = { 1, 0, 0, 1, 0, 0, 1, 1 }, SPB[8] = { 0, 1, 0, 0, 0, 0, 0, 0 };
	static const int IB[8] = { 3, 3, 2, 2, 2, 2, 4, 2 }, IB2[8] = { 0, 0, 0, 0, 3, 2, 0, 0 };
	BitReader b = { blk, 0 };
	int mode = 0;
	while (mode < 8 && !rd(&b, 1))
		++mode;
	if (mode == 8) /* reserved: the fixture records transparent black */
	{
		memset(out, 0, 64);
		return;
	}
	uint32_t part = rd(&b, PB[mode]), rot = rd(&b, RB[mode]), isb = rd(&b, ISB[mode]);
	int ne = 2 * NS[mode];
	uint32_t ep[6][4];
	for (int ch = 0; ch < 3; ++ch)
		for (int e = 0; e < ne; ++e)
			ep[e][ch] = rd(&b, CB[mode]);
	for (int e = 0; e < ne; ++e)
		ep[e][3] = AB[mode] ? rd(&b, AB[mode]) : 255u;
	int cbits = CB[mode], abits = AB[mode];
	if (EPB[mode] || SPB[mode])
	{
		uint32_t pb[6];
		if (EPB[mode])
			for (int e = 0; e < ne; ++e)
				pb[e] = rd(&b, 1);
		else
		{
			uint32_t s0 = rd(&b, 1), s1 = rd(&b, 1);
			pb[0] = pb[1] = s0, pb[2] = pb[3] = s1;
		}
		for (int e = 0; e < ne; ++e)
			for (int ch = 0; ch < (abits ? 4 : 3); ++ch)
				ep[e][ch] = ep[e][ch] << 1 | pb[e];
		++cbits;
		if (abits)
			++abits;
	}
	for (int e = 0; e < ne; ++e)
	{
		for (int ch = 0; ch < 3; ++ch)
			ep[e][ch] = (ep[e][ch] << (8 - cbits) | ep[e][ch] >> (2 * cbits - 8)) & 255u;
		if (abits)
			ep[e][3] = (ep[e][3] << (8 - abits) | ep[e][3] >> (2 * abits - 8)) & 255u;
	}
	int subset[16], anchor[16] = { 1 };
	for (int t = 0; t < 16; ++t)
		subset[t] = NS[mode] == 1 ? 0 : (NS[mode] == 2 ? P2 : P3)[part][t] - '0';
	if (NS[mode] == 2)
		anchor[A2[part]] = 1;
	if (NS[mode] == 3)
		anchor[A3a[part]] = 1, anchor[A3b[part]] = 1;
	uint32_t idx[16], idx2[16] = { 0 };
	for (int t = 0; t < 16; ++t)
		idx[t] = rd(&b, IB[mode] - anchor[t]);
	if (IB2[mode])
		for (int t = 0; t < 16; ++t)
			idx2[t] = rd(&b, IB2[mode] - (t == 0));
	for (int t = 0; t < 16; ++t)
	{
		const uint32_t* lo = ep[2 * subset[t]];
		const uint32_t* hi = ep[2 * subset[t] + 1];
		uint32_t wc = bptc_weight(IB[mode], idx[t]), wa = wc;
		if (IB2[mode])
		{
			uint32_t w2 = bptc_weight(IB2[mode], idx2[t]);
			if (isb)
				wa = wc, wc = w2;
			else
				wa = w2;
		}
		uint32_t px[4] = { bptc_mix(lo[0], hi[0], wc), bptc_mix(lo[1], hi[1], wc), bptc_mix(lo[2], hi[2], wc), bptc_mix(lo[3], hi[3], wa) };
		if (rot)
		{
			uint32_t s = px[3];
			px[3] = px[rot - 1], px[rot - 1] = s;
		}
		out[t] = px[0] | px[1] << 8 | px[2] << 16 | px[3] << 24;
	}
}

/* format: 1, 2, 3, 7 (NV_FORMAT_*) */
void tr_decode_block(uint32_t format, const uint8_t* blk, uint32_t out[16])
{
	uint32_t a[16];
	if (format == 1)
		tr_colour_block(blk, 0, out);
	else if (format == 2)
	{
		tr_colour_block(blk + 8, 1, out);
		for (int t = 0; t < 16; ++t)
			out[t] = (out[t] & 0xffffffu) | (uint32_t)((blk[t / 2] >> (4 * (t % 2)) & 15u) * 17u) << 24;
	}
	else if (format == 3)
	{
		tr_colour_block(blk + 8, 1, out);
		tr_bc3_alpha(blk, a);
		for (int t = 0; t < 16; ++t)
			out[t] = (out[t] & 0xffffffu) | a[t] << 24;
	}
	else
		tr_bc7_block(blk, out);
}

static uint32_t tr_side(uint32_t s, uint32_t l) { return (s >> l) ? s >> l : 1u; }

/* a whole chain: level l is max(1, w >> l) x max(1, h >> l), its blocks row-major, partial blocks cropped */
void tr_decode_chain(uint32_t format, uint32_t width, uint32_t height, uint32_t levels, const uint8_t* blocks, uint32_t* texels)
{
	uint32_t bs = format == 1 ? 8 : 16;
	for (uint32_t l = 0; l < levels; ++l)
	{
		uint32_t w = tr_side(width, l), h = tr_side(height, l);
		for (uint32_t by = 0; by < (h + 3) / 4; ++by)
			for (uint32_t bx = 0; bx < (w + 3) / 4; ++bx, blocks += bs)
			{
				uint32_t px[16];
				tr_decode_block(format, blocks, px);
				for (uint32_t t = 0; t < 16; ++t)
					if (bx * 4 + t % 4 < w && by * 4 + t / 4 < h)
						texels[(size_t)(by * 4 + t / 4) * w + bx * 4 + t % 4] = px[t];
			}
		texels += (size_t)w * h;
	}
}

/* ---- the sampler (§4.18) */
typedef struct
{
	uint32_t offset, width, height, levels;
} TexDesc;

static uint64_t tr_bad_index; /* loads whose index fell outside the texel buffer (never performed): must stay 0 */
static uint64_t tr_level_hits[16]; /* samples whose level d was l, and whose f was not 0 in [15]: what the tests assert they cover */

static int64_t tr_int(REAL x) { return isfinite(x) ? (int64_t)x : 0; } /* the conversion of a non-finite value is 0 */

static void tr_fetch(const uint32_t* texels, uint64_t texelWords, uint64_t word, REAL c[4])
{
	uint32_t code = 0;
	if (word < texelWords)
		code = texels[word];
	else
		++tr_bad_index;
	for (int k = 0; k < 4; ++k)
		c[k] = (REAL)(code >> (8 * k) & 255u) / K(255.0f);
}

static void tr_axis(REAL x, uint32_t size, int64_t i[2], REAL* alpha)
{
	REAL s = x - floor(x);
	REAL u = s * (REAL)size - K(0.5f);
	REAL i0 = floor(u);
	*alpha = u - i0;
	int64_t n = (int64_t)size, a = tr_int(i0);
	i[0] = ((a % n) + n) % n;
	i[1] = (((a + 1) % n) + n) % n;
}

static REAL tr_blend(REAL a, REAL b, REAL alpha) { return a * (K(1.0f) - alpha) + b * alpha; }

static void tr_bilinear(const uint32_t* texels, uint64_t texelWords, uint64_t base, uint32_t w, uint32_t h, REAL u, REAL v, REAL out[4])
{
	int64_t x[2], y[2];
	REAL ax, ay, c[4][4];
	tr_axis(u, w, x, &ax);
	tr_axis(v, h, y, &ay);
	for (int j = 0; j < 2; ++j)
		for (int i = 0; i < 2; ++i)
			tr_fetch(texels, texelWords, base + (uint64_t)y[j] * w + (uint64_t)x[i], c[2 * j + i]);
	for (int k = 0; k < 4; ++k)
		out[k] = tr_blend(tr_blend(c[0][k], c[1][k], ax), tr_blend(c[2][k], c[3][k], ax), ay);
}

static REAL tr_lambda(const TexDesc* t, const REAL dx[2], const REAL dy[2])
{
	REAL W = (REAL)t->width, H = (REAL)t->height;
	REAL rx = (dx[0] * W) * (dx[0] * W) + (dx[1] * H) * (dx[1] * H), ry = (dy[0] * W) * (dy[0] * W) + (dy[1] * H) * (dy[1] * H);
	REAL lambda = K(0.5f) * log2(rx < ry ? ry : rx);
	REAL top = (REAL)(t->levels - 1);
	if (!(lambda > K(0.0f)))
		lambda = K(0.0f); /* NaN and rho = 0 too */
	return lambda < top ? lambda : top;
}

/* 1: sampled; 0: textures[id] cannot be sampled (id past the table, or the chain not inside texelWords) */
static int tr_sample(const TexDesc* descs, uint32_t count, const uint32_t* texels, uint64_t texelWords, uint32_t id, const REAL uv[2], const REAL dx[2],
                     const REAL dy[2], REAL out[4])
{
	if (id >= count)
		return 0;
	const TexDesc* t = &descs[id];
	if (!t->width || !t->height || !t->levels || t->width > 16384 || t->height > 16384 || t->levels > 15)
		return 0;
	uint64_t base[16], at = t->offset;
	for (uint32_t l = 0; l < t->levels; ++l)
		base[l] = at, at += (uint64_t)tr_side(t->width, l) * tr_side(t->height, l);
	if (at > texelWords)
		return 0;
	REAL lambda = tr_lambda(t, dx, dy);
	REAL fl = floor(lambda), f = lambda - fl;
	uint32_t d = (uint32_t)tr_int(fl), d1 = d + 1 < t->levels ? d + 1 : t->levels - 1;
	++tr_level_hits[d];
	if (f != K(0.0f))
		++tr_level_hits[15];
	REAL lo[4], hi[4];
	tr_bilinear(texels, texelWords, base[d], tr_side(t->width, d), tr_side(t->height, d), uv[0], uv[1], lo);
	tr_bilinear(texels, texelWords, base[d1], tr_side(t->width, d1), tr_side(t->height, d1), uv[0], uv[1], hi);
	for (int k = 0; k < 4; ++k)
		out[k] = tr_blend(lo[k], hi[k], f);
	return 1;
}

/* n samples: uv, dx, dy as float pairs; out n x 4 REAL, ok n bytes */
void tr_sample_many(const TexDesc* descs, uint32_t count, const uint32_t* texels, uint64_t texelWords, uint32_t id, uint32_t n, const float* uv,
                    const float* dx, const float* dy, REAL* out, uint8_t* ok)
{
	for (uint32_t i = 0; i < n; ++i)
	{
		REAL a[2] = { uv[2 * i], uv[2 * i + 1] }, b[2] = { dx[2 * i], dx[2 * i + 1] }, c[2] = { dy[2 * i], dy[2 * i + 1] };
		ok[i] = (uint8_t)tr_sample(descs, count, texels, texelWords, id, a, b, c, out + 4 * (size_t)i);
	}
}

uint64_t tr_bad_indices(void) { return tr_bad_index; }
void tr_hits(uint64_t out[16], int reset)
{
	memcpy(out, tr_level_hits, sizeof(tr_level_hits));
	if (reset)
		memset(tr_level_hits, 0, sizeof(tr_level_hits));
}

/* ---- nv_visibility_attributes_textured: visattr_ref.c's pass with the complete fragment stage.  Outputs as va_attributes; flag 16 = the
 * material names a texture that was NOT sampled; flag 32 = a normal map was sampled; lod: lambda of the last texture sampled (optional) */
/* the texel a slot (0 albedo, 1 normal, 2 specular, 3 emissive) was given, recorded for tests/test_shading_vs_ref.py; always 1 */
static int tr_tap(REAL* taps, uint32_t pixel, int slot, const REAL s[4])
{
	if (taps)
		memcpy(taps + (size_t)pixel * 16 + 4 * slot, s, 4 * sizeof(REAL));
	return 1;
}

static int tr_bary(const Corner c[3], REAL fx, REAL fy, uint32_t W, uint32_t H, REAL l[3])
{
	REAL nx = (fx / (REAL)W) * K(2.0f) - K(1.0f), ny = K(1.0f) - (fy / (REAL)H) * K(2.0f), dx[3], dy[3], b[3];
	for (int k = 0; k < 3; ++k)
		dx[k] = c[k].clip[0] - nx * c[k].clip[3], dy[k] = c[k].clip[1] - ny * c[k].clip[3];
	b[0] = dx[1] * dy[2] - dy[1] * dx[2];
	b[1] = dx[2] * dy[0] - dy[2] * dx[0];
	b[2] = dx[0] * dy[1] - dy[0] * dx[1];
	REAL s = (b[0] + b[1]) + b[2];
	for (int k = 0; k < 3; ++k)
		l[k] = b[k] / s;
	if (s == K(0.0f) || !isfinite(l[0]) || !isfinite(l[1]) || !isfinite(l[2]))
	{
		l[0] = K(1.0f), l[1] = K(0.0f), l[2] = K(0.0f);
		return 1;
	}
	return 0;
}

static void tr_attributes_impl(const Globals* g, const VisRecord* records, uint32_t W, uint32_t H, const Draw* draws, uint32_t drawCount, const Meshlet* meshlets,
                   uint32_t meshletCount, const uint32_t* data, uint32_t dataWords, const Vertex* vertices, uint32_t vertexCount,
                   const Material* materials, uint32_t materialCount, const TexDesc* descs, uint32_t textureCount, const uint32_t* texels,
                   uint64_t texelWords, REAL* vals, uint32_t* ids, uint32_t* gb0, uint32_t* gb1, uint64_t* totals4, uint8_t* flags, REAL* chan,
                   REAL* taps)
{
	for (uint32_t i = 0; i < W * H; ++i)
	{
		const VisRecord* r = &records[i];
		REAL out[14] = { 0 }, ch[8] = { 0 };
		uint32_t id[2] = { 0xffffffffu, 0 }, g0 = 0, g1 = 0;
		uint8_t fl = 0;
		uint64_t vi[3];
		int named = r->drawId != 0xffffffffu;
		int ok = named && va_triangle(r, draws, drawCount, meshlets, meshletCount, data, dataWords, vertexCount, materials, materialCount, vi);
		if (named && !ok)
			fl |= 2;
		if (ok)
		{
			const Draw* d = &draws[r->drawId];
			Corner c[3];
			for (int k = 0; k < 3; ++k)
				va_vertex(g, d, &vertices[vi[k]], &c[k]);
			fl |= 1;
			uint32_t py = i / W, px = i - py * W;
			REAL fx = (REAL)px + K(0.5f), fy = (REAL)py + K(0.5f), l[3], lx[3], ly[3];
			if (tr_bary(c, fx, fy, W, H, l))
				fl |= 4;
			REAL uv[2], n[3], t[4], w[3], dx[2] = { 0, 0 }, dy[2] = { 0, 0 };
			for (int k = 0; k < 2; ++k)
				uv[k] = va_mix(l, c[0].uv[k], c[1].uv[k], c[2].uv[k]);
			for (int k = 0; k < 3; ++k)
				n[k] = va_mix(l, c[0].n[k], c[1].n[k], c[2].n[k]);
			for (int k = 0; k < 4; ++k)
				t[k] = va_mix(l, c[0].t[k], c[1].t[k], c[2].t[k]);
			for (int k = 0; k < 3; ++k)
				w[k] = va_mix(l, c[0].w[k], c[1].w[k], c[2].w[k]);
			/* the derivatives: the same triangle at the centres of (px + 1, py) and (px, py + 1); a degenerate neighbour gives 0 */
			if (!tr_bary(c, (REAL)(px + 1) + K(0.5f), fy, W, H, lx))
				for (int k = 0; k < 2; ++k)
					dx[k] = va_mix(lx, c[0].uv[k], c[1].uv[k], c[2].uv[k]) - uv[k];
			if (!tr_bary(c, fx, (REAL)(py + 1) + K(0.5f), W, H, ly))
				for (int k = 0; k < 2; ++k)
					dy[k] = va_mix(ly, c[0].uv[k], c[1].uv[k], c[2].uv[k]) - uv[k];
			out[0] = uv[0], out[1] = uv[1], out[2] = l[1], out[3] = l[2];
			out[4] = n[0], out[5] = n[1], out[6] = n[2];
			out[7] = t[0], out[8] = t[1], out[9] = t[2], out[10] = t[3];
			out[11] = w[0], out[12] = w[1], out[13] = w[2];
			id[0] = r->drawId, id[1] = d->materialIndex;
			/* src/shaders/mesh.frag.glsl:57-89 */
			const Material* m = &materials[d->materialIndex];
			REAL albedo[4], nmap[3] = { K(0.0f), K(0.0f), K(1.0f) }, gloss = (REAL)m->specularFactor[3], em[3], s[4];
			for (int k = 0; k < 4; ++k)
				albedo[k] = (REAL)m->diffuseFactor[k];
			for (int k = 0; k < 3; ++k)
				em[k] = (REAL)m->emissiveFactor[k];
			if (m->albedoTexture > 0)
			{
				if (tr_sample(descs, textureCount, texels, texelWords, m->albedoTexture, uv, dx, dy, s) && tr_tap(taps, i, 0, s))
				{
					for (int k = 0; k < 3; ++k)
						albedo[k] = albedo[k] * pow(s[k], K(2.2f));
					albedo[3] = albedo[3] * s[3];
				}
				else
					fl |= 16;
			}
			if (m->normalTexture > 0)
			{
				if (tr_sample(descs, textureCount, texels, texelWords, m->normalTexture, uv, dx, dy, s) && tr_tap(taps, i, 1, s))
				{
					for (int k = 0; k < 3; ++k)
						nmap[k] = s[k] * K(2.0f) - K(1.0f);
					fl |= 32;
				}
				else
					fl |= 16;
			}
			if (m->specularTexture > 0)
			{
				if (tr_sample(descs, textureCount, texels, texelWords, m->specularTexture, uv, dx, dy, s) && tr_tap(taps, i, 2, s))
					gloss = gloss * s[3];
				else
					fl |= 16;
			}
			if (m->emissiveTexture > 0)
			{
				if (tr_sample(descs, textureCount, texels, texelWords, m->emissiveTexture, uv, dx, dy, s) && tr_tap(taps, i, 3, s))
					for (int k = 0; k < 3; ++k)
						em[k] = em[k] * pow(s[k], K(2.2f));
				else
					fl |= 16;
			}
			REAL noise = va_fract(K(52.9829189f) * va_fract(fx * K(0.06711056f) + fy * K(0.00583715f)));
			REAL deband = noise * K(2.0f) - K(1.0f);
			REAL bt[3] = { n[1] * t[2] - t[1] * n[2], n[2] * t[0] - t[2] * n[0], n[0] * t[1] - t[0] * n[1] }, nrm[3];
			for (int k = 0; k < 3; ++k)
			{
				REAL bitangent = bt[k] * t[3];
				nrm[k] = (nmap[0] * t[k] + nmap[1] * bitangent) + nmap[2] * n[k];
			}
			va_normalize(nrm);
			REAL emissivef = ((em[0] * K(0.3f) + em[1] * K(0.6f)) + em[2] * K(0.1f)) / (((albedo[0] * K(0.3f) + albedo[1] * K(0.6f)) + albedo[2] * K(0.1f)) + K(1e-3f));
			for (int k = 0; k < 3; ++k)
				ch[k] = va_tosrgb(albedo[k]);
			ch[3] = log2(K(1.0f) + emissivef) / K(5.0f);
			g0 = va_unorm(ch[0], K(255.0f)) | va_unorm(ch[1], K(255.0f)) << 8 | va_unorm(ch[2], K(255.0f)) << 16 | va_unorm(ch[3], K(255.0f)) << 24;
			REAL oct[2];
			va_encode_oct(nrm, oct);
			REAL ex = oct[0], ey = oct[1];
			REAL band = deband * (K(0.5f) / K(1023.0f));
			ch[4] = (ex * K(0.5f) + K(0.5f)) + band;
			ch[5] = (ey * K(0.5f) + K(0.5f)) + band;
			ch[6] = gloss;
			ch[7] = K(0.0f);
			g1 = va_unorm(ch[4], K(1023.0f)) | va_unorm(ch[5], K(1023.0f)) << 10 | va_unorm(ch[6], K(1023.0f)) << 20 | va_unorm(ch[7], K(3.0f)) << 30;
		}
		if (totals4)
		{
			totals4[0] += fl & 1 ? 1 : 0;
			totals4[1] += fl & 2 ? 1 : 0;
			totals4[2] += fl & 4 ? 1 : 0;
			totals4[3] += fl & 16 ? 1 : 0;
		}
		if (vals)
			memcpy(vals + (size_t)i * 14, out, sizeof(out));
		if (ids)
			ids[2 * (size_t)i] = id[0], ids[2 * (size_t)i + 1] = id[1];
		if (gb0)
			gb0[i] = g0;
		if (gb1)
			gb1[i] = g1;
		if (flags)
			flags[i] = fl;
		if (chan)
			memcpy(chan + (size_t)i * 8, ch, sizeof(ch));
	}
}

void tr_attributes(const Globals* g, const VisRecord* records, uint32_t W, uint32_t H, const Draw* draws, uint32_t drawCount, const Meshlet* meshlets,
                   uint32_t meshletCount, const uint32_t* data, uint32_t dataWords, const Vertex* vertices, uint32_t vertexCount,
                   const Material* materials, uint32_t materialCount, const TexDesc* descs, uint32_t textureCount, const uint32_t* texels,
                   uint64_t texelWords, REAL* vals, uint32_t* ids, uint32_t* gb0, uint32_t* gb1, uint64_t* totals4, uint8_t* flags, REAL* chan)
{
	tr_attributes_impl(g, records, W, H, draws, drawCount, meshlets, meshletCount, data, dataWords, vertices, vertexCount, materials, materialCount, descs,
	                   textureCount, texels, texelWords, vals, ids, gb0, gb1, totals4, flags, chan, 0);
}

/* tr_attributes, and per pixel the four texels tr_sample returned (taps: W * H * 16 REAL, slots albedo / normal / specular / emissive; a slot
 * that was not sampled keeps what the caller put there): a thin wrapper for tests/test_shading_vs_ref.py */
void tr_attributes_taps(const Globals* g, const VisRecord* records, uint32_t W, uint32_t H, const Draw* draws, uint32_t drawCount, const Meshlet* meshlets,
                        uint32_t meshletCount, const uint32_t* data, uint32_t dataWords, const Vertex* vertices, uint32_t vertexCount,
                        const Material* materials, uint32_t materialCount, const TexDesc* descs, uint32_t textureCount, const uint32_t* texels,
                        uint64_t texelWords, REAL* vals, uint32_t* ids, uint32_t* gb0, uint32_t* gb1, uint64_t* totals4, uint8_t* flags, REAL* chan,
                        REAL* taps)
{
	tr_attributes_impl(g, records, W, H, draws, drawCount, meshlets, meshletCount, data, dataWords, vertices, vertexCount, materials, materialCount, descs,
	                   textureCount, texels, texelWords, vals, ids, gb0, gb1, totals4, flags, chan, taps);
}
