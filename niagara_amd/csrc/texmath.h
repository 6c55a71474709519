// texmath.h — the material textures of DESIGN.md §4.18 in ONE text that compiles for the device (hipcc) and for the host (g++): the decode of
// one texel of a BC1 / BC2 / BC3 / BC7 block to RGBA8, the UNORM fetch, and `textureSampler` (niagara.cpp:627, resources.cpp:294-310: LINEAR min
// and mag, mipmap LINEAR, REPEAT, lod 0..16) as a software sampler over a decoded RGBA8 mip chain.  texdecode.hip, visattr_tex.hip and the
// host entry points of texload.cpp run the same text; tests/texture_ref.c restates it independently.  The same sampler also runs over a texel
// SOURCE, and TxBlockSource is the source that decodes each tap from its BC block (block-resident sets).
//
// Build with -ffp-contract=off: every fp32 operation of the sampler is one IEEE operation in the order written (log2 excepted, §4.18).
//
// Decode.  The result is DEFINED by the bytes niagara's CPU decoder gives (tests/golden/textures/bc_blocks.npz).  Everything is addressed by bit
// position inside the 128-bit block — a texel's value is a pure function of (block, texel) — so no stream state and no array lives anywhere:
// the per-mode constants are nibbles of 32-bit literals, the weights bytes of 64-bit literals, and the partition / anchor tables constant
// data (never a private array).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define NV_TX __host__ __device__ inline __attribute__((always_inline))
#define NV_TXM __host__ __device__ inline __attribute__((always_inline)) // (a member function)
#else
#define NV_TX static inline
#define NV_TXM inline
#endif
// constant data of both sides: the host reads the variable itself, device code gets a copy in the constant address space (a constexpr
// variable is usable from device code as it stands; a __constant__ one would read as zeros on the host)
#define NV_TX_TABLE static constexpr

namespace nv
{

// formats of NvDdsInfo.format; the first four decode, the last three parse and are refused by the set
constexpr uint32_t TX_BC1 = 1u, TX_BC2 = 2u, TX_BC3 = 3u, TX_BC7 = 7u, TX_BC4 = 4u, TX_BC5 = 5u, TX_BC6H = 6u;
constexpr uint32_t TX_MAX_SIDE = 16384u, TX_MAX_LEVELS = 15u; // 16384 = 2^14: levels 0..14

NV_TX bool tx_decodable(uint32_t format) { return format == TX_BC1 || format == TX_BC2 || format == TX_BC3 || format == TX_BC7; }
NV_TX uint32_t tx_block_bytes(uint32_t format) { return format == TX_BC1 || format == TX_BC4 ? 8u : 16u; }

#ifndef NV_TX_SAMPLER_ONLY
// ---- BC7 (BPTC) tables.  Subset of texel t: 2 subsets (P2 >> t) & 1, 3 subsets (P3 >> 2 t) & 3; anchors (the texels whose index has one
// bit less; subset 0's is texel 0): second subset of 2 in bits 0-3, second and third subset of 3 in bits 4-7 and 8-11.
NV_TX_TABLE uint16_t TX_P2[64] = {
	0xccccu, 0x8888u, 0xeeeeu, 0xecc8u, 0xc880u, 0xfeecu, 0xfec8u, 0xec80u, 0xc800u, 0xffecu, 0xfe80u, 0xe800u, 0xffe8u, 0xff00u, 0xfff0u, 0xf000u,
	0xf710u, 0x008eu, 0x7100u, 0x08ceu, 0x008cu, 0x7310u, 0x3100u, 0x8cceu, 0x088cu, 0x3110u, 0x6666u, 0x366cu, 0x17e8u, 0x0ff0u, 0x718eu, 0x399cu,
	0xaaaau, 0xf0f0u, 0x5a5au, 0x33ccu, 0x3c3cu, 0x55aau, 0x9696u, 0xa55au, 0x73ceu, 0x13c8u, 0x324cu, 0x3bdcu, 0x6996u, 0xc33cu, 0x9966u, 0x0660u,
	0x0272u, 0x04e4u, 0x4e40u, 0x2720u, 0xc936u, 0x936cu, 0x39c6u, 0x639cu, 0x9336u, 0x9cc6u, 0x817eu, 0xe718u, 0xccf0u, 0x0fccu, 0x7744u, 0xee22u,
};
NV_TX_TABLE uint32_t TX_P3[64] = {
	0xaa685050u, 0x6a5a5040u, 0x5a5a4200u, 0x5450a0a8u, 0xa5a50000u, 0xa0a05050u, 0x5555a0a0u, 0x5a5a5050u,
	0xaa550000u, 0xaa555500u, 0xaaaa5500u, 0x90909090u, 0x94949494u, 0xa4a4a4a4u, 0xa9a59450u, 0x2a0a4250u,
	0xa5945040u, 0x0a425054u, 0xa5a5a500u, 0x55a0a0a0u, 0xa8a85454u, 0x6a6a4040u, 0xa4a45000u, 0x1a1a0500u,
	0x0050a4a4u, 0xaaa59090u, 0x14696914u, 0x69691400u, 0xa08585a0u, 0xaa821414u, 0x50a4a450u, 0x6a5a0200u,
	0xa9a58000u, 0x5090a0a8u, 0xa8a09050u, 0x24242424u, 0x00aa5500u, 0x24924924u, 0x24499224u, 0x50a50a50u,
	0x500aa550u, 0xaaaa4444u, 0x66660000u, 0xa5a0a5a0u, 0x50a050a0u, 0x69286928u, 0x44aaaa44u, 0x66666600u,
	0xaa444444u, 0x54a854a8u, 0x95809580u, 0x96969600u, 0xa85454a8u, 0x80959580u, 0xaa141414u, 0x96960000u,
	0xaaaa1414u, 0xa05050a0u, 0xa0a5a5a0u, 0x96000000u, 0x40804080u, 0xa9a8a9a8u, 0xaaaaaa44u, 0x2a4a5254u,
};
NV_TX_TABLE uint16_t TX_ANCHOR[64] = {
	0xf3fu, 0x83fu, 0x8ffu, 0x3ffu, 0xf8fu, 0xf3fu, 0x3ffu, 0x8ffu, 0xf8fu, 0xf8fu, 0xf6fu, 0xf6fu, 0xf6fu, 0xf5fu, 0xf3fu, 0x83fu,
	0xf3fu, 0x832u, 0xf88u, 0x3f2u, 0xf32u, 0x838u, 0xf68u, 0x8afu, 0x352u, 0xf88u, 0x682u, 0xa62u, 0xf88u, 0xf58u, 0xaf2u, 0x8f2u,
	0xf8fu, 0x3ffu, 0xf36u, 0xa58u, 0xa62u, 0x8a8u, 0x98fu, 0xaffu, 0x6f2u, 0xf38u, 0x8f2u, 0xf52u, 0x3f2u, 0x6ffu, 0x6ffu, 0x8f6u,
	0xf36u, 0x3f2u, 0xf56u, 0xf58u, 0xf5fu, 0xf8fu, 0xf52u, 0xfa2u, 0xf5fu, 0xfafu, 0xf8fu, 0xfdfu, 0x3ffu, 0xfc2u, 0xf32u, 0x83fu,
};

// n <= 8 bits of the 128-bit block {lo, hi} from bit `pos` (pos + n <= 128 by the layout sums below; the masks keep every shift defined)
NV_TX uint32_t tx_bits(uint64_t lo, uint64_t hi, uint32_t pos, uint32_t n)
{
	const uint32_t p = pos & 63u;
	const uint64_t v = (pos & 64u) ? hi >> p : (p ? lo >> p | hi << (64u - p) : lo);
	return (uint32_t)v & ((1u << n) - 1u);
}

NV_TX uint32_t tx_nibble(uint32_t packed, uint32_t i) { return packed >> (i * 4u) & 15u; }

// round(x / d) for d > 0, halves up (no interpolant of the formats lands on a half except 255 x / 62 and 255 x / 126, which round up in the fixture)
NV_TX uint32_t tx_div_round(uint32_t x, uint32_t d) { return (2u * x + d) / (2u * d); }

// BC1 colour block `b` (8 bytes), texel t = y * 4 + x: RGBA8 with R in the low byte.  opaque: the BC2 / BC3 colour block (four colours always).
// The fixture's bytes are those of this rule: the 5 / 6-bit endpoints are interpolated with integer weights (w0, w1) of sum k = 1 (an
// endpoint), 3 (thirds) or 2 (the half of the three-colour mode) BEFORE the expansion to 8 bits, and the sum is scaled by 255 / (31 k),
// 255 / (63 k) for green, rounded to nearest.  k is a compile-time constant on every path: the divisions become multiplications.
NV_TX uint32_t tx_bc1_texel(uint64_t b, uint32_t t, bool opaque)
{
	const uint32_t c0 = (uint32_t)b & 0xffffu, c1 = (uint32_t)(b >> 16) & 0xffffu;
	const uint32_t idx = (uint32_t)(b >> (32u + 2u * t)) & 3u;
	const uint32_t r0 = c0 >> 11, g0 = c0 >> 5 & 63u, b0 = c0 & 31u, r1 = c1 >> 11, g1 = c1 >> 5 & 63u, b1 = c1 & 31u;
	uint32_t r, g, bl;
	if (idx < 2u)
	{
		const uint32_t rr = idx ? r1 : r0, gg = idx ? g1 : g0, bb = idx ? b1 : b0;
		r = tx_div_round(rr * 255u, 31u), g = tx_div_round(gg * 255u, 63u), bl = tx_div_round(bb * 255u, 31u);
	}
	else if (c0 > c1 || opaque)
	{
		const uint32_t w0 = idx == 2u ? 2u : 1u, w1 = 3u - w0;
		r = tx_div_round((w0 * r0 + w1 * r1) * 255u, 93u), g = tx_div_round((w0 * g0 + w1 * g1) * 255u, 189u), bl = tx_div_round((w0 * b0 + w1 * b1) * 255u, 93u);
	}
	else if (idx == 2u)
		r = tx_div_round((r0 + r1) * 255u, 62u), g = tx_div_round((g0 + g1) * 255u, 126u), bl = tx_div_round((b0 + b1) * 255u, 62u);
	else
		return 0u; // transparent black
	return 0xff000000u | bl << 16 | g << 8 | r;
}

// BC3 alpha block
NV_TX uint32_t tx_bc3_alpha(uint64_t b, uint32_t t)
{
	const uint32_t a0 = (uint32_t)b & 255u, a1 = (uint32_t)(b >> 8) & 255u;
	const uint32_t idx = (uint32_t)(b >> (16u + 3u * t)) & 7u;
	if (idx < 2u)
		return idx ? a1 : a0;
	if (a0 > a1)
		return ((8u - idx) * a0 + (idx - 1u) * a1) / 7u;
	if (idx < 6u)
		return ((6u - idx) * a0 + (idx - 1u) * a1) / 5u;
	return idx == 6u ? 0u : 255u;
}

// BC7 interpolation weight of an index of `bits` (2, 3, 4) bits: round(64 i / (2^bits - 1))
NV_TX uint32_t tx_bc7_weight(uint32_t bits, uint32_t i)
{
	const uint64_t w2 = 0x402b1500ull, w3 = 0x40372e251b120900ull, w4lo = 0x1e1a15110d090400ull, w4hi = 0x403c37332f2b2622ull;
	const uint64_t w = bits == 2u ? w2 : bits == 3u ? w3 : (i & 8u) ? w4hi : w4lo;
	return (uint32_t)(w >> ((i & 7u) * 8u)) & 255u;
}

NV_TX uint32_t tx_bc7_mix(uint32_t a, uint32_t b, uint32_t w) { return (a * (64u - w) + b * w + 32u) >> 6; }

// an endpoint channel: `bits` raw bits at `pos`, the p-bit appended below them, expanded to 8 bits by replicating the top bits
NV_TX uint32_t tx_bc7_endpoint(uint64_t lo, uint64_t hi, uint32_t pos, uint32_t bits, bool hasP, uint32_t p)
{
	const uint32_t raw = tx_bits(lo, hi, pos, bits), n = bits + (hasP ? 1u : 0u);
	const uint32_t v = (hasP ? raw << 1 | p : raw) << (8u - n);
	return v | v >> n;
}

// One texel of a BC7 block.  Layout, from bit 0: mode + 1 bits (mode = number of leading zero bits; none set in byte 0: RESERVED, decodes to
// 0), partition, rotation, index selection, colour endpoints channel-major (R of every endpoint, G, B), alpha endpoints, p-bits, the primary
// indices (texel-major; an anchor texel has one bit less) and the secondary indices (modes 4, 5; texel 0 is the anchor).  Every mode sums to 128.
NV_TX uint32_t tx_bc7_texel(uint64_t lo, uint64_t hi, uint32_t t)
{
	const uint32_t byte0 = (uint32_t)lo & 255u;
	if (byte0 == 0u)
		return 0u;
	const uint32_t mode = (uint32_t)__builtin_ctz(byte0);
	//                                   mode:  76543210
	const uint32_t ns = tx_nibble(0x21112323u, mode);  // subsets
	const uint32_t pb = tx_nibble(0x60006664u, mode);  // partition bits
	const uint32_t rb = tx_nibble(0x00220000u, mode);  // rotation bits
	const uint32_t cb = tx_nibble(0x57757564u, mode);  // colour endpoint bits
	const uint32_t ab = tx_nibble(0x57860000u, mode);  // alpha endpoint bits
	const uint32_t ib = tx_nibble(0x24222233u, mode);  // primary index bits
	const uint32_t ib2 = tx_nibble(0x00230000u, mode); // secondary index bits
	const bool uniqueP = mode == 0u || mode == 3u || mode == 6u || mode == 7u, sharedP = mode == 1u;
	const uint32_t ne = ns * 2u;

	uint32_t pos = mode + 1u;
	const uint32_t partition = tx_bits(lo, hi, pos, pb);
	pos += pb;
	const uint32_t rotation = tx_bits(lo, hi, pos, rb);
	pos += rb;
	const uint32_t isb = mode == 4u ? tx_bits(lo, hi, pos, 1u) : 0u;
	pos += mode == 4u ? 1u : 0u;
	const uint32_t colourBase = pos, alphaBase = colourBase + 3u * ne * cb, pBase = alphaBase + ne * ab;
	const uint32_t indexBase = pBase + (uniqueP ? ne : sharedP ? 2u : 0u);

	// the texel's subset and the anchors of its partition
	const uint32_t anchors = TX_ANCHOR[partition];
	const uint32_t subset = ns == 1u ? 0u : ns == 2u ? (uint32_t)TX_P2[partition] >> t & 1u : TX_P3[partition] >> (2u * t) & 3u;
	const uint32_t a1 = ns == 1u ? 16u : ns == 2u ? anchors & 15u : anchors >> 4 & 15u; // 16: no such anchor
	const uint32_t a2 = ns == 3u ? anchors >> 8 & 15u : 16u;
	const bool anchor = t == 0u || t == a1 || t == a2;
	const uint32_t index = tx_bits(lo, hi, indexBase + t * ib - (t > 0u ? 1u : 0u) - (t > a1 ? 1u : 0u) - (t > a2 ? 1u : 0u), anchor ? ib - 1u : ib);
	const uint32_t index2Base = indexBase + 16u * ib - ns;
	const uint32_t index2 = ib2 ? tx_bits(lo, hi, index2Base + t * ib2 - (t > 0u ? 1u : 0u), t == 0u ? ib2 - 1u : ib2) : 0u;

	// the subset's two endpoints: raw bits, p-bit, expansion to 8 bits by replicating the top bits
	const uint32_t e0 = subset * 2u, e1 = e0 + 1u;
	const uint32_t p0 = uniqueP ? tx_bits(lo, hi, pBase + e0, 1u) : sharedP ? tx_bits(lo, hi, pBase + subset, 1u) : 0u;
	const uint32_t p1 = uniqueP ? tx_bits(lo, hi, pBase + e1, 1u) : p0;
	const bool hasP = uniqueP || sharedP;
	const uint32_t r0 = tx_bc7_endpoint(lo, hi, colourBase + e0 * cb, cb, hasP, p0), r1 = tx_bc7_endpoint(lo, hi, colourBase + e1 * cb, cb, hasP, p1);
	const uint32_t g0 = tx_bc7_endpoint(lo, hi, colourBase + (ne + e0) * cb, cb, hasP, p0), g1 = tx_bc7_endpoint(lo, hi, colourBase + (ne + e1) * cb, cb, hasP, p1);
	const uint32_t b0 = tx_bc7_endpoint(lo, hi, colourBase + (2u * ne + e0) * cb, cb, hasP, p0), b1 = tx_bc7_endpoint(lo, hi, colourBase + (2u * ne + e1) * cb, cb, hasP, p1);
	const uint32_t al0 = ab ? tx_bc7_endpoint(lo, hi, alphaBase + e0 * ab, ab, hasP, p0) : 255u, al1 = ab ? tx_bc7_endpoint(lo, hi, alphaBase + e1 * ab, ab, hasP, p1) : 255u;

	// colour takes the secondary index when the selection bit is set, alpha then the primary one
	const uint32_t wp = tx_bc7_weight(ib, index), ws = ib2 ? tx_bc7_weight(ib2, index2) : wp;
	const uint32_t wc = isb ? ws : wp, wa = ib2 ? (isb ? wp : ws) : wp;
	uint32_t r = tx_bc7_mix(r0, r1, wc), g = tx_bc7_mix(g0, g1, wc), b = tx_bc7_mix(b0, b1, wc), a = tx_bc7_mix(al0, al1, wa);
	if (rotation == 1u)
	{
		const uint32_t s = a;
		a = r, r = s;
	}
	else if (rotation == 2u)
	{
		const uint32_t s = a;
		a = g, g = s;
	}
	else if (rotation == 3u)
	{
		const uint32_t s = a;
		a = b, b = s;
	}
	return (a & 255u) << 24 | (b & 255u) << 16 | (g & 255u) << 8 | (r & 255u);
}

// texel t of a block of a decodable format; {lo, hi} = its 16 bytes (BC1: lo only)
NV_TX uint32_t tx_decode_texel(uint32_t format, uint64_t lo, uint64_t hi, uint32_t t)
{
	if (format == TX_BC1)
		return tx_bc1_texel(lo, t, false);
	if (format == TX_BC2)
		return (tx_bc1_texel(hi, t, true) & 0x00ffffffu) | ((uint32_t)(lo >> (4u * t)) & 15u) * 17u << 24;
	if (format == TX_BC3)
		return (tx_bc1_texel(hi, t, true) & 0x00ffffffu) | tx_bc3_alpha(lo, t) << 24;
	return tx_bc7_texel(lo, hi, t);
}

#endif // NV_TX_SAMPLER_ONLY

// ---- the mip chain.  Level l is max(1, w >> l) x max(1, h >> l); compressed, its partial blocks round up (getImageSizeBC, textures.cpp:129)
NV_TX uint32_t tx_level_side(uint32_t side, uint32_t level) { return (side >> level) ? side >> level : 1u; }

// the descriptor of one decoded texture (== NvTextureDesc): its RGBA8 levels lie one after the other from word `offset` of the texel buffer
struct TxDesc
{
	uint32_t offset, width, height, levels;
};

// words of the first `levels` levels
NV_TX uint64_t tx_chain_words(uint32_t width, uint32_t height, uint32_t levels)
{
	uint64_t n = 0;
	for (uint32_t l = 0; l < levels; ++l)
		n += (uint64_t)tx_level_side(width, l) * tx_level_side(height, l);
	return n;
}

// the check in front of every texel load: a sane shape and the whole chain inside the caller's `texelWords`.  levels <= 15 bounds every loop.
NV_TX bool tx_desc_ok(const TxDesc& d, uint64_t texelWords)
{
	if (d.width == 0u || d.height == 0u || d.width > TX_MAX_SIDE || d.height > TX_MAX_SIDE || d.levels == 0u || d.levels > TX_MAX_LEVELS)
		return false;
	return (uint64_t)d.offset + tx_chain_words(d.width, d.height, d.levels) <= texelWords;
}

// ---- the sampler
struct TxF4
{
	float x, y, z, w;
};

NV_TX float tx_max(float a, float b) { return a < b ? b : a; }

// the integer conversion of the sampler: a non-finite value converts to 0 (§4.18); a finite one is in int range by construction (|x| <= 16384.5)
NV_TX int32_t tx_to_int(float x) { return __builtin_fabsf(x) < __builtin_inff() ? (int32_t)x : 0; }

// UNORM fetch: code / 255, one division
NV_TX TxF4 tx_fetch(const uint32_t* texels, uint64_t word)
{
	const uint32_t c = texels[word];
	return TxF4{ (float)(c & 255u) / 255.0f, (float)(c >> 8 & 255u) / 255.0f, (float)(c >> 16 & 255u) / 255.0f, (float)(c >> 24) / 255.0f };
}

// REPEAT + LINEAR on one axis of `size` texels: i0, i1 in [0, size) for EVERY bit pattern of x, alpha = the weight of i1
NV_TX void tx_axis(float x, uint32_t size, uint32_t& i0, uint32_t& i1, float& alpha)
{
	const float s = x - __builtin_floorf(x);
	const float u = s * (float)size - 0.5f;
	const float fl = __builtin_floorf(u);
	alpha = u - fl;
	const int32_t i = tx_to_int(fl); // -1 .. size - 1 (s = 1 is reached by a tiny negative x)
	const int32_t m0 = i < 0 ? i + (int32_t)size : i, m1 = i + 1 >= (int32_t)size ? i + 1 - (int32_t)size : i + 1;
	i0 = (uint32_t)m0 < size ? (uint32_t)m0 : 0u; // (the modulo already lands in range; the guards make that independent of the float reasoning)
	i1 = (uint32_t)m1 < size ? (uint32_t)m1 : 0u;
}

NV_TX float tx_lerp(float a, float b, float alpha) { return a * (1.0f - alpha) + b * alpha; }
NV_TX TxF4 tx_lerp(TxF4 a, TxF4 b, float alpha)
{
	return TxF4{ tx_lerp(a.x, b.x, alpha), tx_lerp(a.y, b.y, alpha), tx_lerp(a.z, b.z, alpha), tx_lerp(a.w, b.w, alpha) };
}

// bilinear on one level (w x h texels from word `base`): x first, then y
NV_TX TxF4 tx_bilinear(const uint32_t* texels, uint64_t base, uint32_t w, uint32_t h, float u, float v)
{
	uint32_t x0, x1, y0, y1;
	float ax, ay;
	tx_axis(u, w, x0, x1, ax);
	tx_axis(v, h, y0, y1, ay);
	const uint64_t r0 = base + (uint64_t)y0 * w, r1 = base + (uint64_t)y1 * w;
	const TxF4 top = tx_lerp(tx_fetch(texels, r0 + x0), tx_fetch(texels, r0 + x1), ax);
	const TxF4 bottom = tx_lerp(tx_fetch(texels, r1 + x0), tx_fetch(texels, r1 + x1), ax);
	return tx_lerp(top, bottom, ay);
}

// the isotropic level of detail (Vulkan 1.3 §16.5.7 without anisotropy) clamped to [0, levels - 1]; NaN -> 0.  W, H: level 0's size
NV_TX float tx_lambda(float dudx, float dvdx, float dudy, float dvdy, uint32_t W, uint32_t H, uint32_t levels)
{
	const float ax = dudx * (float)W, bx = dvdx * (float)H, ay = dudy * (float)W, by = dvdy * (float)H;
	const float rx = ax * ax + bx * bx, ry = ay * ay + by * by;
	const float lambda = 0.5f * __builtin_log2f(tx_max(rx, ry));
	const float top = (float)(levels - 1u);
	const float l0 = lambda > 0.0f ? lambda : 0.0f; // NaN, -inf (rho = 0) -> 0
	return l0 < top ? l0 : top;
}

// trilinear at level of detail `lod` of a texture tx_desc_ok accepted: lod is clamped to [0, levels - 1] here too (NaN -> 0), so the
// property "every index in range" needs nothing of the caller; levels d = floor(lambda) and min(d + 1, levels - 1), blended with
// f = lambda - d; a weight of exactly 0 still multiplies (8 taps always)
NV_TX TxF4 tx_sample_lod(const uint32_t* texels, const TxDesc& t, float u, float v, float lod)
{
	const float top = (float)(t.levels - 1u);
	const float low = lod > 0.0f ? lod : 0.0f;
	const float lambda = low < top ? low : top;
	const float fl = __builtin_floorf(lambda);
	const float f = lambda - fl;
	uint32_t d = (uint32_t)tx_to_int(fl);
	d = d < t.levels ? d : t.levels - 1u;
	const uint32_t d1 = d + 1u < t.levels ? d + 1u : t.levels - 1u;
	uint64_t base = t.offset, b0 = t.offset, b1 = t.offset;
	for (uint32_t l = 0; l < t.levels; ++l)
	{
		b0 = l == d ? base : b0;
		b1 = l == d1 ? base : b1;
		base += (uint64_t)tx_level_side(t.width, l) * tx_level_side(t.height, l);
	}
	const TxF4 lo = tx_bilinear(texels, b0, tx_level_side(t.width, d), tx_level_side(t.height, d), u, v);
	const TxF4 hi = tx_bilinear(texels, b1, tx_level_side(t.width, d1), tx_level_side(t.height, d1), u, v);
	return tx_lerp(lo, hi, f);
}

// texture(sampler2D, uv) with explicit derivatives
NV_TX TxF4 tx_sample(const uint32_t* texels, const TxDesc& t, float u, float v, float dudx, float dvdx, float dudy, float dvdy)
{
	return tx_sample_lod(texels, t, u, v, tx_lambda(dudx, dvdx, dudy, dvdy, t.width, t.height, t.levels));
}

// textureLod(sampler2D, uv, 0) (shadow.comp.glsl:117 reads its .w): the same sampler at lambda = 0
NV_TX TxF4 tx_sample_lod0(const uint32_t* texels, const TxDesc& t, float u, float v) { return tx_sample_lod(texels, t, u, v, 0.0f); }

// ---- the same sampler over a texel SOURCE.  The functions above are the decoded source and keep their text; these overloads
// run the same operations in the same order on the RGBA8 codes a source hands out, so a source that returns the codes of the decoded chain gives
// the decoded sampler's bits.  SRC has width, height, levels (accepted by its own *_desc_ok), level_bases(d, d1, b0, b1) — where levels d and
// d1 start, in the source's own unit — and quad(base, w, h, x0, x1, y0, y1, c00, c01, c10, c11): the codes of the four taps of one level.
NV_TX TxF4 tx_unorm(uint32_t c)
{
	return TxF4{ (float)(c & 255u) / 255.0f, (float)(c >> 8 & 255u) / 255.0f, (float)(c >> 16 & 255u) / 255.0f, (float)(c >> 24) / 255.0f };
}

template <typename SRC>
NV_TX TxF4 tx_bilinear(const SRC& src, uint64_t base, uint32_t w, uint32_t h, float u, float v)
{
	uint32_t x0, x1, y0, y1;
	float ax, ay;
	tx_axis(u, w, x0, x1, ax);
	tx_axis(v, h, y0, y1, ay);
	uint32_t c00, c01, c10, c11;
	src.quad(base, w, h, x0, x1, y0, y1, c00, c01, c10, c11);
	const TxF4 top = tx_lerp(tx_unorm(c00), tx_unorm(c01), ax);
	const TxF4 bottom = tx_lerp(tx_unorm(c10), tx_unorm(c11), ax);
	return tx_lerp(top, bottom, ay);
}

template <typename SRC>
NV_TX TxF4 tx_sample_lod(const SRC& src, float u, float v, float lod)
{
	const float top = (float)(src.levels - 1u);
	const float low = lod > 0.0f ? lod : 0.0f;
	const float lambda = low < top ? low : top;
	const float fl = __builtin_floorf(lambda);
	const float f = lambda - fl;
	uint32_t d = (uint32_t)tx_to_int(fl);
	d = d < src.levels ? d : src.levels - 1u;
	const uint32_t d1 = d + 1u < src.levels ? d + 1u : src.levels - 1u;
	uint64_t b0, b1;
	src.level_bases(d, d1, b0, b1);
	const TxF4 lo = tx_bilinear(src, b0, tx_level_side(src.width, d), tx_level_side(src.height, d), u, v);
	const TxF4 hi = tx_bilinear(src, b1, tx_level_side(src.width, d1), tx_level_side(src.height, d1), u, v);
	return tx_lerp(lo, hi, f);
}

template <typename SRC>
NV_TX TxF4 tx_sample(const SRC& src, float u, float v, float dudx, float dvdx, float dudy, float dvdy)
{
	return tx_sample_lod(src, u, v, tx_lambda(dudx, dvdx, dudy, dvdy, src.width, src.height, src.levels));
}

template <typename SRC>
NV_TX TxF4 tx_sample_lod0(const SRC& src, float u, float v) { return tx_sample_lod(src, u, v, 0.0f); }

// ---- what a texture set is.  A set is resident in one of two forms, TxDecoded here and TxBlocks below, and its three
// consumers — the attribute pass (visattr.h), the alpha-tested raster (rasterdepth.h) and the alpha-tested shadow trace (rtalpha.h) — take the
// form as a type and ask it for exactly this:
//   Desc, Unit                one texture's descriptor (four words, the C ABI's) and what the set's buffer is an array of
//   none()                    a well-formed descriptor that names nothing: what a consumer holds before it has looked a texture up
//   ok(d, extent)             the check in front of every load through d; `extent` is the buffer's size as the entry point took it.  A consumer
//                             compares the texture id with its table's count FIRST, loads the descriptor, then asks this (args.h TxTable::desc,
//                             rtalpha.h rt_albedo_desc); it loads nothing from the buffer through a descriptor this refused
//   sample(data, d, ...)      texture(sampler2D, uv) with explicit derivatives: the trilinear tx_sample, 8 taps
//   texture(table, id, ...)   texture(SAMP(id), uv) over a table of the set (args.h TxTable): desc, then sample.  false: textures[id] was not
//                             sampled and nothing was loaded from the buffer; the caller shades from the factors and counts the pixel
//   alpha_lod0(data, d, u, v) textureLod(sampler2D, uv, 0).w from level 0's four taps alone (the shadow trace's, shadow.comp.glsl:117)
// The two forms hand out the same RGBA8 codes and run the same operations on them in the same order, so a consumer's results are the same bits.
struct TxDecoded
{
	typedef TxDesc Desc;
	typedef uint32_t Unit; // RGBA8 words; extent = texelWords

	static NV_TXM Desc none() { return Desc{ 0u, 1u, 1u, 1u }; }
	static NV_TXM bool ok(const Desc& d, uint64_t extent) { return tx_desc_ok(d, extent); }
	static NV_TXM TxF4 sample(const Unit* texels, const Desc& d, float u, float v, float dudx, float dvdx, float dudy, float dvdy)
	{
		return tx_sample(texels, d, u, v, dudx, dvdx, dudy, dvdy);
	}
	template <typename TABLE>
	static NV_TXM bool texture(const TABLE& tx, uint32_t id, float u, float v, float dudx, float dvdx, float dudy, float dvdy, TxF4& c)
	{
		Desc d;
		if (!tx.desc(id, d))
			return false;
		c = sample(tx.data, d, u, v, dudx, dvdx, dudy, dvdy);
		return true;
	}

	// tx_sample_lod0(texels, t, u, v).w with the four alpha taps of level 0 alone.  tx_sample_lod at lambda = 0 blends level 0 with weight 1 - 0
	// and level min(1, levels - 1) with weight 0: lo * 1 + hi * 0.  Every alpha is in [0, 1] or NaN, and a NaN comes from u, v alone (tx_axis), so
	// hi is NaN only where lo is: for a finite lo the blend is lo + 0 = lo (lo >= 0, never -0), for a NaN lo it is NaN like lo.  The taps of the
	// second level and the three colour channels change nothing and are left out; tests/test_shadow_alpha_cpu.py holds the two forms bit-identical
	// (a NaN for a NaN: its sign and payload are no result, the test that follows is alpha >= 0.5).
	// t has passed ok(): tx_axis keeps every index inside level 0 for EVERY bit pattern of u, v.
	static NV_TXM float alpha_lod0(const Unit* texels, const Desc& t, float u, float v)
	{
		uint32_t x0, x1, y0, y1;
		float ax, ay;
		tx_axis(u, t.width, x0, x1, ax);
		tx_axis(v, t.height, y0, y1, ay);
		const uint64_t r0 = (uint64_t)t.offset + (uint64_t)y0 * t.width, r1 = (uint64_t)t.offset + (uint64_t)y1 * t.width;
		const uint32_t c00 = texels[r0 + x0], c01 = texels[r0 + x1], c10 = texels[r1 + x0], c11 = texels[r1 + x1]; // the four loads together
		const float a00 = (float)(c00 >> 24) / 255.0f, a01 = (float)(c01 >> 24) / 255.0f, a10 = (float)(c10 >> 24) / 255.0f, a11 = (float)(c11 >> 24) / 255.0f;
		return tx_lerp(tx_lerp(a00, a01, ax), tx_lerp(a10, a11, ax), ay);
	}
};

#ifndef NV_TX_SAMPLER_ONLY
// ---- the block source (§4.21): the set's buffer holds the DDS payloads verbatim and a tap decodes its texel from its block.

// BC7 in two parts: what a block says once (the mode's fields, the bases of its bit fields, the partition word and its anchors) and what one
// texel adds.  tx_bc7_texel above keeps its text; tx_bc7_texel_h(lo, hi, tx_bc7_header(lo, hi), t) is held equal to it on every fixture block.
struct TxBc7Header
{
	uint32_t fields;  // ns | cb << 4 | ab << 8 | ib << 12 | ib2 << 16 | rotation << 20 | isb << 24 | (uniqueP ? 1 : sharedP ? 2 : 0) << 28; 0: RESERVED
	uint32_t bases;   // colourBase | alphaBase << 8 | pBase << 16 | indexBase << 24 (each < 128)
	uint32_t part;    // TX_P2 / TX_P3 of the partition (ns = 2 / 3)
	uint32_t anchors; // a1 | a2 << 8 (16: no such anchor)
};

NV_TX TxBc7Header tx_bc7_header(uint64_t lo, uint64_t hi)
{
	const uint32_t byte0 = (uint32_t)lo & 255u;
	if (byte0 == 0u)
		return TxBc7Header{ 0u, 0u, 0u, 0u };
	const uint32_t mode = (uint32_t)__builtin_ctz(byte0);
	const uint32_t ns = tx_nibble(0x21112323u, mode), pb = tx_nibble(0x60006664u, mode), rb = tx_nibble(0x00220000u, mode);
	const uint32_t cb = tx_nibble(0x57757564u, mode), ab = tx_nibble(0x57860000u, mode), ib = tx_nibble(0x24222233u, mode);
	const uint32_t ib2 = tx_nibble(0x00230000u, mode);
	const bool uniqueP = mode == 0u || mode == 3u || mode == 6u || mode == 7u, sharedP = mode == 1u;
	const uint32_t ne = ns * 2u;
	uint32_t pos = mode + 1u;
	const uint32_t partition = tx_bits(lo, hi, pos, pb);
	pos += pb;
	const uint32_t rotation = tx_bits(lo, hi, pos, rb);
	pos += rb;
	const uint32_t isb = mode == 4u ? tx_bits(lo, hi, pos, 1u) : 0u;
	pos += mode == 4u ? 1u : 0u;
	const uint32_t colourBase = pos, alphaBase = colourBase + 3u * ne * cb, pBase = alphaBase + ne * ab;
	const uint32_t indexBase = pBase + (uniqueP ? ne : sharedP ? 2u : 0u);
	const uint32_t anchors = TX_ANCHOR[partition];
	const uint32_t a1 = ns == 1u ? 16u : ns == 2u ? anchors & 15u : anchors >> 4 & 15u;
	const uint32_t a2 = ns == 3u ? anchors >> 8 & 15u : 16u;
	TxBc7Header h;
	h.fields = ns | cb << 4 | ab << 8 | ib << 12 | ib2 << 16 | rotation << 20 | isb << 24 | (uniqueP ? 1u : sharedP ? 2u : 0u) << 28;
	h.bases = colourBase | alphaBase << 8 | pBase << 16 | indexBase << 24;
	h.part = ns == 2u ? (uint32_t)TX_P2[partition] : ns == 3u ? TX_P3[partition] : 0u;
	h.anchors = a1 | a2 << 8;
	return h;
}

// what both per-texel parts start with: the texel's subset, its two index weights and its endpoints' p-bits
struct TxBc7Tap
{
	uint32_t e0, wc, wa, p0, p1;
	bool hasP;
};

NV_TX TxBc7Tap tx_bc7_tap(uint64_t lo, uint64_t hi, const TxBc7Header& h, uint32_t t)
{
	const uint32_t ns = h.fields & 15u, ib = h.fields >> 12 & 15u, ib2 = h.fields >> 16 & 15u, isb = h.fields >> 24 & 1u, pkind = h.fields >> 28;
	const uint32_t pBase = h.bases >> 16 & 255u, indexBase = h.bases >> 24;
	const uint32_t a1 = h.anchors & 255u, a2 = h.anchors >> 8;
	const uint32_t subset = ns == 1u ? 0u : ns == 2u ? h.part >> t & 1u : h.part >> (2u * t) & 3u;
	const bool anchor = t == 0u || t == a1 || t == a2;
	const uint32_t index = tx_bits(lo, hi, indexBase + t * ib - (t > 0u ? 1u : 0u) - (t > a1 ? 1u : 0u) - (t > a2 ? 1u : 0u), anchor ? ib - 1u : ib);
	const uint32_t index2Base = indexBase + 16u * ib - ns;
	const uint32_t index2 = ib2 ? tx_bits(lo, hi, index2Base + t * ib2 - (t > 0u ? 1u : 0u), t == 0u ? ib2 - 1u : ib2) : 0u;
	const bool uniqueP = pkind == 1u, sharedP = pkind == 2u;
	TxBc7Tap k;
	k.e0 = subset * 2u;
	k.p0 = uniqueP ? tx_bits(lo, hi, pBase + k.e0, 1u) : sharedP ? tx_bits(lo, hi, pBase + subset, 1u) : 0u;
	k.p1 = uniqueP ? tx_bits(lo, hi, pBase + k.e0 + 1u, 1u) : k.p0;
	k.hasP = uniqueP || sharedP;
	const uint32_t wp = tx_bc7_weight(ib, index), ws = ib2 ? tx_bc7_weight(ib2, index2) : wp;
	k.wc = isb ? ws : wp, k.wa = ib2 ? (isb ? wp : ws) : wp;
	return k;
}

// texel t of the BC7 block {lo, hi} whose header is h: tx_bc7_texel(lo, hi, t)
NV_TX uint32_t tx_bc7_texel_h(uint64_t lo, uint64_t hi, const TxBc7Header& h, uint32_t t)
{
	if (h.fields == 0u)
		return 0u;
	const uint32_t ne = (h.fields & 15u) * 2u, cb = h.fields >> 4 & 15u, ab = h.fields >> 8 & 15u, rotation = h.fields >> 20 & 15u;
	const uint32_t colourBase = h.bases & 255u, alphaBase = h.bases >> 8 & 255u;
	const TxBc7Tap k = tx_bc7_tap(lo, hi, h, t);
	const uint32_t e0 = k.e0, e1 = e0 + 1u;
	const uint32_t r0 = tx_bc7_endpoint(lo, hi, colourBase + e0 * cb, cb, k.hasP, k.p0), r1 = tx_bc7_endpoint(lo, hi, colourBase + e1 * cb, cb, k.hasP, k.p1);
	const uint32_t g0 = tx_bc7_endpoint(lo, hi, colourBase + (ne + e0) * cb, cb, k.hasP, k.p0), g1 = tx_bc7_endpoint(lo, hi, colourBase + (ne + e1) * cb, cb, k.hasP, k.p1);
	const uint32_t b0 = tx_bc7_endpoint(lo, hi, colourBase + (2u * ne + e0) * cb, cb, k.hasP, k.p0), b1 = tx_bc7_endpoint(lo, hi, colourBase + (2u * ne + e1) * cb, cb, k.hasP, k.p1);
	const uint32_t al0 = ab ? tx_bc7_endpoint(lo, hi, alphaBase + e0 * ab, ab, k.hasP, k.p0) : 255u, al1 = ab ? tx_bc7_endpoint(lo, hi, alphaBase + e1 * ab, ab, k.hasP, k.p1) : 255u;
	uint32_t r = tx_bc7_mix(r0, r1, k.wc), g = tx_bc7_mix(g0, g1, k.wc), b = tx_bc7_mix(b0, b1, k.wc), a = tx_bc7_mix(al0, al1, k.wa);
	// (selects, where tx_bc7_texel branches: the rotation differs between the lanes of a wave)
	const uint32_t s = a;
	a = rotation == 1u ? r : rotation == 2u ? g : rotation == 3u ? b : a;
	r = rotation == 1u ? s : r, g = rotation == 2u ? s : g, b = rotation == 3u ? s : b;
	return (a & 255u) << 24 | (b & 255u) << 16 | (g & 255u) << 8 | (r & 255u);
}

// the alpha of texel t alone: tx_bc7_texel(lo, hi, t) >> 24.  Without rotation the alpha endpoints and the alpha weight; with it the colour
// channel the rotation swapped into alpha, with the colour weight.
NV_TX uint32_t tx_bc7_alpha_h(uint64_t lo, uint64_t hi, const TxBc7Header& h, uint32_t t)
{
	if (h.fields == 0u)
		return 0u;
	const uint32_t ne = (h.fields & 15u) * 2u, cb = h.fields >> 4 & 15u, ab = h.fields >> 8 & 15u, rotation = h.fields >> 20 & 15u;
	const uint32_t colourBase = h.bases & 255u, alphaBase = h.bases >> 8 & 255u;
	if (rotation == 0u && ab == 0u)
		return 255u;
	const TxBc7Tap k = tx_bc7_tap(lo, hi, h, t);
	const uint32_t bits = rotation ? cb : ab;
	const uint32_t at = rotation ? colourBase + ((rotation - 1u) * ne + k.e0) * cb : alphaBase + k.e0 * ab;
	const uint32_t v0 = tx_bc7_endpoint(lo, hi, at, bits, k.hasP, k.p0), v1 = tx_bc7_endpoint(lo, hi, at + bits, bits, k.hasP, k.p1);
	return tx_bc7_mix(v0, v1, rotation ? k.wc : k.wa) & 255u;
}

// the alpha of texel t of a block of a decodable format: tx_decode_texel(format, lo, hi, t) >> 24, for the two consumers that read .w only.
// BC1: the index and the endpoint order; BC2 / BC3: the alpha half; BC7: tx_bc7_alpha_h.
NV_TX uint32_t tx_decode_alpha(uint32_t format, uint64_t lo, uint64_t hi, uint32_t t)
{
	if (format == TX_BC1)
	{
		const uint32_t c0 = (uint32_t)lo & 0xffffu, c1 = (uint32_t)(lo >> 16) & 0xffffu, idx = (uint32_t)(lo >> (32u + 2u * t)) & 3u;
		return idx == 3u && c0 <= c1 ? 0u : 255u;
	}
	if (format == TX_BC2)
		return ((uint32_t)(lo >> (4u * t)) & 15u) * 17u;
	if (format == TX_BC3)
		return tx_bc3_alpha(lo, t);
	return tx_bc7_alpha_h(lo, hi, tx_bc7_header(lo, hi), t);
}

// the descriptor of one block-resident texture (== NvTextureBlockDesc): its payload — level after level as the file has them — lies from byte
// 16 * offset of the block buffer; levelsFormat = levels | format << 8
struct TxBlockDesc
{
	uint32_t offset, width, height, levelsFormat;
};

NV_TX uint32_t tx_level_blocks_x(uint32_t width, uint32_t level) { return (tx_level_side(width, level) + 3u) >> 2; }

// bytes of the first `levels` levels' blocks
NV_TX uint64_t tx_chain_block_bytes(uint32_t width, uint32_t height, uint32_t levels, uint32_t format)
{
	uint64_t n = 0;
	for (uint32_t l = 0; l < levels; ++l)
		n += (uint64_t)tx_level_blocks_x(width, l) * tx_level_blocks_x(height, l);
	return n * tx_block_bytes(format);
}

// the check in front of every block load: tx_desc_ok's shape limits, a decodable format, nothing but levels and format in levelsFormat, and
// the whole chain (rounded up to 16 bytes, as the layout places it) inside the caller's `units16`, in 64 bits
NV_TX bool tx_block_desc_ok(const TxBlockDesc& d, uint64_t units16)
{
	const uint32_t levels = d.levelsFormat & 255u, format = d.levelsFormat >> 8 & 255u;
	if (d.width == 0u || d.height == 0u || d.width > TX_MAX_SIDE || d.height > TX_MAX_SIDE || levels == 0u || levels > TX_MAX_LEVELS)
		return false;
	if (!tx_decodable(format) || (d.levelsFormat >> 16) != 0u)
		return false;
	return (uint64_t)d.offset + (tx_chain_block_bytes(d.width, d.height, levels, format) + 15u) / 16u <= units16;
}

// one block in registers: its bytes (BC1: lo only) and, for BC7, its header
struct TxBlock
{
	uint64_t lo, hi;
	TxBc7Header h;
};

// the source: a texture tx_block_desc_ok accepted.  Bases are byte offsets into `blocks`.
struct TxBlockSource
{
	const void* blocks;
	uint64_t byteBase; // 16 * offset
	uint32_t width, height, levels, format;

	NV_TXM void level_bases(uint32_t d, uint32_t d1, uint64_t& b0, uint64_t& b1) const
	{
		const uint32_t bb = tx_block_bytes(format);
		uint64_t base = byteBase;
		b0 = base, b1 = base;
		for (uint32_t l = 0; l < levels; ++l)
		{
			b0 = l == d ? base : b0;
			b1 = l == d1 ? base : b1;
			base += (uint64_t)tx_level_blocks_x(width, l) * tx_level_blocks_x(height, l) * bb;
		}
	}

	// block `index` of the level at `base`: 8 bytes (BC1) or 16 bytes in one load, parsed once
	NV_TXM TxBlock load(uint64_t base, uint32_t index) const
	{
		TxBlock b;
		b.h = TxBc7Header{ 0u, 0u, 0u, 0u };
		if (format == TX_BC1)
		{
			const unsigned char* p = static_cast<const unsigned char*>(blocks) + base + (uint64_t)index * 8u;
#if defined(__HIP_DEVICE_COMPILE__)
			p = static_cast<const unsigned char*>(__builtin_assume_aligned(p, 8));
#endif
			__builtin_memcpy(&b.lo, p, 8);
			b.hi = 0u;
		}
		else
		{
			const unsigned char* p = static_cast<const unsigned char*>(blocks) + base + (uint64_t)index * 16u;
#if defined(__HIP_DEVICE_COMPILE__)
			p = static_cast<const unsigned char*>(__builtin_assume_aligned(p, 16)); // (the entry points refuse a misaligned buffer; offsets are 16-byte units)
#endif
			uint64_t q[2];
			__builtin_memcpy(q, p, 16);
			b.lo = q[0], b.hi = q[1];
			if (format == TX_BC7)
				b.h = tx_bc7_header(b.lo, b.hi);
		}
		return b;
	}

	NV_TXM uint32_t texel(const TxBlock& b, uint32_t t) const
	{
		return format == TX_BC7 ? tx_bc7_texel_h(b.lo, b.hi, b.h, t) : tx_decode_texel(format, b.lo, b.hi, t);
	}
	NV_TXM uint32_t alpha(const TxBlock& b, uint32_t t) const
	{
		return format == TX_BC7 ? tx_bc7_alpha_h(b.lo, b.hi, b.h, t) : tx_decode_alpha(format, b.lo, b.hi, t);
	}

	// The four taps of one level, each block loaded and parsed once: the walk goes 00 -> 01 -> 11 -> 10 when x0 and x1 share a block column
	// and 00 -> 10 -> 11 -> 01 otherwise, so a step that changes the block is taken once per distinct block (1 for 9 of 16 texel positions,
	// 2 across one edge, 4 at a corner); a step inside the block keeps it.  ALPHA: the codes' top bytes only, in bits 24-31.
	template <bool ALPHA>
	NV_TXM void walk(uint64_t base, uint32_t w, uint32_t x0, uint32_t x1, uint32_t y0, uint32_t y1, uint32_t& c00, uint32_t& c01, uint32_t& c10, uint32_t& c11) const
	{
		const uint32_t bw = (w + 3u) >> 2;
		const bool xfirst = (x0 >> 2) == (x1 >> 2);
		const uint32_t xa = xfirst ? x1 : x0, ya = xfirst ? y0 : y1; // the second tap
		const uint32_t xb = xfirst ? x0 : x1, yb = xfirst ? y1 : y0; // the fourth
		uint32_t cur = (y0 >> 2) * bw + (x0 >> 2);
		TxBlock b = load(base, cur);
		c00 = ALPHA ? alpha(b, (y0 & 3u) * 4u + (x0 & 3u)) << 24 : texel(b, (y0 & 3u) * 4u + (x0 & 3u));
		uint32_t at = (ya >> 2) * bw + (xa >> 2);
		if (at != cur)
			b = load(base, at), cur = at;
		const uint32_t ca = ALPHA ? alpha(b, (ya & 3u) * 4u + (xa & 3u)) << 24 : texel(b, (ya & 3u) * 4u + (xa & 3u));
		at = (y1 >> 2) * bw + (x1 >> 2);
		if (at != cur)
			b = load(base, at), cur = at;
		c11 = ALPHA ? alpha(b, (y1 & 3u) * 4u + (x1 & 3u)) << 24 : texel(b, (y1 & 3u) * 4u + (x1 & 3u));
		at = (yb >> 2) * bw + (xb >> 2);
		if (at != cur)
			b = load(base, at), cur = at;
		const uint32_t cb = ALPHA ? alpha(b, (yb & 3u) * 4u + (xb & 3u)) << 24 : texel(b, (yb & 3u) * 4u + (xb & 3u));
		c01 = xfirst ? ca : cb;
		c10 = xfirst ? cb : ca;
	}

	NV_TXM void quad(uint64_t base, uint32_t w, uint32_t h, uint32_t x0, uint32_t x1, uint32_t y0, uint32_t y1, uint32_t& c00, uint32_t& c01, uint32_t& c10, uint32_t& c11) const
	{
		(void)h;
		walk<false>(base, w, x0, x1, y0, y1, c00, c01, c10, c11);
	}

	// the RGBA8 code of texel (x, y) of `level` (level < levels, x and y inside the level)
	NV_TXM uint32_t fetch(uint32_t level, uint32_t x, uint32_t y) const
	{
		uint64_t b0, b1;
		level_bases(level, level, b0, b1);
		const TxBlock b = load(b0, (y >> 2) * tx_level_blocks_x(width, level) + (x >> 2));
		return texel(b, (y & 3u) * 4u + (x & 3u));
	}
};

// the source of a descriptor tx_block_desc_ok accepted
NV_TX TxBlockSource tx_block_source(const void* blocks, const TxBlockDesc& d)
{
	return TxBlockSource{ blocks, (uint64_t)d.offset * 16u, d.width, d.height, d.levelsFormat & 255u, d.levelsFormat >> 8 & 255u };
}

// the block-resident form of a texture set: TxDecoded's interface over the DDS payloads.  Only a translation unit that includes this header in
// full has it: one that defines NV_TX_SAMPLER_ONLY and names TxBlocks does not compile.
struct TxBlocks
{
	typedef TxBlockDesc Desc;
	typedef unsigned char Unit; // the payloads' bytes, 16-byte aligned; extent = units16

	static NV_TXM Desc none() { return Desc{ 0u, 1u, 1u, 1u | TX_BC1 << 8 }; }
	static NV_TXM bool ok(const Desc& d, uint64_t extent) { return tx_block_desc_ok(d, extent); }
	static NV_TXM TxF4 sample(const Unit* blocks, const Desc& d, float u, float v, float dudx, float dvdx, float dudy, float dvdy)
	{
		return tx_sample(tx_block_source(blocks, d), u, v, dudx, dvdx, dudy, dvdy);
	}
	// (TxDecoded::texture with TABLE::desc's three statements written out: the text the block kernel of the attribute pass was compiled from.  Through
	// the call the compiler lays the same operations out in another order, and the kernels keep their code: profiles/texture_set_refactor.md)
	template <typename TABLE>
	static NV_TXM bool texture(const TABLE& tx, uint32_t id, float u, float v, float dudx, float dvdx, float dudy, float dvdy, TxF4& c)
	{
		if (id >= tx.count)
			return false;
		const auto w = tx.descs[id];
		const Desc d = { w.x, w.y, w.z, w.w };
		if (!ok(d, tx.extent))
			return false;
		c = sample(tx.data, d, u, v, dudx, dvdx, dudy, dvdy);
		return true;
	}

	// TxDecoded::alpha_lod0 with the four taps' alpha decoded from their blocks — alpha alone (tx_decode_alpha), a block loaded once per distinct
	// block of the four taps (level 0 starts at the texture's first byte).  The alpha codes are the decoded chain's top bytes and the blend is the same
	static NV_TXM float alpha_lod0(const Unit* blocks, const Desc& d, float u, float v)
	{
		const TxBlockSource src = tx_block_source(blocks, d);
		uint32_t x0, x1, y0, y1;
		float ax, ay;
		tx_axis(u, src.width, x0, x1, ax);
		tx_axis(v, src.height, y0, y1, ay);
		uint32_t c00, c01, c10, c11;
		src.walk<true>(src.byteBase, src.width, x0, x1, y0, y1, c00, c01, c10, c11);
		const float a00 = (float)(c00 >> 24) / 255.0f, a01 = (float)(c01 >> 24) / 255.0f, a10 = (float)(c10 >> 24) / 255.0f, a11 = (float)(c11 >> 24) / 255.0f;
		return tx_lerp(tx_lerp(a00, a01, ax), tx_lerp(a10, a11, ax), ay);
	}
};
#endif // NV_TX_SAMPLER_ONLY

} // namespace nv
