// tools/texture_block_check.cpp — a stand-alone driver of the host side of the block-resident texture sets for the
// sanitizers: the block layout, the per-texel fetch over every texel of every level against the decoded chain, the alpha-only decode and the
// BC7 header / per-texel split against the plain decode, and the block sampler against the decoded sampler, bit for bit, over adversarial and
// random coordinates and descriptors.  The block buffer is an exactly-sized heap allocation, so AddressSanitizer is the judge of "every
// index that reaches a load is in range".  Build and run (host code only, no device):
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I include
//       tools/texture_block_check.cpp niagara_amd/csrc/texload.cpp -o texture_block_check
//   ./texture_block_check [file of raw 16-byte blocks]
//
// With a file argument (raw 16-byte blocks, e.g. the fixture's) the textures are filled from those blocks; without, with pseudo-random blocks
// that force every BC7 mode and the reserved one.  Exit status 0 and "texture_block_check: ok" mean every call returned what it must and no
// sanitizer spoke.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/niagara_vis.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
	g_state ^= g_state << 13, g_state ^= g_state >> 7, g_state ^= g_state << 17;
	return (uint32_t)(g_state >> 16);
}

#define CHECK(c) \
	do \
	{ \
		if (!(c)) \
		{ \
			fprintf(stderr, "texture_block_check: %s failed at line %d\n", #c, __LINE__); \
			exit(1); \
		} \
	} while (0)

static uint32_t side(uint32_t s, uint32_t l) { return (s >> l) ? s >> l : 1u; }

int main(int argc, char** argv)
{
	std::vector<uint8_t> extra;
	if (argc > 1)
	{
		FILE* f = fopen(argv[1], "rb");
		CHECK(f);
		uint8_t buf[4096];
		for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;)
			extra.insert(extra.end(), buf, buf + n);
		fclose(f);
		CHECK(!extra.empty());
	}

	// ---- 1. the set: odd shapes, the 2 x 1 / 1 x 1 tail, every format, every BC7 mode
	const uint32_t formats[4] = { NV_FORMAT_BC1, NV_FORMAT_BC2, NV_FORMAT_BC3, NV_FORMAT_BC7 };
	const uint32_t shapes[][3] = { { 4, 4, 1 }, { 20, 12, 5 }, { 1, 1, 1 }, { 2, 1, 2 }, { 256, 64, 9 }, { 5, 7, 3 }, { 64, 64, 7 }, { 3, 1, 4 }, { 8, 8, 1 } };
	std::vector<NvDdsInfo> infos;
	std::vector<std::vector<uint8_t>> payloads;
	for (const auto& s : shapes)
		for (uint32_t format : formats)
		{
			NvDdsInfo info;
			memset(&info, 0, sizeof(info));
			info.format = format, info.width = s[0], info.height = s[1], info.levels = s[2], info.blockBytes = format == NV_FORMAT_BC1 ? 8u : 16u;
			for (uint32_t l = 0; l < info.levels; ++l)
			{
				info.levelOffset[l] = info.payloadBytes;
				info.payloadBytes += (uint64_t)((side(s[0], l) + 3) / 4) * ((side(s[1], l) + 3) / 4) * info.blockBytes;
			}
			std::vector<uint8_t> p(info.payloadBytes);
			for (size_t i = 0; i < p.size(); ++i)
				p[i] = extra.empty() ? (uint8_t)rnd() : extra[(i + infos.size() * 16) % extra.size()];
			if (format == NV_FORMAT_BC7 && extra.empty())
				for (uint64_t b = 0; b < info.payloadBytes / 16; ++b)
				{
					const uint32_t mode = (uint32_t)(b % 9);
					uint8_t& first = p[b * 16];
					first = mode == 8 ? 0 : (uint8_t)((first & ~((2u << mode) - 1u)) | 1u << mode);
				}
			infos.push_back(info);
			payloads.push_back(p);
		}
	const uint32_t count = (uint32_t)infos.size();
	std::vector<NvTextureBlockDesc> bdescs(count + 1);
	std::vector<NvTextureDesc> descs(count + 1);
	uint64_t units = 0, words = 0, sum16 = 0;
	CHECK(nv_texture_block_layout(infos.data(), count, bdescs.data(), &units) == NV_OK && bdescs[0].levelsFormat == 0 && bdescs[0].width == 0);
	CHECK(nv_texture_set_layout(infos.data(), count, descs.data(), &words) == NV_OK);
	for (uint32_t i = 0; i < count; ++i)
	{
		CHECK(bdescs[i + 1].offset == sum16 && bdescs[i + 1].levelsFormat == (infos[i].levels | infos[i].format << 8));
		sum16 += (infos[i].payloadBytes + 15) / 16;
	}
	CHECK(units == sum16);
	// exactly-sized, and not more aligned than malloc makes it: a 16-byte read past the last BC1 block of the set would be a heap overflow
	std::vector<uint8_t> blocks(units * 16, 0xA5);
	std::vector<uint32_t> texels(words, 0xDEADBEEFu);
	for (uint32_t i = 0; i < count; ++i)
	{
		memcpy(blocks.data() + (size_t)bdescs[i + 1].offset * 16, payloads[i].data(), payloads[i].size());
		CHECK(nv_texture_decode_host(&infos[i], payloads[i].data(), &descs[i + 1], texels.data(), words) == NV_OK);
	}
	{
		NvDdsInfo bad = infos[0];
		std::vector<NvTextureBlockDesc> d2(2);
		uint64_t u2;
		bad.format = NV_FORMAT_BC4;
		CHECK(nv_texture_block_layout(&bad, 1, d2.data(), &u2) == NV_ETEXFORMAT);
		bad.format = 9;
		CHECK(nv_texture_block_layout(&bad, 1, d2.data(), &u2) == NV_EINVAL);
		bad = infos[0], bad.levels = 16;
		CHECK(nv_texture_block_layout(&bad, 1, d2.data(), &u2) == NV_EINVAL);
		bad = infos[0], bad.width = 16385;
		CHECK(nv_texture_block_layout(&bad, 1, d2.data(), &u2) == NV_EINVAL);
		CHECK(nv_texture_block_layout(nullptr, 1, d2.data(), &u2) == NV_EINVAL);
	}

	// ---- 2. the fetch: every texel of every level is the word the decode stored
	uint64_t fetched = 0;
	for (uint32_t i = 0; i < count; ++i)
	{
		uint64_t at = descs[i + 1].offset;
		for (uint32_t l = 0; l < infos[i].levels; ++l)
		{
			const uint32_t w = side(infos[i].width, l), h = side(infos[i].height, l);
			for (uint32_t y = 0; y < h; ++y)
				for (uint32_t x = 0; x < w; ++x, ++fetched)
				{
					uint32_t c = 0;
					CHECK(nv_texture_block_fetch_host(&bdescs[i + 1], blocks.data(), units, l, x, y, &c) == NV_OK);
					CHECK(c == texels[at + (uint64_t)y * w + x]);
				}
			uint32_t c;
			CHECK(nv_texture_block_fetch_host(&bdescs[i + 1], blocks.data(), units, l, w, 0, &c) == NV_EINVAL);
			CHECK(nv_texture_block_fetch_host(&bdescs[i + 1], blocks.data(), units, l, 0, h, &c) == NV_EINVAL);
			at += (uint64_t)w * h;
		}
		uint32_t c;
		CHECK(nv_texture_block_fetch_host(&bdescs[i + 1], blocks.data(), units, infos[i].levels, 0, 0, &c) == NV_EINVAL);
	}
	{
		// the last texture against a buffer one unit short, a format outside the four, too many levels, stray upper bits
		uint32_t c;
		CHECK(nv_texture_block_fetch_host(&bdescs[count], blocks.data(), units - 1, 0, 0, 0, &c) == NV_EINVAL);
		NvTextureBlockDesc d = bdescs[count];
		d.offset += 1;
		CHECK(nv_texture_block_fetch_host(&d, blocks.data(), units, 0, 0, 0, &c) == NV_EINVAL);
		d = bdescs[1], d.levelsFormat = 1u | NV_FORMAT_BC4 << 8;
		CHECK(nv_texture_block_fetch_host(&d, blocks.data(), units, 0, 0, 0, &c) == NV_EINVAL);
		d = bdescs[1], d.levelsFormat = 16u | NV_FORMAT_BC1 << 8;
		CHECK(nv_texture_block_fetch_host(&d, blocks.data(), units, 0, 0, 0, &c) == NV_EINVAL);
		d = bdescs[1], d.levelsFormat |= 1u << 16;
		CHECK(nv_texture_block_fetch_host(&d, blocks.data(), units, 0, 0, 0, &c) == NV_EINVAL);
		d = bdescs[1], d.offset = 0xFFFFFFFFu;
		CHECK(nv_texture_block_fetch_host(&d, blocks.data(), units, 0, 0, 0, &c) == NV_EINVAL);
	}

	// ---- 3. per block: the alpha-only decode and the BC7 split against the decoded words (the 4 x 4 textures and the blocks of the rest)
	uint64_t decoded = 0;
	for (uint32_t i = 0; i < count; ++i)
		for (uint64_t b = 0; b < infos[i].payloadBytes / infos[i].blockBytes; ++b, ++decoded)
		{
			uint64_t lo = 0, hi = 0;
			memcpy(&lo, payloads[i].data() + b * infos[i].blockBytes, 8);
			if (infos[i].blockBytes == 16)
				memcpy(&hi, payloads[i].data() + b * 16 + 8, 8);
			NvDdsInfo one;
			memset(&one, 0, sizeof(one));
			one.format = infos[i].format, one.width = 4, one.height = 4, one.levels = 1, one.blockBytes = infos[i].blockBytes, one.payloadBytes = one.blockBytes;
			const NvTextureDesc d = { 0, 4, 4, 1 };
			uint32_t want[16], alpha[16], split[16];
			CHECK(nv_texture_decode_host(&one, payloads[i].data() + b * infos[i].blockBytes, &d, want, 16) == NV_OK);
			CHECK(nv_texture_block_decode_host(infos[i].format, lo, hi, alpha, split) == NV_OK);
			for (int t = 0; t < 16; ++t)
				CHECK(alpha[t] == want[t] >> 24 && split[t] == want[t]);
		}
	uint32_t a16[16], s16[16];
	CHECK(nv_texture_block_decode_host(NV_FORMAT_BC5, 0, 0, a16, s16) == NV_EINVAL);

	// ---- 4. the sampler: the decoded sampler's bits, for adversarial and for arbitrary coordinates
	const float special[] = { NAN, INFINITY, -INFINITY, 65504.0f, -65504.0f, 3.4e38f, -3.4e38f, 1e-45f, -1e-45f, 0.0f, -0.0f, 1.0f, -1.0f,
		                      0.99999994f, -5.9604645e-8f, 16383.5f, 1e9f, -1e9f, 0.5f };
	const int ns = (int)(sizeof(special) / sizeof(special[0]));
	uint64_t samples = 0;
	for (uint32_t id = 1; id <= count; ++id)
		for (int a = 0; a < ns; ++a)
			for (int b = 0; b < ns; ++b, ++samples)
			{
				const float uv[2] = { special[a], special[b] }, dx[2] = { special[(a + b) % ns], special[(a * 7 + 3) % ns] }, dy[2] = { special[b], special[a] };
				float got[4], want[4];
				CHECK(nv_texture_block_sample_host(bdescs.data(), count + 1, blocks.data(), units, id, uv, dx, dy, got) == NV_OK);
				CHECK(nv_texture_sample_host(descs.data(), count + 1, texels.data(), words, id, uv, dx, dy, want) == NV_OK);
				for (int k = 0; k < 4; ++k)
					CHECK(memcmp(&got[k], &want[k], 4) == 0 || (got[k] != got[k] && want[k] != want[k]));
			}
	for (int i = 0; i < 300000; ++i, ++samples)
	{
		const uint32_t id = 1 + rnd() % count;
		float f[6], got[4], want[4];
		if (i & 1)
		{
			uint32_t bits[6];
			for (uint32_t& b : bits)
				b = rnd() << 16 ^ rnd(); // any bit pattern
			memcpy(f, bits, sizeof(f));
		}
		else
		{
			for (int k = 0; k < 2; ++k)
				f[k] = (float)(rnd() % 65536) / 16384.0f - 2.0f; // uv across several periods
			for (int k = 2; k < 6; ++k)
				f[k] = ((float)(rnd() % 4096) - 2048.0f) / (float)(1u << (rnd() % 14 + 6)); // derivatives over every level
		}
		CHECK(nv_texture_block_sample_host(bdescs.data(), count + 1, blocks.data(), units, id, f, f + 2, f + 4, got) == NV_OK);
		CHECK(nv_texture_sample_host(descs.data(), count + 1, texels.data(), words, id, f, f + 2, f + 4, want) == NV_OK);
		for (int k = 0; k < 4; ++k)
			CHECK(memcmp(&got[k], &want[k], 4) == 0 || (got[k] != got[k] && want[k] != want[k]));
	}
	const float uv[2] = { 0.25f, 0.75f }, zero[2] = { 0.0f, 0.0f };
	float out[4];
	CHECK(nv_texture_block_sample_host(bdescs.data(), count + 1, blocks.data(), units, 0, uv, zero, zero, out) == NV_EINVAL);
	CHECK(nv_texture_block_sample_host(bdescs.data(), count + 1, blocks.data(), units, count + 1, uv, zero, zero, out) == NV_EINVAL);
	CHECK(nv_texture_block_sample_host(bdescs.data(), count + 1, blocks.data(), units, 0xFFFFFFFFu, uv, zero, zero, out) == NV_EINVAL);
	CHECK(nv_texture_block_sample_host(bdescs.data(), count + 1, blocks.data(), units - 1, count, uv, zero, zero, out) == NV_EINVAL);
	for (int i = 0; i < 200000; ++i)
	{
		const uint32_t lf = rnd() % 4 ? (rnd() % 20) | (rnd() % 10) << 8 : rnd() << 16 ^ rnd();
		NvTextureBlockDesc bad[2] = { { 0, 0, 0, 0 }, { rnd() % 3 ? rnd() % (uint32_t)(units + 8) : rnd() << 16 ^ rnd(), rnd() % 3 ? rnd() % 70 : rnd() << 16 ^ rnd(),
			                                            rnd() % 3 ? rnd() % 70 : rnd(), lf } };
		const int rc = nv_texture_block_sample_host(bad, 2, blocks.data(), units, 1, uv, uv, uv, out); // a load only if the whole chain is inside
		CHECK(rc == NV_OK || rc == NV_EINVAL);
	}
	printf("texture_block_check: ok (%u textures, %llu units of 16 bytes against %llu texel words, %llu texels fetched, %llu blocks, %llu samples)\n", count,
	       (unsigned long long)units, (unsigned long long)words, (unsigned long long)fetched, (unsigned long long)decoded, (unsigned long long)samples);
	return 0;
}
