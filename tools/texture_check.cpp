// tools/texture_check.cpp — a stand-alone driver of the host side of the material textures for the sanitizers: the DDS
// parser over truncated and corrupted headers, the set layout, the host decode of every 16-byte pattern family into exactly-sized heap
// buffers, and the host sampler over adversarial coordinates and descriptors.  Exactly-sized allocations make AddressSanitizer the judge of
// "every index that reaches a load is in range".  Build and run (host code only, no device):
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       tools/texture_check.cpp niagara_amd/csrc/texload.cpp -o texture_check && ./texture_check [file of raw 16-byte blocks]
//
// With a file argument (raw 16-byte blocks) those blocks are decoded too; without, pseudo-random blocks with every BC7 mode forced are.
// Exit status 0 and "texture_check: ok" mean every call returned what it must and no sanitizer spoke.
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
			fprintf(stderr, "texture_check: %s failed at line %d\n", #c, __LINE__); \
			exit(1); \
		} \
	} while (0)

static std::vector<uint8_t> dds(uint32_t fourCC, uint32_t dxgi, uint32_t width, uint32_t height, uint32_t levels, uint32_t blockBytes)
{
	const bool dx10 = fourCC == 0x30315844u;
	std::vector<uint32_t> w(dx10 ? 37 : 32, 0u);
	w[0] = 0x20534444u, w[1] = 124u, w[3] = height, w[4] = width, w[7] = levels, w[19] = 32u, w[20] = 4u, w[21] = fourCC;
	if (dx10)
		w[32] = dxgi, w[33] = 3u, w[35] = 1u;
	uint64_t bytes = 0;
	for (uint32_t l = 0, lw = width, lh = height; l < levels; ++l, lw = lw > 1 ? lw / 2 : 1, lh = lh > 1 ? lh / 2 : 1)
		bytes += (uint64_t)((lw + 3) / 4) * ((lh + 3) / 4) * blockBytes;
	std::vector<uint8_t> out(w.size() * 4 + bytes);
	memcpy(out.data(), w.data(), w.size() * 4);
	for (size_t i = w.size() * 4; i < out.size(); ++i)
		out[i] = (uint8_t)rnd();
	return out;
}

int main(int argc, char** argv)
{
	// ---- 1. the parser: every prefix of a valid file, and every single corrupted header word
	const struct
	{
		uint32_t fourCC, dxgi, block, format;
	} kinds[] = { { 0x31545844u, 0, 8, NV_FORMAT_BC1 }, { 0x33545844u, 0, 16, NV_FORMAT_BC2 }, { 0x35545844u, 0, 16, NV_FORMAT_BC3 },
		          { 0x30315844u, 98, 16, NV_FORMAT_BC7 }, { 0x30315844u, 71, 8, NV_FORMAT_BC1 }, { 0x31495441u, 0, 8, NV_FORMAT_BC4 },
		          { 0x30315844u, 95, 16, NV_FORMAT_BC6H } };
	for (const auto& k : kinds)
	{
		const std::vector<uint8_t> file = dds(k.fourCC, k.dxgi, 20, 12, 5, k.block);
		NvDdsInfo info;
		CHECK(nv_dds_parse(file.data(), file.size(), &info) == NV_OK && info.format == k.format && info.levels == 5 && info.blockBytes == k.block);
		CHECK(info.payloadOffset + info.payloadBytes == file.size() && info.levelOffset[4] == 24u * k.block);
		for (size_t cut = 0; cut < file.size(); ++cut)
		{
			std::vector<uint8_t> part(file.begin(), file.begin() + cut); // exactly-sized: a read past `cut` is a heap overflow
			CHECK(nv_dds_parse(part.data(), part.size(), &info) == NV_EFORMAT || (cut == 0 && !part.data()));
		}
		for (size_t word = 0; word < info.payloadOffset / 4; ++word)
			for (int trial = 0; trial < 8; ++trial)
			{
				std::vector<uint8_t> bad(file);
				const uint32_t v = trial == 0 ? 0u : trial == 1 ? 0xFFFFFFFFu : rnd();
				memcpy(bad.data() + word * 4, &v, 4);
				const int rc = nv_dds_parse(bad.data(), bad.size(), &info);
				CHECK(rc == NV_OK || rc == NV_EFORMAT);
				if (rc == NV_OK)
					CHECK(info.payloadOffset + info.payloadBytes == bad.size());
			}
	}
	NvDdsInfo none;
	CHECK(nv_dds_parse(nullptr, 0, &none) == NV_EINVAL);

	// ---- 2. layout + decode into exactly-sized buffers: odd shapes, the 2 x 1 / 1 x 1 tail, every format, every BC7 mode
	std::vector<uint8_t> extra;
	if (argc > 1)
	{
		FILE* f = fopen(argv[1], "rb");
		CHECK(f);
		uint8_t buf[4096];
		for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;)
			extra.insert(extra.end(), buf, buf + n);
		fclose(f);
	}
	const uint32_t shapes[][3] = { { 4, 4, 1 }, { 20, 12, 5 }, { 1, 1, 1 }, { 2, 1, 2 }, { 256, 64, 9 }, { 5, 7, 3 }, { 64, 64, 7 }, { 3, 1, 4 } };
	std::vector<std::vector<uint8_t>> files;
	std::vector<NvDdsInfo> infos;
	for (const auto& s : shapes)
		for (int k = 0; k < 4; ++k)
		{
			files.push_back(dds(kinds[k].fourCC, kinds[k].dxgi, s[0], s[1], s[2], kinds[k].block));
			std::vector<uint8_t>& file = files.back();
			NvDdsInfo info;
			CHECK(nv_dds_parse(file.data(), file.size(), &info) == NV_OK);
			if (kinds[k].format == NV_FORMAT_BC7) // force every mode (and the reserved one) in turn
				for (uint64_t b = 0; b < info.payloadBytes / 16; ++b)
				{
					const uint32_t mode = (uint32_t)(b % 9);
					uint8_t& first = file[info.payloadOffset + b * 16];
					first = mode == 8 ? 0 : (uint8_t)((first & ~((2u << mode) - 1u)) | 1u << mode);
				}
			if (!extra.empty())
				for (uint64_t b = 0; b < info.payloadBytes; ++b)
					file[info.payloadOffset + b] = extra[(b + files.size() * 16) % extra.size()];
			infos.push_back(info);
		}
	std::vector<NvTextureDesc> descs(infos.size() + 1);
	uint64_t words = 0;
	CHECK(nv_texture_set_layout(infos.data(), (uint32_t)infos.size(), descs.data(), &words) == NV_OK && descs[0].levels == 0);
	std::vector<uint32_t> texels(words, 0xDEADBEEFu);
	for (size_t i = 0; i < infos.size(); ++i)
	{
		std::vector<uint8_t> payload(files[i].begin() + infos[i].payloadOffset, files[i].end()); // exactly-sized
		CHECK(nv_texture_decode_host(&infos[i], payload.data(), &descs[i + 1], texels.data(), words) == NV_OK);
	}
	{
		NvDdsInfo bc4 = infos[0];
		bc4.format = NV_FORMAT_BC4;
		uint64_t w2;
		std::vector<NvTextureDesc> d2(2);
		CHECK(nv_texture_set_layout(&bc4, 1, d2.data(), &w2) == NV_ETEXFORMAT);
		NvTextureDesc shifted = descs[infos.size()];
		shifted.offset += 1; // the last chain would end one word past the buffer
		std::vector<uint8_t> payload(files.back().begin() + infos.back().payloadOffset, files.back().end());
		CHECK(nv_texture_decode_host(&infos.back(), payload.data(), &shifted, texels.data(), words) == NV_EINVAL);
	}

	// ---- 3. the sampler: adversarial coordinates on every texture, adversarial descriptors
	const float special[] = { NAN, INFINITY, -INFINITY, 65504.0f, -65504.0f, 3.4e38f, -3.4e38f, 1e-45f, -1e-45f, 0.0f, -0.0f, 1.0f, -1.0f,
		                      0.99999994f, -5.9604645e-8f, 16383.5f, 1e9f, -1e9f, 0.5f };
	const int ns = (int)(sizeof(special) / sizeof(special[0]));
	double sum = 0;
	for (uint32_t id = 1; id < descs.size(); ++id)
		for (int a = 0; a < ns; ++a)
			for (int b = 0; b < ns; ++b)
			{
				const float uv[2] = { special[a], special[b] }, dx[2] = { special[(a + b) % ns], special[(a * 7 + 3) % ns] }, dy[2] = { special[b], special[a] };
				float out[4];
				CHECK(nv_texture_sample_host(descs.data(), (uint32_t)descs.size(), texels.data(), words, id, uv, dx, dy, out) == NV_OK);
				sum += out[0] == out[0] ? out[0] : 0.0;
			}
	for (int i = 0; i < 200000; ++i)
	{
		const uint32_t id = 1 + rnd() % (uint32_t)(descs.size() - 1);
		uint32_t bits[6];
		for (uint32_t& b : bits)
			b = rnd() << 16 ^ rnd(); // any bit pattern
		float f[6], out[4];
		memcpy(f, bits, sizeof(f));
		CHECK(nv_texture_sample_host(descs.data(), (uint32_t)descs.size(), texels.data(), words, id, f, f + 2, f + 4, out) == NV_OK);
		sum += out[3] == out[3] ? out[3] : 0.0;
	}
	const float uv[2] = { 0.25f, 0.75f }, zero[2] = { 0.0f, 0.0f };
	float out[4];
	CHECK(nv_texture_sample_host(descs.data(), (uint32_t)descs.size(), texels.data(), words, 0, uv, zero, zero, out) == NV_EINVAL);
	CHECK(nv_texture_sample_host(descs.data(), (uint32_t)descs.size(), texels.data(), words, (uint32_t)descs.size(), uv, zero, zero, out) == NV_EINVAL);
	CHECK(nv_texture_sample_host(descs.data(), (uint32_t)descs.size(), texels.data(), words, 0xFFFFFFFFu, uv, zero, zero, out) == NV_EINVAL);
	for (int i = 0; i < 200000; ++i)
	{
		NvTextureDesc bad[2] = { { 0, 0, 0, 0 }, { rnd() << 16 ^ rnd(), rnd() % 3 ? rnd() % 70 : rnd() << 16 ^ rnd(), rnd() % 3 ? rnd() % 70 : rnd(), rnd() % 20 } };
		const int rc = nv_texture_sample_host(bad, 2, texels.data(), words, 1, uv, uv, uv, out); // a load only if the whole chain is inside
		CHECK(rc == NV_OK || rc == NV_EINVAL);
	}
	printf("texture_check: ok (%zu textures, %llu texel words, checksum %.3f)\n", infos.size(), (unsigned long long)words, sum);
	return 0;
}
