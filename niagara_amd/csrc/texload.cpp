// texload.cpp — the host side of the material textures: the DDS reader, the layout of a texture set, the CPU decode and the
// CPU sampler (both through texmath.h, the text the kernels run) and the texture paths of a scene cache.  No device work, no allocation.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/niagara_vis.h"
#include "texmath.h"

static_assert(sizeof(nv::TxDesc) == sizeof(NvTextureDesc), "TxDesc is NvTextureDesc");
static_assert(sizeof(nv::TxBlockDesc) == sizeof(NvTextureBlockDesc), "TxBlockDesc is NvTextureBlockDesc");
static_assert(NV_FORMAT_BC1 ==nv::TX_BC1 && NV_FORMAT_BC2 == nv::TX_BC2 && NV_FORMAT_BC3 == nv::TX_BC3 && NV_FORMAT_BC7 == nv::TX_BC7, "formats");
static_assert(NV_TEXTURE_MAX_LEVELS == nv::TX_MAX_LEVELS, "levels");

namespace
{
// DDS_HEADER / DDS_PIXELFORMAT / DDS_HEADER_DXT10 as word offsets from the start of the file (the magic is word 0)
enum
{
	kSize = 1,
	kHeight = 3,
	kWidth = 4,
	kMipMapCount = 7,
	kPfSize = 19,
	kPfFourCC = 21,
	kCaps2 = 28,
	kHeaderEnd = 32, // 4 + 124 bytes
	kDxgiFormat = 32,
	kResourceDimension = 33,
	kHeader10End = 37
};

constexpr uint32_t four_cc(char a, char b, char c, char d)
{
	return (uint32_t)(uint8_t)a | (uint32_t)(uint8_t)b << 8 | (uint32_t)(uint8_t)c << 16 | (uint32_t)(uint8_t)d << 24;
}

// getFormat, src/textures.cpp:82-127 (the SRGB spellings name the same UNORM view); 0: undefined
uint32_t dds_format(uint32_t fourCC, uint32_t dxgi)
{
	if (fourCC == four_cc('D', 'X', 'T', '1'))
		return NV_FORMAT_BC1;
	if (fourCC == four_cc('D', 'X', 'T', '3'))
		return NV_FORMAT_BC2;
	if (fourCC == four_cc('D', 'X', 'T', '5'))
		return NV_FORMAT_BC3;
	if (fourCC == four_cc('A', 'T', 'I', '1'))
		return NV_FORMAT_BC4;
	if (fourCC == four_cc('A', 'T', 'I', '2'))
		return NV_FORMAT_BC5;
	if (fourCC != four_cc('D', 'X', '1', '0'))
		return 0;
	switch (dxgi)
	{
	case 71: case 72: return NV_FORMAT_BC1;
	case 74: case 75: return NV_FORMAT_BC2;
	case 77: case 78: return NV_FORMAT_BC3;
	case 80: case 81: return NV_FORMAT_BC4;
	case 83: case 84: return NV_FORMAT_BC5;
	case 95: case 96: return NV_FORMAT_BC6H;
	case 98: case 99: return NV_FORMAT_BC7;
	}
	return 0;
}

bool shape_ok(uint32_t width, uint32_t height, uint32_t levels)
{
	return width && height && levels && width <= nv::TX_MAX_SIDE && height <= nv::TX_MAX_SIDE && levels <= nv::TX_MAX_LEVELS;
}

uint64_t level_blocks(uint32_t width, uint32_t height, uint32_t level)
{
	return (uint64_t)((nv::tx_level_side(width, level) + 3u) / 4u) * ((nv::tx_level_side(height, level) + 3u) / 4u);
}
} // namespace

extern "C" {

int nv_dds_parse(const void* bytes, uint64_t size, NvDdsInfo* out)
{
	if (!bytes || !out)
		return NV_EINVAL;
	memset(out, 0, sizeof(*out));
	uint32_t w[kHeader10End] = {};
	if (size < kHeaderEnd * 4u)
		return NV_EFORMAT; // :168,172
	memcpy(w, bytes, kHeaderEnd * 4u);
	if (w[0] != four_cc('D', 'D', 'S', ' '))
		return NV_EFORMAT; // :168
	const bool dx10 = w[kPfFourCC] == four_cc('D', 'X', '1', '0');
	if (dx10)
	{
		if (size < kHeader10End * 4u)
			return NV_EFORMAT; // :176
		memcpy(w, bytes, kHeader10End * 4u);
	}
	if (w[kSize] != 124u || w[kPfSize] != 32u)
		return NV_EFORMAT; // :179
	if (w[kCaps2] & (0x200u | 0x200000u))
		return NV_EFORMAT; // :182 cube map, volume
	if (dx10 && w[kResourceDimension] != 3u)
		return NV_EFORMAT; // :185
	const uint32_t format = dds_format(w[kPfFourCC], w[kDxgiFormat]);
	if (!format)
		return NV_EFORMAT; // :189
	const uint32_t width = w[kWidth], height = w[kHeight], levels = w[kMipMapCount];
	if (!shape_ok(width, height, levels))
		return NV_EFORMAT;
	out->format = format;
	out->width = width, out->height = height, out->levels = levels;
	out->blockBytes = nv::tx_block_bytes(format);
	out->payloadOffset = (dx10 ? kHeader10End : kHeaderEnd) * 4u;
	uint64_t off = 0;
	for (uint32_t l = 0; l < levels; ++l)
	{
		out->levelOffset[l] = off;
		off += level_blocks(width, height, l) * out->blockBytes;
	}
	out->payloadBytes = off;
	if (size - out->payloadOffset != off)
		return NV_EFORMAT; // :203 short read, :206 bytes behind the payload
	return NV_OK;
}

int nv_texture_set_layout(const NvDdsInfo* infos, uint32_t count, NvTextureDesc* descs, uint64_t* texelWords)
{
	if ((count && !infos) || !descs || !texelWords)
		return NV_EINVAL;
	descs[0] = NvTextureDesc{ 0u, 0u, 0u, 0u };
	uint64_t words = 0;
	for (uint32_t i = 0; i < count; ++i)
	{
		const NvDdsInfo& t = infos[i];
		if (!shape_ok(t.width, t.height, t.levels))
			return NV_EINVAL;
		if (!nv::tx_decodable(t.format))
			return t.format == NV_FORMAT_BC4 || t.format == NV_FORMAT_BC5 || t.format == NV_FORMAT_BC6H ? NV_ETEXFORMAT : NV_EINVAL;
		descs[i + 1] = NvTextureDesc{ (uint32_t)words, t.width, t.height, t.levels };
		words += nv::tx_chain_words(t.width, t.height, t.levels);
		if (words >> 32)
			return NV_EINVAL;
	}
	*texelWords = words;
	return NV_OK;
}

int nv_texture_decode_host(const NvDdsInfo* info, const void* blocks, const NvTextureDesc* desc, uint32_t* texels, uint64_t texelWords)
{
	if (!info || !blocks || !desc || !texels || !shape_ok(info->width, info->height, info->levels))
		return NV_EINVAL;
	if (!nv::tx_decodable(info->format))
		return info->format == NV_FORMAT_BC4 || info->format == NV_FORMAT_BC5 || info->format == NV_FORMAT_BC6H ? NV_ETEXFORMAT : NV_EINVAL;
	const nv::TxDesc d = { desc->offset, desc->width, desc->height, desc->levels };
	if (d.width != info->width || d.height != info->height || d.levels != info->levels || !nv::tx_desc_ok(d, texelWords))
		return NV_EINVAL;
	const uint32_t blockBytes = nv::tx_block_bytes(info->format);
	const uint8_t* src = static_cast<const uint8_t*>(blocks);
	uint32_t* dst = texels + d.offset;
	for (uint32_t l = 0; l < d.levels; ++l)
	{
		const uint32_t w = nv::tx_level_side(d.width, l), h = nv::tx_level_side(d.height, l), bw = (w + 3u) / 4u, bh = (h + 3u) / 4u;
		for (uint32_t by = 0; by < bh; ++by)
			for (uint32_t bx = 0; bx < bw; ++bx, src += blockBytes)
			{
				uint64_t lo = 0, hi = 0;
				memcpy(&lo, src, 8);
				if (blockBytes == 16u)
					memcpy(&hi, src + 8, 8);
				for (uint32_t t = 0; t < 16u; ++t)
				{
					const uint32_t x = bx * 4u + (t & 3u), y = by * 4u + (t >> 2);
					if (x < w && y < h)
						dst[(size_t)y * w + x] = nv::tx_decode_texel(info->format, lo, hi, t);
				}
			}
		dst += (size_t)w * h;
	}
	return NV_OK;
}

int nv_texture_sample_host(const NvTextureDesc* descs, uint32_t textureCount, const uint32_t* texels, uint64_t texelWords, uint32_t id,
                           const float uv[2], const float duvdx[2], const float duvdy[2], float out_rgba[4])
{
	if (!descs || !texels || !uv || !duvdx || !duvdy || !out_rgba || id == 0u || id >= textureCount)
		return NV_EINVAL;
	const nv::TxDesc d = { descs[id].offset, descs[id].width, descs[id].height, descs[id].levels };
	if (!nv::tx_desc_ok(d, texelWords))
		return NV_EINVAL;
	const nv::TxF4 c = nv::tx_sample(texels, d, uv[0], uv[1], duvdx[0], duvdx[1], duvdy[0], duvdy[1]);
	out_rgba[0] = c.x, out_rgba[1] = c.y, out_rgba[2] = c.z, out_rgba[3] = c.w;
	return NV_OK;
}

// ---- block-resident sets
int nv_texture_block_layout(const NvDdsInfo* infos, uint32_t count, NvTextureBlockDesc* descs, uint64_t* units16)
{
	if ((count && !infos) || !descs || !units16)
		return NV_EINVAL;
	descs[0] = NvTextureBlockDesc{ 0u, 0u, 0u, 0u };
	uint64_t units = 0;
	for (uint32_t i = 0; i < count; ++i)
	{
		const NvDdsInfo& t = infos[i];
		if (!shape_ok(t.width, t.height, t.levels))
			return NV_EINVAL;
		if (!nv::tx_decodable(t.format))
			return t.format == NV_FORMAT_BC4 || t.format == NV_FORMAT_BC5 || t.format == NV_FORMAT_BC6H ? NV_ETEXFORMAT : NV_EINVAL;
		descs[i + 1] = NvTextureBlockDesc{ (uint32_t)units, t.width, t.height, t.levels | t.format << 8 };
		units += (nv::tx_chain_block_bytes(t.width, t.height, t.levels, t.format) + 15u) / 16u; // == payloadBytes rounded up (nv_dds_parse)
		if (units >> 32)
			return NV_EINVAL;
	}
	*units16 = units;
	return NV_OK;
}

int nv_texture_block_fetch_host(const NvTextureBlockDesc* desc, const void* blocks, uint64_t units16, uint32_t level, uint32_t x, uint32_t y, uint32_t* rgba)
{
	if (!desc || !blocks || !rgba)
		return NV_EINVAL;
	const nv::TxBlockDesc d = { desc->offset, desc->width, desc->height, desc->levelsFormat };
	if (!nv::tx_block_desc_ok(d, units16))
		return NV_EINVAL;
	const nv::TxBlockSource src = nv::tx_block_source(blocks, d);
	if (level >= src.levels || x >= nv::tx_level_side(src.width, level) || y >= nv::tx_level_side(src.height, level))
		return NV_EINVAL;
	*rgba = src.fetch(level, x, y);
	return NV_OK;
}

int nv_texture_block_sample_host(const NvTextureBlockDesc* descs, uint32_t textureCount, const void* blocks, uint64_t units16, uint32_t id,
                                 const float uv[2], const float duvdx[2], const float duvdy[2], float out_rgba[4])
{
	if (!descs || !blocks || !uv || !duvdx || !duvdy || !out_rgba || id == 0u || id >= textureCount)
		return NV_EINVAL;
	const nv::TxBlockDesc d = { descs[id].offset, descs[id].width, descs[id].height, descs[id].levelsFormat };
	if (!nv::tx_block_desc_ok(d, units16))
		return NV_EINVAL;
	const nv::TxF4 c = nv::tx_sample(nv::tx_block_source(blocks, d), uv[0], uv[1], duvdx[0], duvdx[1], duvdy[0], duvdy[1]);
	out_rgba[0] = c.x, out_rgba[1] = c.y, out_rgba[2] = c.z, out_rgba[3] = c.w;
	return NV_OK;
}

int nv_texture_block_decode_host(uint32_t format, uint64_t lo, uint64_t hi, uint32_t out_alpha[16], uint32_t out_split[16])
{
	if (!nv::tx_decodable(format) || !out_alpha || !out_split)
		return NV_EINVAL;
	const nv::TxBc7Header h = nv::tx_bc7_header(lo, hi);
	for (uint32_t t = 0; t < 16u; ++t)
	{
		out_alpha[t] = nv::tx_decode_alpha(format, lo, hi, t);
		out_split[t] = format == NV_FORMAT_BC7 ? nv::tx_bc7_texel_h(lo, hi, h, t) : nv::tx_decode_texel(format, lo, hi, t);
	}
	return NV_OK;
}

int nv_scenecache_texture_paths(const char* path, const NvSceneCacheInfo* info, char (*paths)[256])
{
	if (!path || !info || (info->texturePathCount && !paths))
		return NV_EINVAL;
	if (!info->texturePathCount)
		return NV_OK;
	const uint64_t bytes = (uint64_t)info->texturePathCount * 256u;
	// the header and the sections nv_scenecache_info sized lie in front of the records
	if (info->fileSize < info->drawOffset || info->fileSize - info->drawOffset < bytes)
		return NV_EFORMAT;
	FILE* f = fopen(path, "rb");
	if (!f)
		return NV_EIO;
	int rc = NV_OK;
	if (fseek(f, 0, SEEK_END) != 0 || (uint64_t)ftell(f) != info->fileSize)
		rc = NV_EFORMAT; // not the file `info` describes
	else if (fseek(f, (long)(info->fileSize - bytes), SEEK_SET) != 0 || fread(paths, 1, bytes, f) != bytes)
		rc = NV_EIO;
	fclose(f);
	if (rc == NV_OK)
		for (uint32_t i = 0; i < info->texturePathCount; ++i)
			paths[i][255] = 0;
	return rc;
}

} // extern "C"
