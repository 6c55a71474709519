// rt_alpha_check.cpp — a stand-alone host program over niagara_amd/csrc/rtbuild.cpp: builds the textured scene blob of a
// small instanced scene, checks it against nv_rt_scene_build's, feeds the validator patched flag words, and walks the blob with
// nv_rt_scene_trace_host_textured_rays over hostile inputs — random bits in the triangles' texcoord words, descriptors that point past the texel
// buffer, counts of zero, indices out of range — with every caller's buffer allocated at its exact size.  It has no device code and is meant to be
// built with the host sanitizers, which turn a load outside a buffer into an error:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I include
//       tools/rt_alpha_check.cpp niagara_amd/csrc/rtbuild.cpp -o rt_alpha_check && ./rt_alpha_check
// Exit status 0 and "rt_alpha_check: ok" when everything holds.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/niagara_vis.h"
#include "../niagara_amd/csrc/rtmath.h"

static uint16_t half_bits(float f) // the values used here (multiples of 0.25 up to 2) are exact in fp16
{
	uint32_t u;
	memcpy(&u, &f, 4);
	const uint32_t s = (u >> 16) & 0x8000u;
	if ((u & 0x7fffffffu) == 0)
		return (uint16_t)s;
	const int e = (int)((u >> 23) & 255u) - 127 + 15;
	return (uint16_t)(s | (uint32_t)e << 10 | ((u >> 13) & 1023u));
}

static uint32_t g_rng = 2468u;
static uint32_t rnd32()
{
	g_rng = g_rng * 1664525u + 1013904223u;
	return g_rng;
}
static float rnd() { return (float)(rnd32() >> 8) * (1.0f / 16777216.0f); } // [0, 1)

#define CHECK(c)                                                       \
	do                                                                 \
	{                                                                  \
		if (!(c))                                                      \
		{                                                              \
			fprintf(stderr, "rt_alpha_check: %s:%d: %s\n", __FILE__, __LINE__, #c); \
			return 1;                                                  \
		}                                                              \
	} while (0)

int main()
{
	// a closed box [-1, 1]^3 with texcoords
	std::vector<NvVertex> vertices(8);
	for (int i = 0; i < 8; ++i)
	{
		memset(&vertices[i], 0, sizeof(NvVertex));
		vertices[i].vx = half_bits(i & 1 ? 1.0f : -1.0f), vertices[i].vy = half_bits(i & 2 ? 1.0f : -1.0f), vertices[i].vz = half_bits(i & 4 ? 1.0f : -1.0f);
		vertices[i].tu = half_bits(0.25f * (float)i - 1.0f), vertices[i].tv = half_bits(i & 2 ? 1.75f : -0.5f);
	}
	const uint32_t box[36] = { 0, 1, 3, 0, 3, 2, 4, 6, 7, 4, 7, 5, 0, 4, 5, 0, 5, 1, 2, 3, 7, 2, 7, 6, 0, 2, 6, 0, 6, 4, 1, 5, 7, 1, 7, 3 };
	std::vector<uint32_t> indices(box, box + 36);
	NvMesh mesh;
	memset(&mesh, 0, sizeof(mesh));
	mesh.vertexCount = 8, mesh.lodCount = 1, mesh.lods[0].indexCount = 36;

	const uint32_t materialCount = 5, textureCount = 4;
	std::vector<NvMeshDraw> draws(24);
	for (size_t i = 0; i < draws.size(); ++i)
	{
		NvMeshDraw& d = draws[i];
		memset(&d, 0, sizeof(d));
		float q[4], l = 0;
		for (int k = 0; k < 4; ++k)
			q[k] = rnd() * 2.0f - 1.0f, l += q[k] * q[k];
		for (int k = 0; k < 4; ++k)
			d.orientation[k] = q[k] / sqrtf(l);
		for (int k = 0; k < 3; ++k)
			d.position[k] = (rnd() * 2.0f - 1.0f) * 8.0f;
		d.scale = 0.5f + rnd() * 3.0f;
		d.postPass = i % 4 == 3 ? 0u : 1u;
		d.materialIndex = (uint32_t)(i % (materialCount + 1)); // one past the table among them
	}
	std::vector<NvMaterial> materials(materialCount);
	memset(materials.data(), 0, materials.size() * sizeof(NvMaterial));
	materials[0].albedoTexture = 1, materials[1].albedoTexture = 2, materials[2].albedoTexture = 3, materials[3].albedoTexture = 0, materials[4].albedoTexture = 9;
	// the set: 5 x 3 with two levels (15 + 2 words), 1 x 1, 4 x 4; exactly 34 words
	std::vector<NvTextureDesc> textures(textureCount);
	textures[0] = NvTextureDesc{ 0, 0, 0, 0 };
	textures[1] = NvTextureDesc{ 0, 5, 3, 2 };
	textures[2] = NvTextureDesc{ 17, 1, 1, 1 };
	textures[3] = NvTextureDesc{ 18, 4, 4, 1 };
	std::vector<uint32_t> texels(34);
	for (uint32_t& t : texels)
		t = (rnd32() & 0x00ffffffu) | ((rnd32() & 1u) ? 0xff000000u : 0u);

	const uint32_t drawCount = (uint32_t)draws.size();
	uint64_t bytes = 0, plainBytes = 0;
	CHECK(nv_rt_scene_build_textured(&mesh, 1, indices.data(), 36, vertices.data(), 8, draws.data(), drawCount, nullptr, &bytes) == NV_OK);
	CHECK(nv_rt_scene_build(&mesh, 1, indices.data(), 36, vertices.data(), 8, draws.data(), drawCount, nullptr, &plainBytes) == NV_OK && plainBytes == bytes);
	void* blob = aligned_alloc(16, (size_t)bytes);
	void* plain = aligned_alloc(16, (size_t)bytes);
	void* work = aligned_alloc(16, (size_t)bytes);
	CHECK(blob && plain && work);
	uint64_t room = bytes;
	CHECK(nv_rt_scene_build_textured(&mesh, 1, indices.data(), 36, vertices.data(), 8, draws.data(), drawCount, blob, &room) == NV_OK && room == bytes);
	room = bytes;
	CHECK(nv_rt_scene_build(&mesh, 1, indices.data(), 36, vertices.data(), 8, draws.data(), drawCount, plain, &room) == NV_OK);
	room = bytes - 16;
	CHECK(nv_rt_scene_build_textured(&mesh, 1, indices.data(), 36, vertices.data(), 8, draws.data(), drawCount, work, &room) == NV_EINVAL);
	const nv::RtHeader* h = static_cast<const nv::RtHeader*>(blob);
	CHECK(h->flags == nv::RT_FLAG_TEXCOORDS && static_cast<const nv::RtHeader*>(plain)->flags == 0u && h->triangles == 12);

	// the textured blob with its flag and its w words zeroed is the plain blob
	memcpy(work, blob, (size_t)bytes);
	static_cast<nv::RtHeader*>(work)->flags = 0u;
	uint32_t* w = reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(work) + h->triOff);
	uint32_t nonzero = 0;
	for (uint32_t c = 0; c < h->triangles * 3u; ++c)
		nonzero += w[4u * c + 3u] != 0u, w[4u * c + 3u] = 0u;
	CHECK(nonzero > 0 && memcmp(work, plain, (size_t)bytes) == 0);

	// the validator: bit 0 alone
	for (uint32_t bit = 0; bit < 32; ++bit)
	{
		memcpy(work, blob, (size_t)bytes);
		static_cast<nv::RtHeader*>(work)->flags = 1u << bit;
		CHECK((nv_rt_scene_validate(work, bytes) == NV_OK) == (bit == 0));
		static_cast<nv::RtHeader*>(work)->flags = 1u | 1u << bit;
		CHECK((nv_rt_scene_validate(work, bytes) == NV_OK) == (bit == 0));
	}
	CHECK(nv_rt_scene_validate(blob, bytes) == NV_OK && nv_rt_scene_validate(plain, bytes) == NV_OK);

	// rays
	const uint64_t rays = 4000;
	std::vector<float> origins(rays * 3), dirs(rays * 3);
	for (uint64_t r = 0; r < rays; ++r)
		for (int k = 0; k < 3; ++k)
			origins[3 * r + k] = (rnd() * 2.0f - 1.0f) * 12.0f, dirs[3 * r + k] = rnd() * 2.0f - 1.0f;
	std::vector<uint8_t> base(rays), opaque(rays), out(rays);
	const float tmin = 1e-2f, tmax = 1e3f;
	CHECK(nv_rt_scene_trace_host_textured_rays(blob, origins.data(), dirs.data(), rays, tmin, tmax, 1, draws.data(), drawCount, materials.data(), materialCount,
	                                           textures.data(), textureCount, texels.data(), texels.size(), base.data()) == NV_OK);
	CHECK(nv_rt_scene_trace_host_rays(blob, origins.data(), dirs.data(), rays, tmin, tmax, 1, opaque.data()) == NV_OK);
	uint32_t lit = 0, dark = 0, opened = 0;
	for (uint64_t r = 0; r < rays; ++r)
	{
		CHECK(base[r] == 0 || base[r] == 255);
		CHECK(!(base[r] == 0 && opaque[r] == 255)); // the alpha test only ever lights a ray
		lit += base[r] == 255, dark += base[r] == 0, opened += base[r] != opaque[r];
	}
	CHECK(lit > 100 && dark > 100 && opened > 20);
	// quality 0 is the plain traversal's; refusals
	CHECK(nv_rt_scene_trace_host_textured_rays(blob, origins.data(), dirs.data(), rays, tmin, tmax, 0, draws.data(), drawCount, materials.data(), materialCount,
	                                           textures.data(), textureCount, texels.data(), texels.size(), out.data()) == NV_OK);
	CHECK(nv_rt_scene_trace_host_rays(blob, origins.data(), dirs.data(), rays, tmin, tmax, 0, opaque.data()) == NV_OK && memcmp(out.data(), opaque.data(), rays) == 0);
	CHECK(nv_rt_scene_trace_host_textured_rays(plain, origins.data(), dirs.data(), rays, tmin, tmax, 1, draws.data(), drawCount, materials.data(), materialCount,
	                                           textures.data(), textureCount, texels.data(), texels.size(), out.data()) == NV_EINVAL);
	CHECK(nv_rt_scene_trace_host_textured_rays(blob, origins.data(), dirs.data(), rays, tmin, tmax, 1, nullptr, drawCount, materials.data(), materialCount,
	                                           textures.data(), textureCount, texels.data(), texels.size(), out.data()) == NV_EINVAL);
	CHECK(nv_rt_scene_trace_host_textured_rays(blob, origins.data(), dirs.data(), rays, tmin, tmax, 2, draws.data(), drawCount, materials.data(), materialCount,
	                                           textures.data(), textureCount, texels.data(), texels.size(), out.data()) == NV_EINVAL);

	// zero counts: every instance is opaque
	CHECK(nv_rt_scene_trace_host_rays(blob, origins.data(), dirs.data(), rays, tmin, tmax, 1, opaque.data()) == NV_OK);
	CHECK(nv_rt_scene_trace_host_textured_rays(blob, origins.data(), dirs.data(), rays, tmin, tmax, 1, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, out.data()) == NV_OK &&
	      memcmp(out.data(), opaque.data(), rays) == 0);
	CHECK(nv_rt_scene_trace_host_textured_rays(blob, origins.data(), dirs.data(), rays, tmin, tmax, 1, draws.data(), drawCount, materials.data(), materialCount,
	                                           textures.data(), textureCount, texels.data(), 0, out.data()) == NV_OK && memcmp(out.data(), opaque.data(), rays) == 0);

	// hostile descriptors over a texel buffer of its exact size: whatever a descriptor says, nothing outside the buffer is loaded
	uint32_t absent = 0;
	for (int round = 0; round < 300; ++round)
	{
		std::vector<NvTextureDesc> bad(textures);
		for (uint32_t t = 1; t < textureCount; ++t)
		{
			NvTextureDesc& d = bad[t];
			switch (rnd32() % 6u)
			{
			case 0: d.offset = rnd32(); break;
			case 1: d.width = rnd32() % 3u ? rnd32() % 40000u : rnd32(); break;
			case 2: d.height = rnd32() % 3u ? rnd32() % 40000u : rnd32(); break;
			case 3: d.levels = rnd32() % 20u; break;
			case 4: d.offset = (uint32_t)texels.size() - rnd32() % 4u, d.width = 1u + rnd32() % 3u, d.height = 1u + rnd32() % 3u, d.levels = 1u + rnd32() % 2u; break;
			default: d = NvTextureDesc{ rnd32(), rnd32(), rnd32(), rnd32() }; break;
			}
		}
		// each round gets a fresh heap copy of exactly the words the call is told about
		const uint64_t words = round % 3 == 0 ? texels.size() : rnd32() % (texels.size() + 1u);
		uint32_t* exact = words ? static_cast<uint32_t*>(malloc((size_t)words * 4u)) : nullptr;
		if (words)
			memcpy(exact, texels.data(), (size_t)words * 4u);
		CHECK(nv_rt_scene_trace_host_textured_rays(blob, origins.data(), dirs.data(), 400, tmin, tmax, 1, draws.data(), drawCount, materials.data(), materialCount,
		                                           bad.data(), textureCount, exact, words, out.data()) == NV_OK);
		for (uint64_t r = 0; r < 400; ++r)
			absent += out[r] != base[r];
		free(exact);
	}
	CHECK(absent > 0); // some of them changed what the rays saw

	// hostile texcoords: random bits, infinities and NaNs in the w words
	for (int round = 0; round < 40; ++round)
	{
		memcpy(work, blob, (size_t)bytes);
		for (uint32_t c = 0; c < h->triangles * 3u; ++c)
		{
			const uint32_t pick = rnd32() % 4u;
			w[4u * c + 3u] = pick == 0 ? rnd32() : pick == 1 ? 0x7c00fc00u : pick == 2 ? 0x7e007fffu : (w[4u * c + 3u] ^ (1u << (rnd32() % 32u)));
		}
		CHECK(nv_rt_scene_validate(work, bytes) == NV_OK);
		CHECK(nv_rt_scene_trace_host_textured_rays(work, origins.data(), dirs.data(), 1000, tmin, tmax, 1, draws.data(), drawCount, materials.data(), materialCount,
		                                           textures.data(), textureCount, texels.data(), texels.size(), out.data()) == NV_OK);
		for (uint64_t r = 0; r < 1000; ++r)
			CHECK((out[r] == 0 || out[r] == 255) && !(out[r] == 0 && opaque[r] == 255));
	}

	// the host TLAS rebuild keeps the flag and the texcoords
	for (NvMeshDraw& d : draws)
		d.position[0] += 1.5f;
	uint64_t rebuilt = 0;
	CHECK(nv_rt_tlas_build_host(blob, bytes, draws.data(), drawCount, nullptr, &rebuilt) == NV_OK);
	void* moved = aligned_alloc(16, (size_t)rebuilt);
	CHECK(moved);
	room = rebuilt;
	CHECK(nv_rt_tlas_build_host(blob, bytes, draws.data(), drawCount, moved, &room) == NV_OK && nv_rt_scene_validate(moved, room) == NV_OK);
	const nv::RtHeader* mh = static_cast<const nv::RtHeader*>(moved);
	CHECK(mh->flags == nv::RT_FLAG_TEXCOORDS && mh->triangles == h->triangles);
	CHECK(memcmp(static_cast<unsigned char*>(moved) + mh->triOff, static_cast<unsigned char*>(blob) + h->triOff, (size_t)h->triangles * 48u) == 0);
	CHECK(nv_rt_scene_trace_host_textured_rays(moved, origins.data(), dirs.data(), rays, tmin, tmax, 1, draws.data(), drawCount, materials.data(), materialCount,
	                                           textures.data(), textureCount, texels.data(), texels.size(), out.data()) == NV_OK);

	// the four-tap alpha against the full sampler, uv of every kind
	const float special[] = { 0.0f, -0.0f, 1.0f, -1.0f, 1e-45f, -1e-45f, -1e-8f, 0.999999f, 1e30f, -1e30f, INFINITY, -INFINITY, NAN, 123456.78f, -0.3333f };
	const size_t ns = sizeof(special) / sizeof(special[0]);
	std::vector<float> uv, a(ns * ns), b(ns * ns);
	for (size_t i = 0; i < ns; ++i)
		for (size_t j = 0; j < ns; ++j)
			uv.push_back(special[i]), uv.push_back(special[j]);
	for (uint32_t t = 1; t < textureCount; ++t)
	{
		CHECK(nv_rt_alpha_sample_host(&textures[t], texels.data(), texels.size(), uv.data(), ns * ns, a.data(), b.data()) == NV_OK);
		for (size_t i = 0; i < ns * ns; ++i) // bit for bit; a NaN for a NaN (which NaN an operation hands on is the compiler's choice of operand order)
			CHECK(isnan(b[i]) ? isnan(a[i]) != 0 : memcmp(&a[i], &b[i], 4) == 0);
	}
	NvTextureDesc past = { 33, 2, 1, 1 };
	CHECK(nv_rt_alpha_sample_host(&past, texels.data(), texels.size(), uv.data(), ns * ns, a.data(), b.data()) == NV_EINVAL);

	free(blob);
	free(plain);
	free(work);
	free(moved);
	printf("rt_alpha_check: ok (%u lit, %u dark, %u lit by the alpha test, %u rays changed by hostile descriptors)\n", lit, dark, opened, absent);
	return 0;
}
