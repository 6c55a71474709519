// rt_scene_check.cpp — a stand-alone host program over niagara_amd/csrc/rtbuild.cpp: builds the scene blob of a small
// instanced scene, validates it, walks it with nv_rt_scene_trace_host against an all-triangles loop over the same triangle test, and feeds
// the validator truncated and patched blobs.  It has no device code and is meant to be built with the host sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I include
//       tools/rt_scene_check.cpp niagara_amd/csrc/rtbuild.cpp -o rt_scene_check && ./rt_scene_check
// Exit status 0 and "rt_scene_check: ok" when everything holds.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/niagara_vis.h"
#include "../niagara_amd/csrc/rtmath.h"

static uint16_t half_bits(float f) // the values used here (multiples of 0.5 up to 2) are exact in fp16
{
	uint32_t u;
	memcpy(&u, &f, 4);
	const uint32_t s = (u >> 16) & 0x8000u;
	if ((u & 0x7fffffffu) == 0)
		return (uint16_t)s;
	const int e = (int)((u >> 23) & 255u) - 127 + 15;
	return (uint16_t)(s | (uint32_t)e << 10 | ((u >> 13) & 1023u));
}

static uint32_t g_rng = 12345u;
static float rnd() // [0, 1)
{
	g_rng = g_rng * 1664525u + 1013904223u;
	return (float)(g_rng >> 8) * (1.0f / 16777216.0f);
}

#define CHECK(c)                                                       \
	do                                                                 \
	{                                                                  \
		if (!(c))                                                      \
		{                                                              \
			fprintf(stderr, "rt_scene_check: %s:%d: %s\n", __FILE__, __LINE__, #c); \
			return 1;                                                  \
		}                                                              \
	} while (0)

int main()
{
	// one mesh: a closed box [-1, 1]^3, 8 vertices, 12 triangles; a second mesh without triangles
	std::vector<NvVertex> vertices(8);
	for (int i = 0; i < 8; ++i)
	{
		memset(&vertices[i], 0, sizeof(NvVertex));
		vertices[i].vx = half_bits(i & 1 ? 1.0f : -1.0f), vertices[i].vy = half_bits(i & 2 ? 1.0f : -1.0f), vertices[i].vz = half_bits(i & 4 ? 1.0f : -1.0f);
	}
	const uint32_t box[36] = { 0, 1, 3, 0, 3, 2, 4, 6, 7, 4, 7, 5, 0, 4, 5, 0, 5, 1, 2, 3, 7, 2, 7, 6, 0, 2, 6, 0, 6, 4, 1, 5, 7, 1, 7, 3 };
	std::vector<uint32_t> indices(box, box + 36);
	indices.push_back(0), indices.push_back(1), indices.push_back(99); // a triangle with a corner past the vertex capacity: left out
	NvMesh meshes[2];
	memset(meshes, 0, sizeof(meshes));
	meshes[0].vertexCount = 8, meshes[0].lodCount = 1, meshes[0].lods[0].indexCount = 39;
	meshes[1].lodCount = 1;

	std::vector<NvMeshDraw> draws(40);
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
			d.position[k] = (rnd() * 2.0f - 1.0f) * 20.0f;
		d.scale = 0.25f + rnd() * 4.0f;
		d.meshIndex = i % 7 == 6 ? 1u : 0u;
		d.postPass = (uint32_t)(i % 3);
	}
	draws[3].scale = 0.0f, draws[4].scale = NAN, draws[5].meshIndex = 9; // non-casters

	uint64_t bytes = 0;
	CHECK(nv_rt_scene_build(meshes, 2, indices.data(), (uint32_t)indices.size(), vertices.data(), 8, draws.data(), (uint32_t)draws.size(), nullptr, &bytes) == NV_OK);
	CHECK(bytes >= 64 && bytes % 16 == 0);
	void* blob = aligned_alloc(16, (size_t)bytes);
	void* again = aligned_alloc(16, (size_t)bytes);
	CHECK(blob && again);
	uint64_t room = bytes;
	CHECK(nv_rt_scene_build(meshes, 2, indices.data(), (uint32_t)indices.size(), vertices.data(), 8, draws.data(), (uint32_t)draws.size(), blob, &room) == NV_OK && room == bytes);
	room = bytes;
	CHECK(nv_rt_scene_build(meshes, 2, indices.data(), (uint32_t)indices.size(), vertices.data(), 8, draws.data(), (uint32_t)draws.size(), again, &room) == NV_OK);
	CHECK(memcmp(blob, again, (size_t)bytes) == 0); // deterministic
	room = bytes - 16;
	CHECK(nv_rt_scene_build(meshes, 2, indices.data(), (uint32_t)indices.size(), vertices.data(), 8, draws.data(), (uint32_t)draws.size(), again, &room) == NV_EINVAL);
	CHECK(nv_rt_scene_validate(blob, bytes) == NV_OK);
	NvRtSceneStats st;
	CHECK(nv_rt_scene_stats(blob, bytes, &st) == NV_OK && st.triangles == 12 && st.blasCount == 1 && st.blasMaxLeaf <= 4 && st.tlasMaxLeaf == 1);

	// the traversal against every triangle of every casting instance, the same T
	uint32_t hits = 0;
	for (int r = 0; r < 20000; ++r)
	{
		float o[3], d[3];
		for (int k = 0; k < 3; ++k)
			o[k] = (rnd() * 2.0f - 1.0f) * 25.0f, d[k] = rnd() * 2.0f - 1.0f;
		if (r % 5 == 0)
			d[r % 3] = 0.0f; // exact zero components
		for (int quality = 0; quality < 2; ++quality)
		{
			bool want = false;
			for (size_t i = 0; i < draws.size() && !want; ++i)
			{
				const NvMeshDraw& dr = draws[i];
				if (dr.meshIndex != 0 || !(dr.scale > 0.0f) || dr.postPass > (uint32_t)quality)
					continue;
				nv::rt3 o2, d2;
				nv::rt_object_ray(nv::rt3{ o[0], o[1], o[2] }, nv::rt3{ d[0], d[1], d[2] }, dr.position, dr.orientation, dr.scale, &o2, &d2);
				const nv::RtRay ray = nv::rt_ray_setup(o2, d2);
				for (int t = 0; t < 12 && !want; ++t)
				{
					nv::rt3 v[3];
					for (int k = 0; k < 3; ++k)
					{
						const uint32_t c = box[3 * t + k];
						v[k] = nv::rt3{ c & 1 ? 1.0f : -1.0f, c & 2 ? 1.0f : -1.0f, c & 4 ? 1.0f : -1.0f };
					}
					want = nv::rt_triangle(ray, v[0], v[1], v[2], 1e-2f, 1e3f);
				}
			}
			const int got = nv_rt_scene_trace_host(blob, o, d, 1e-2f, 1e3f, quality);
			CHECK(got == (want ? 1 : 0));
			hits += (uint32_t)got;
		}
	}
	CHECK(hits > 1000);
	const float nanOrigin[3] = { NAN, 0, 0 }, dir[3] = { 0, 0, 1 };
	CHECK(nv_rt_scene_trace_host(blob, nanOrigin, dir, 1e-2f, 1e3f, 1) == 0);
	CHECK(nv_rt_scene_trace_host(blob, dir, dir, 1e-2f, 1e3f, 2) == NV_EINVAL);

	// the validator: truncation, and every word of the node, table and instance sections set to all ones, one at a time
	CHECK(nv_rt_scene_validate(blob, bytes - 16) == NV_EINVAL);
	CHECK(nv_rt_scene_validate(blob, 32) == NV_EINVAL);
	const nv::RtHeader* h = static_cast<const nv::RtHeader*>(blob);
	uint32_t refused = 0;
	for (uint32_t w = 0; w < h->triOff / 4u; ++w)
	{
		memcpy(again, blob, (size_t)bytes);
		static_cast<uint32_t*>(again)[w] = 0xffffffffu;
		if (nv_rt_scene_validate(again, bytes) != NV_OK)
		{
			++refused;
			continue;
		}
		// what the validator lets through must be safe to walk (under the sanitizers: no read outside the blob, and the loops end)
		const float o[3] = { 30.0f, 1.0f, 2.0f }, d[3] = { -1.0f, 0.01f, 0.02f };
		(void)nv_rt_scene_trace_host(again, o, d, 1e-2f, 1e3f, 1);
	}
	CHECK(refused > 0);

	// zero draws, zero meshes
	room = bytes;
	CHECK(nv_rt_scene_build(nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, again, &room) == NV_OK && nv_rt_scene_validate(again, room) == NV_OK);
	CHECK(nv_rt_scene_trace_host(again, dir, dir, 1e-2f, 1e3f, 1) == 0);
	free(blob);
	free(again);
	printf("rt_scene_check: ok (%u hits, %u patched blobs refused)\n", hits, refused);
	return 0;
}
