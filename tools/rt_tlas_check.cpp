// rt_tlas_check.cpp — a stand-alone host program over niagara_amd/csrc/rtbuild.cpp: rebuilds the TLAS of a small instanced
// scene with nv_rt_tlas_build_host over the edge counts (0, 1, 2, 3 casters), duplicate keys (every instance with one transform), two far
// clusters, an instance with the infinite box and every kind of draw that does not cast; validates each blob, checks the layout rules and
// walks it with nv_rt_scene_trace_host against an all-triangles loop over the same triangle test.  No device code; meant for the host
// sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I include
//       tools/rt_tlas_check.cpp niagara_amd/csrc/rtbuild.cpp -o rt_tlas_check && ./rt_tlas_check
// Exit status 0 and "rt_tlas_check: ok" when everything holds.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/niagara_vis.h"
#include "../niagara_amd/csrc/rtmath.h"

static uint16_t half_bits(float f) // +-1 only
{
	return f < 0.0f ? 0xbc00u : 0x3c00u;
}

static uint32_t g_rng = 2468u;
static float rnd() // [0, 1)
{
	g_rng = g_rng * 1664525u + 1013904223u;
	return (float)(g_rng >> 8) * (1.0f / 16777216.0f);
}

#define CHECK(c)                                                      \
	do                                                                \
	{                                                                 \
		if (!(c))                                                     \
		{                                                             \
			fprintf(stderr, "rt_tlas_check: %s:%d: %s\n", __FILE__, __LINE__, #c); \
			return 1;                                                 \
		}                                                             \
	} while (0)

static const uint32_t BOX[36] = { 0, 1, 3, 0, 3, 2, 4, 6, 7, 4, 7, 5, 0, 4, 5, 0, 5, 1, 2, 3, 7, 2, 7, 6, 0, 2, 6, 0, 6, 4, 1, 5, 7, 1, 7, 3 };

static bool casts(const NvMeshDraw& d, int quality)
{
	bool finite = isfinite(d.scale);
	for (int k = 0; k < 3; ++k)
		finite = finite && isfinite(d.position[k]);
	for (int k = 0; k < 4; ++k)
		finite = finite && isfinite(d.orientation[k]);
	return d.meshIndex == 0 && finite && d.scale > 0.0f && d.postPass <= (uint32_t)quality;
}

// rebuild, validate, check the layout, trace against the brute force; returns the number of occluded rays or -1
static long check_rebuild(const void* blob, uint64_t bytes, const std::vector<NvMeshDraw>& draws, uint32_t expectInstances, uint32_t rays)
{
	uint64_t need = 0;
	const NvMeshDraw* dp = draws.empty() ? nullptr : draws.data();
	if (nv_rt_tlas_build_host(blob, bytes, dp, (uint32_t)draws.size(), nullptr, &need) != NV_OK || need < 64 || need % 16)
		return -1;
	void* out = aligned_alloc(16, (size_t)need);
	void* again = aligned_alloc(16, (size_t)need);
	long result = -1;
	do
	{
		if (!out || !again)
			break;
		uint64_t room = need;
		if (nv_rt_tlas_build_host(blob, bytes, dp, (uint32_t)draws.size(), out, &room) != NV_OK || room != need)
			break;
		room = need;
		if (nv_rt_tlas_build_host(out, need, dp, (uint32_t)draws.size(), again, &room) != NV_OK || room != need || memcmp(out, again, (size_t)need))
			break; // a rebuild from a rebuilt blob: the same bytes
		room = need - 16;
		if (nv_rt_tlas_build_host(blob, bytes, dp, (uint32_t)draws.size(), again, &room) != NV_EINVAL)
			break;
		if (nv_rt_scene_validate(out, need) != NV_OK)
			break;
		NvRtSceneStats st;
		if (nv_rt_scene_stats(out, need, &st) != NV_OK || st.instances != expectInstances || st.tlasLeaves != expectInstances ||
		    st.tlasNodes != (expectInstances ? 2 * expectInstances - 1 : 0) || (expectInstances && st.tlasMaxLeaf != 1))
			break;
		const nv::RtHeader* h = static_cast<const nv::RtHeader*>(out);
		const nv::RtNode* nodes = reinterpret_cast<const nv::RtNode*>(static_cast<const unsigned char*>(out) + h->tlasOff);
		bool ok = h->drawCount == draws.size();
		for (uint32_t i = 0; i < h->tlasNodes && ok; ++i)
			if (nodes[i].leaf == 0) // an inner box is exactly the min / max of its children's
			{
				const nv::RtNode &a = nodes[i + 1], &b = nodes[nodes[i + 1].skip];
				for (int k = 0; k < 3; ++k)
					ok = ok && nodes[i].lo[k] == fminf(a.lo[k], b.lo[k]) && nodes[i].hi[k] == fmaxf(a.hi[k], b.hi[k]);
				ok = ok && b.skip == nodes[i].skip;
			}
		if (!ok)
			break;
		long hits = 0;
		for (uint32_t r = 0; r < rays && ok; ++r)
		{
			float o[3], d[3];
			for (int k = 0; k < 3; ++k)
				o[k] = (rnd() * 2.0f - 1.0f) * 25.0f, d[k] = rnd() * 2.0f - 1.0f;
			if (r % 5 == 0)
				d[r % 3] = 0.0f;
			if (r % 97 == 0)
				o[r % 3] = r % 2 ? NAN : INFINITY;
			for (int quality = 0; quality < 2 && ok; ++quality)
			{
				bool want = false;
				const bool finite = isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]);
				for (size_t i = 0; i < draws.size() && !want && finite; ++i)
				{
					if (!casts(draws[i], quality))
						continue;
					nv::rt3 o2, d2;
					nv::rt_object_ray(nv::rt3{ o[0], o[1], o[2] }, nv::rt3{ d[0], d[1], d[2] }, draws[i].position, draws[i].orientation, draws[i].scale, &o2, &d2);
					const nv::RtRay ray = nv::rt_ray_setup(o2, d2);
					for (int t = 0; t < 12 && !want; ++t)
					{
						nv::rt3 v[3];
						for (int k = 0; k < 3; ++k)
						{
							const uint32_t c = BOX[3 * t + k];
							v[k] = nv::rt3{ c & 1 ? 1.0f : -1.0f, c & 2 ? 1.0f : -1.0f, c & 4 ? 1.0f : -1.0f };
						}
						want = nv::rt_triangle(ray, v[0], v[1], v[2], 1e-2f, 1e3f);
					}
				}
				const int got = nv_rt_scene_trace_host(out, o, d, 1e-2f, 1e3f, quality);
				ok = got == (want ? 1 : 0);
				hits += got;
			}
		}
		if (ok)
			result = hits;
	} while (0);
	free(out);
	free(again);
	return result;
}

static NvMeshDraw random_draw(float spread)
{
	NvMeshDraw d;
	memset(&d, 0, sizeof(d));
	float q[4], l = 0;
	for (int k = 0; k < 4; ++k)
		q[k] = rnd() * 2.0f - 1.0f, l += q[k] * q[k];
	for (int k = 0; k < 4; ++k)
		d.orientation[k] = q[k] / sqrtf(l);
	for (int k = 0; k < 3; ++k)
		d.position[k] = (rnd() * 2.0f - 1.0f) * spread;
	d.scale = 0.25f + rnd() * 4.0f;
	return d;
}

int main()
{
	// mesh 0: a closed box [-1, 1]^3; mesh 1: no triangles
	std::vector<NvVertex> vertices(8);
	for (int i = 0; i < 8; ++i)
	{
		memset(&vertices[i], 0, sizeof(NvVertex));
		vertices[i].vx = half_bits(i & 1 ? 1.0f : -1.0f), vertices[i].vy = half_bits(i & 2 ? 1.0f : -1.0f), vertices[i].vz = half_bits(i & 4 ? 1.0f : -1.0f);
	}
	NvMesh meshes[2];
	memset(meshes, 0, sizeof(meshes));
	meshes[0].vertexCount = 8, meshes[0].lodCount = 1, meshes[0].lods[0].indexCount = 36;
	meshes[1].lodCount = 1;
	std::vector<NvMeshDraw> first(5);
	for (size_t i = 0; i < first.size(); ++i)
		first[i] = random_draw(20.0f);
	uint64_t bytes = 0;
	CHECK(nv_rt_scene_build(meshes, 2, BOX, 36, vertices.data(), 8, first.data(), (uint32_t)first.size(), nullptr, &bytes) == NV_OK);
	void* blob = aligned_alloc(16, (size_t)bytes);
	CHECK(blob);
	uint64_t room = bytes;
	CHECK(nv_rt_scene_build(meshes, 2, BOX, 36, vertices.data(), 8, first.data(), (uint32_t)first.size(), blob, &room) == NV_OK && room == bytes);

	// refusals
	uint64_t need = 0;
	CHECK(nv_rt_tlas_build_host(blob, bytes, first.data(), 5, nullptr, nullptr) == NV_EINVAL);
	CHECK(nv_rt_tlas_build_host(blob, bytes, nullptr, 5, nullptr, &need) == NV_EINVAL);
	CHECK(nv_rt_tlas_build_host(blob, bytes - 16, first.data(), 5, nullptr, &need) == NV_EINVAL);
	CHECK(nv_rt_tlas_build_host(nullptr, 0, first.data(), 5, nullptr, &need) == NV_EINVAL);
	CHECK(nv_rt_tlas_build_host(blob, bytes, first.data(), 1u << 29, nullptr, &need) == NV_EINVAL);
	CHECK(nv_rt_tlas_build_host(blob, bytes, first.data(), 5, static_cast<char*>(blob) + 4, &need) == NV_EINVAL);

	// the edge counts
	long total = 0, got;
	for (uint32_t n = 0; n <= 3; ++n)
	{
		std::vector<NvMeshDraw> draws;
		for (uint32_t i = 0; i < n; ++i)
			draws.push_back(random_draw(10.0f));
		CHECK((got = check_rebuild(blob, bytes, draws, n, 3000)) >= 0);
		total += got;
	}
	// duplicate keys: every instance with one transform (the strings differ in their low word only)
	{
		std::vector<NvMeshDraw> draws(37, random_draw(5.0f));
		CHECK((got = check_rebuild(blob, bytes, draws, 37, 3000)) > 0);
		total += got;
	}
	// two clusters far apart, an instance with the infinite box (the singular quaternion), a zero quaternion, and every kind of draw that does not cast
	{
		std::vector<NvMeshDraw> draws;
		for (int i = 0; i < 60; ++i)
		{
			NvMeshDraw d = random_draw(8.0f);
			d.position[0] += i % 2 ? 1.0e6f : -20.0f;
			d.postPass = (uint32_t)(i % 3); // postPass 2 does not cast
			draws.push_back(d);
		}
		for (int k = 0; k < 4; ++k)
			draws[0].orientation[k] = k == 0 ? 0.70710678f : 0.0f, draws[2].orientation[k] = 0.0f; // the singular map (w = 0, |xyz|^2 = 1/2): the
		                                                                                        // infinite box; a zero quaternion is the identity
		draws[1].position[1] = NAN, draws[3].scale = 0.0f, draws[4].meshIndex = 2, draws[6].meshIndex = 1, draws[7].scale = -1.0f, draws[9].orientation[2] = INFINITY;
		// 40 of the 60 have postPass <= 1; 1, 3, 4, 6, 7 and 9 among them leave, 0 stays an instance
		CHECK((got = check_rebuild(blob, bytes, draws, 34, 6000)) > 0);
		total += got;
	}
	// a large random set: deep trees on both sides of every split
	{
		std::vector<NvMeshDraw> draws;
		for (int i = 0; i < 700; ++i)
			draws.push_back(random_draw(25.0f));
		CHECK((got = check_rebuild(blob, bytes, draws, 700, 2000)) > 0);
		total += got;
	}
	free(blob);
	printf("rt_tlas_check: ok (%ld occluded rays)\n", total);
	return 0;
}
