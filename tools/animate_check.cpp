// animate_check.cpp — a stand-alone host program over niagara_amd/csrc/host.cpp: the animation validator over every reason
// it refuses for, the scene-cache reader of the three animation sections (a file written here, whole and truncated) and the host twin of
// nv_animate_draws over a small table whose keyframes take every path (one keyframe, the wrap, the linear and the trigonometric branch of
// slerp, the negated quaternion, a skipped animation, a light target, no target).  No device code; meant for the host sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I include
//       tools/animate_check.cpp niagara_amd/csrc/host.cpp -o animate_check && ./animate_check
// Exit status 0 and "animate_check: ok" when everything holds.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/niagara_vis.h"

#define CHECK(c)                                                      \
	do                                                                \
	{                                                                 \
		if (!(c))                                                     \
		{                                                             \
			fprintf(stderr, "animate_check: %s:%d: %s\n", __FILE__, __LINE__, #c); \
			return 1;                                                 \
		}                                                             \
	} while (0)

static NvAnimation anim(int32_t draw, int32_t light, float start, float period, uint32_t offset, uint32_t count)
{
	NvAnimation a = { draw, light, start, period, offset, count };
	return a;
}

static int refusal(const std::vector<NvAnimation>& table, uint32_t keyframes, uint32_t draws, uint32_t lights, uint32_t wantReason, uint32_t wantIndex)
{
	uint32_t reason = 99, index = 99;
	const int rc = nv_animation_validate_host(table.data(), (uint32_t)table.size(), keyframes, draws, lights, &reason, &index);
	CHECK(rc == (wantReason == NV_ANIM_OK ? NV_OK : NV_EINVAL));
	CHECK(reason == wantReason && index == wantIndex);
	return 0;
}

int main(int argc, char** argv)
{
	// ---- the validator, one table per reason (exactly sized vectors: a read past the table is a sanitizer report)
	const NvAnimation good = anim(1, -1, 0.0f, 1.0f, 0, 4);
	std::vector<NvAnimation> t(3, good);
	t[0].drawIndex = 0;
	t[2].drawIndex = 2;
	CHECK(refusal(t, 4, 3, 0, NV_ANIM_OK, 0) == 0);
	CHECK(refusal(std::vector<NvAnimation>(), 0, 0, 0, NV_ANIM_OK, 0) == 0);
	std::vector<NvAnimation> b = t;
	b[1].keyframeCount = 0;
	CHECK(refusal(b, 4, 3, 0, NV_ANIM_NO_KEYFRAMES, 1) == 0);
	b = t;
	b[2].keyframeOffset = 1;
	CHECK(refusal(b, 4, 3, 0, NV_ANIM_KEYFRAME_RANGE, 2) == 0);
	b[2].keyframeOffset = 0xffffffffu; // offset + count wraps in 32 bits
	CHECK(refusal(b, 4, 3, 0, NV_ANIM_KEYFRAME_RANGE, 2) == 0);
	const float periods[4] = { 0.0f, -1.0f, INFINITY, NAN };
	for (int k = 0; k < 4; ++k)
	{
		b = t;
		b[0].period = periods[k];
		CHECK(refusal(b, 4, 3, 0, NV_ANIM_PERIOD, 0) == 0);
	}
	b = t;
	b[1].startTime = NAN;
	CHECK(refusal(b, 4, 3, 0, NV_ANIM_PERIOD, 1) == 0);
	CHECK(refusal(t, 4, 2, 0, NV_ANIM_DRAW_INDEX, 2) == 0);
	b = t;
	b[1].lightIndex = 0;
	CHECK(refusal(b, 4, 3, 0, NV_ANIM_LIGHT_INDEX, 1) == 0);
	CHECK(refusal(b, 4, 3, 1, NV_ANIM_OK, 0) == 0);
	b = t;
	b[2].drawIndex = 0;
	CHECK(refusal(b, 4, 3, 0, NV_ANIM_DUPLICATE_DRAW, 2) == 0);
	b = t;
	b[0].lightIndex = b[1].lightIndex = 3;
	CHECK(refusal(b, 4, 3, 4, NV_ANIM_DUPLICATE_LIGHT, 1) == 0);
	b = t;
	b[0].drawIndex = b[1].drawIndex = b[2].drawIndex = -1; // "no target" is no duplicate
	CHECK(refusal(b, 4, 3, 0, NV_ANIM_OK, 0) == 0);

	// ---- the host twin
	const float h = sqrtf(0.5f);
	std::vector<NvKeyframe> keys;
	const float rot[6][4] = { { 0, 0, 0, 1 }, { 0, h, 0, h }, { 0, -h, 0, -h } /* the same rotation, negated */, { 0, 1, 0, 0 }, { 1e-4f, 0, 0, 1 }, { 0, 0, 0, 1 } };
	for (int k = 0; k < 6; ++k)
	{
		NvKeyframe kf = { { (float)k, 2.0f * k, -1.0f * k }, 1.0f + 0.5f * k, { rot[k][0], rot[k][1], rot[k][2], rot[k][3] } };
		keys.push_back(kf);
	}
	std::vector<NvAnimation> table;
	table.push_back(anim(0, -1, 0.0f, 1.0f, 0, 6));   // walks all six keyframes and wraps
	table.push_back(anim(2, 1, 0.25f, 0.5f, 5, 1));   // one keyframe; a draw and a light
	table.push_back(anim(-1, 0, 0.0f, 2.0f, 1, 3));   // a light alone
	table.push_back(anim(-1, -1, 0.0f, 1.0f, 0, 2));  // neither
	table.push_back(anim(3, -1, 100.0f, 1.0f, 0, 6)); // starts later: skipped below
	std::vector<NvMeshDraw> draws(4);
	std::vector<NvLight> lights(2);
	memset(draws.data(), 0x5a, draws.size() * sizeof(NvMeshDraw));
	memset(lights.data(), 0x5a, lights.size() * sizeof(NvLight));
	const std::vector<NvMeshDraw> draws0 = draws;
	const std::vector<NvLight> lights0 = lights;
	const uint32_t nk = (uint32_t)keys.size(), na = (uint32_t)table.size();
	for (int step = 0; step <= 130; ++step)
	{
		const double time = step * 0.05; // 0 .. 6.5: every interval of animation 0, the wrap 5 -> 0 included
		CHECK(nv_animate_draws_host(time, table.data(), na, keys.data(), nk, draws.data(), 4, lights.data(), 2) == NV_OK);
		CHECK(memcmp(&draws[1], &draws0[1], sizeof(NvMeshDraw)) == 0 && memcmp(&draws[3], &draws0[3], sizeof(NvMeshDraw)) == 0);
		for (int d = 0; d < 4; ++d)
			CHECK(memcmp(&draws[d].meshIndex, &draws0[d].meshIndex, 16) == 0);
		for (int l = 0; l < 2; ++l)
			CHECK(memcmp(&lights[l].range, &lights0[l].range, 20) == 0);
		float norm = 0.0f;
		for (int k = 0; k < 4; ++k)
		{
			CHECK(isfinite(draws[0].orientation[k]));
			norm += draws[0].orientation[k] * draws[0].orientation[k];
		}
		CHECK(fabsf(norm - 1.0f) < 1e-3f || time >= 4.0); // unit keyframes give unit results (the 1e-4 keyframe is not unit)
		CHECK(time < 0.25 || fabsf(draws[2].scale - keys[5].scale) <= 1e-6f * keys[5].scale); // mix(s, s, t) is s up to its two roundings
		if (time >= 0.25)
			CHECK(lights[1].position[0] == draws[2].position[0] && lights[1].position[2] == draws[2].position[2]);
	}
	// the time statements at a keyframe instant and in the wrap
	const uint32_t which[3] = { 0, 0, 4 };
	const double times[3] = { 3.0, 5.5, 1.0 };
	uint8_t skipped[3];
	uint32_t i0[3], i1[3];
	float tt[3];
	CHECK(nv_animation_phase_host(table.data(), which, times, 3, skipped, i0, i1, tt) == NV_OK);
	CHECK(!skipped[0] && i0[0] == 3 && i1[0] == 4 && tt[0] == 0.0f);
	CHECK(!skipped[1] && i0[1] == 5 && i1[1] == 0 && tt[1] == 0.5f);
	CHECK(skipped[2]);
	// refusals of the twin: a non-finite time, a table the validator refuses, NULL arrays (targets skipped, indices still validated)
	CHECK(nv_animate_draws_host(NAN, table.data(), na, keys.data(), nk, draws.data(), 4, lights.data(), 2) == NV_EINVAL);
	CHECK(nv_animate_draws_host(INFINITY, table.data(), na, keys.data(), nk, draws.data(), 4, lights.data(), 2) == NV_EINVAL);
	CHECK(nv_animate_draws_host(1.0, table.data(), na, keys.data(), nk, draws.data(), 3, lights.data(), 2) == NV_EINVAL);
	CHECK(nv_animate_draws_host(1.0, table.data(), na, keys.data(), nk - 1, draws.data(), 4, lights.data(), 2) == NV_EINVAL);
	CHECK(nv_animate_draws_host(1.0, table.data(), na, keys.data(), nk, nullptr, 4, nullptr, 2) == NV_OK);
	CHECK(nv_animate_draws_host(1.0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0) == NV_OK);

	// ---- the reader: a minimal file of the cache's layout (header, then the sections; only the raw arrays carry data)
	const char* path = argc > 1 ? argv[1] : "animate_check.cache";
	uint32_t header[40];
	memset(header, 0, sizeof(header));
	header[0] = 0x434E4353u;
	header[1] = 7;
	header[4] = NV_MESH_MAXVTX;
	header[5] = NV_MESH_MAXTRI;
	header[18] = 2;          // drawCount
	header[20] = 2;          // lightCount
	header[21] = na;         // animationCount
	header[22] = nk;         // keyframeCount
	FILE* f = fopen(path, "wb");
	CHECK(f);
	CHECK(fwrite(header, 1, sizeof(header), f) == sizeof(header));
	CHECK(fwrite(draws0.data(), sizeof(NvMeshDraw), 2, f) == 2);
	CHECK(fwrite(lights0.data(), sizeof(NvLight), 2, f) == 2);
	CHECK(fwrite(table.data(), sizeof(NvAnimation), na, f) == na);
	CHECK(fwrite(keys.data(), sizeof(NvKeyframe), nk, f) == nk);
	fclose(f);
	NvSceneCacheInfo info;
	CHECK(nv_scenecache_info(path, &info) == NV_OK);
	CHECK(info.drawCount == 2 && info.lightCount == 2 && info.animationCount == na && info.keyframeCount == nk && info.drawOffset == 160);
	std::vector<NvLight> rl(2);
	std::vector<NvAnimation> ra(na);
	std::vector<NvKeyframe> rk(nk);
	CHECK(nv_scenecache_animations(path, &info, rl.data(), ra.data(), rk.data()) == NV_OK);
	CHECK(memcmp(rl.data(), lights0.data(), 2 * sizeof(NvLight)) == 0 && memcmp(ra.data(), table.data(), na * sizeof(NvAnimation)) == 0 &&
	      memcmp(rk.data(), keys.data(), nk * sizeof(NvKeyframe)) == 0);
	CHECK(nv_scenecache_animations(path, &info, nullptr, nullptr, nullptr) == NV_OK);
	CHECK(nv_scenecache_animations(path, &info, nullptr, ra.data(), nullptr) == NV_OK);
	// one byte short of the keyframes' end
	const long full = 160 + 2 * 48 + 2 * 32 + (long)na * 24 + (long)nk * 32;
	f = fopen(path, "rb+");
	CHECK(f);
	CHECK(fseek(f, 0, SEEK_END) == 0 && ftell(f) == full);
	fclose(f);
	std::vector<unsigned char> bytes((size_t)full);
	f = fopen(path, "rb");
	CHECK(f && fread(bytes.data(), 1, bytes.size(), f) == bytes.size());
	fclose(f);
	f = fopen(path, "wb");
	CHECK(f && fwrite(bytes.data(), 1, bytes.size() - 1, f) == bytes.size() - 1);
	fclose(f);
	CHECK(nv_scenecache_info(path, &info) == NV_OK);
	CHECK(nv_scenecache_animations(path, &info, rl.data(), ra.data(), rk.data()) == NV_EFORMAT);
	remove(path);
	CHECK(nv_scenecache_animations(path, &info, rl.data(), ra.data(), rk.data()) == NV_EIO);

	printf("animate_check: ok (%u animations, %u keyframes)\n", na, nk);
	return 0;
}
