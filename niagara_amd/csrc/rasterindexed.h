// rasterindexed.h — the text nv_rasterdepth_indexed (rasterindexed.hip) and nv_rasterdepth_indexed_visibility (rasterindexed_vis.hip) share
// (DESIGN.md §4.11, §4.23): the chunk arithmetic, the command search and the raster kernel, rasterindexed_kernel<CLIP, ARGS>, and its
// launch, launch_rasterindexed_as<ARGS>.  The argument struct states what the kernel is (args.h: VIS, ALPHA): depth only; with the stable-form
// visibility word of §4.23 (VIS); or, on RasterIndexedSetArgs<SET> (rasterindexed_alpha.hip, rasterindexed_blocks.hip:
// nv_rasterdepth_indexed_textured, nv_rasterdepth_indexed_blocks, §4.24), VIS with an optional target and the covered samples of a post-pass
// launch also passing the fragment's alpha test (ALPHA).  Every instantiation is held to its bits by the GPU tests of its entry point
// (test_raster_indexed_gpu.py, test_raster_clip_gpu.py, test_visindexed_gpu.py, test_visindexed_textured_gpu.py: lane and wave path, near
// clip on and off).  The kernel repeats its walks per CLIP branch and per ALPHA arm: profiles/raster_fold.md has what one text for them costs.
#pragma once

#include "raster.h"
#include "rasterdepth.h" // ALPHA: the record of a material (rd_alpha_slot) and the alpha-tested sample (rd_sample_alpha), §4.20's, not restated

namespace nv
{

constexpr int RI_WAVES = 4;
constexpr int RI_THREADS = RI_WAVES * 64;
constexpr uint32_t RI_CHUNK = 64;         // triangles per chunk (lane = triangle)
constexpr uint32_t RI_SCAN_BLOCKS = 1024; // workgroups of the count launch at most (the fixed part of the scratch)
static_assert(RI_SCAN_BLOCKS % RI_THREADS == 0, "the scan launch takes RI_SCAN_BLOCKS / RI_THREADS entries per thread");
#ifndef RI_BLOCKS_PER_CU
#define RI_BLOCKS_PER_CU 6 // <= 8: the partial totals are sized for 8 workgroups per CU (context.hip)
#endif

NV_DEV uint32_t ri_sat(unsigned long long v) { return v < 0xffffffffull ? (uint32_t)v : 0xffffffffu; }

// triangles of a drawing command whose three index positions lie below the capacity: triangle t's last position firstIndex + 3t + 2 is below
// it iff t < (indexCapacity - firstIndex) / 3, so they are a prefix of the command's triangles
NV_DEV uint32_t ri_triangles(uint32_t indexCount, uint32_t firstIndex, uint32_t indexCapacity)
{
	const uint32_t room = indexCapacity > firstIndex ? (indexCapacity - firstIndex) / 3u : 0u;
	const uint32_t n = indexCount / 3u;
	return n < room ? n : room;
}

// the end (last chunk + 1) of command i's chunks in the launch, saturated
NV_DEV uint32_t ri_end(const RasterIndexedArgs& a, uint32_t i)
{
	return ri_sat((unsigned long long)a.blockChunks[i / a.perBlock] + a.chunkEnds[i]);
}

// The first command i in [lo, hi) with ri_end(i) > k; there is one (k < ri_end(hi - 1)).  All 64 lanes, wave-uniform arguments.  The next 64
// commands are tried first (a wave walking forward finds its next command there), then 64 evenly spaced probes narrow the range.
NV_DEV uint32_t ri_find(const RasterIndexedArgs& a, uint32_t k, uint32_t lo, uint32_t hi, uint32_t lane)
{
	for (;;)
	{
		const uint32_t span = hi - lo;
		const uint64_t near = __ballot(lane < span && ri_end(a, lo + lane) > k);
		if (near)
			return lo + (uint32_t)__builtin_ctzll(near);
		lo += 64u; // (span > 64: the answer lies further on)
		const uint32_t rest = hi - lo;
		if (rest <= 64u)
			continue;
		const uint32_t p = lo + (uint32_t)(((uint64_t)(lane + 1u) * rest) >> 6) - 1u; // lane 63 probes hi - 1
		const uint32_t j = (uint32_t)__builtin_ctzll(__ballot(ri_end(a, p) > k));
		hi = lo + (uint32_t)(((uint64_t)(j + 1u) * rest) >> 6);
		lo = lo + (uint32_t)(((uint64_t)j * rest) >> 6);
	}
}

// The stable-form word of a triangle of an indexed draw (§4.23): id34 = tri34 + 1 with tri34 = triangleOffsets[drawId] + t, or 0 — depth as
// always, no word — when tri34 is outside the draw's span or is 2^34 - 1 or more (conservative, like mvi >= 2^27 - 1 on the cluster path).
constexpr unsigned long long RI_TRI34_END = (1ull << RD_STABLE_SHIFT) - 1ull;
NV_DEV unsigned long long ri_id34(unsigned long long first, unsigned long long end, uint32_t t)
{
	const unsigned long long tri34 = first + t;
	return tri34 < end && tri34 < RI_TRI34_END ? tri34 + 1ull : 0ull;
}

// One covered-or-not pixel centre.  VIS = false is rd_sample as the depth-only kernel calls it.
template <bool VIS>
NV_DEV bool ri_sample(const RdTri& t, int32_t x, int32_t y, uint32_t W, uint32_t* __restrict__ depth, unsigned long long* __restrict__ vis,
                      unsigned long long id)
{
	if constexpr (VIS)
		return rd_sample<true, unsigned long long>(t, x, y, W, depth, id ? vis : nullptr, id);
	else
		return rd_sample(t, x, y, W, depth, nullptr, 0u);
}

// ALPHA: one corner of the ORIGINAL triangle as fragalpha.h takes it: rd_clip_position's clip x, y, w (the statements rd_vertex starts with:
// the bits both stages share) and the record's fourth word, the packed texcoord
NV_DEV FaCorner ri_corner(const NvGlobals& g, const NvVertex* v, f3 q, float qw, float scale, float px, float py, float pz)
{
	const uint4 r = *reinterpret_cast<const uint4*>(v);
	float clip[4];
	rd_clip_position(g, make_uint2(r.x, r.y), q, qw, scale, px, py, pz, clip);
	return FaCorner{ clip[0], clip[1], clip[3], r.w };
}
NV_DEV float4 ri_corner_word(const FaCorner& c) { return make_float4(c.cx, c.cy, c.cw, __uint_as_float(c.uv)); }

// One covered-or-not pixel centre of the ALPHA instantiations: §4.20's sample (coverage, the alpha test, then the atomics) with the indexed word
template <class ARGS>
NV_DEV void ri_sample_alpha(const ARGS& a, const RdTri& t, const RdAlphaSlot& m, const FaCorner& ca, const FaCorner& cb, const FaCorner& cc, int32_t x, int32_t y,
                            float fw, float fh, unsigned long long* __restrict__ vis, unsigned long long id, unsigned long long& kept,
                            unsigned long long& dropped, unsigned long long& unevaluated)
{
	rd_sample_alpha<true, typename ARGS::Set>(t, m, a.tx.data, ca, cb, cc, x, y, a.width, fw, fh, a.depth, id ? vis : nullptr, id, kept, dropped, unevaluated);
}

// The raster kernel.  ARGS = RasterIndexedArgs: nv_rasterdepth_indexed's, depth only.  ARGS = RasterIndexedVisArgs (ARGS::VIS): the same with the
// visibility word; a.triangleOffsets (drawCount + 1 non-decreasing 64-bit prefixes, the caller's) and a.visibility are read then.
// ARGS = RasterIndexedSetArgs<SET> (ARGS::ALPHA, §4.24): VIS with an optional target, and the covered samples of a post-pass launch also pass the
// fragment's alpha test against a texture set of residency SET.  Every addition sits under `if constexpr (VIS)` or `if constexpr (ALPHA)`.
template <bool CLIP, class ARGS>
__global__ __launch_bounds__(RI_THREADS) void rasterindexed_kernel(ARGS a)
{
	constexpr bool VIS = ARGS::VIS, ALPHA = ARGS::ALPHA;
	unsigned long long* vis = nullptr;
	if constexpr (VIS)
		vis = a.visibility;
	__shared__ int4 s_queue[RI_WAVES][RI_CHUNK][3]; // large pieces of the current chunk (one piece number at a time): their snapped corners
	// VIS: the id34 of each queued piece, next to its corners (a named array of its own: the corners' entry keeps its layout)
	__shared__ unsigned long long s_ids[VIS ? RI_WAVES : 1][VIS ? RI_CHUNK : 1];
	// ALPHA: the three corners of the ORIGINAL triangle of each queued piece (clip x, y, w, packed texcoord), a named array of its own as well
	__shared__ float4 s_corners[ALPHA ? RI_WAVES : 1][ALPHA ? RI_CHUNK : 1][3];

	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t chunks = load_uniform_u32(a.blockChunks + a.scanBlocks); // written by the scan launch
	const uint32_t n = min(load_uniform_u32(a.count), a.drawCount);
	const uint32_t numWaves = gridDim.x * RI_WAVES;
	const uint32_t w = blockIdx.x * RI_WAVES + wave;
	const uint32_t per = chunks / numWaves + (chunks % numWaves ? 1u : 0u); // contiguous chunks per wave
	const unsigned long long begin64 = (unsigned long long)w * per;
	const uint32_t begin = (uint32_t)min(begin64, (unsigned long long)chunks);
	const uint32_t end = (uint32_t)min(begin64 + per, (unsigned long long)chunks);
	const int32_t W = (int32_t)a.width, H = (int32_t)a.height;
	const bool bothFaces = a.globals.cullData.postPass != 0;
	int4(*queue)[3] = s_queue[wave];
	unsigned long long* queueIds = s_ids[VIS ? wave : 0u];
	// ALPHA: the test applies in a post-pass launch that has a material table; otherwise every command's mode is 0 and the kernel writes
	// nv_rasterdepth_indexed_visibility's bits (without a target: nv_rasterdepth_indexed's)
	float4(*queueCorners)[3] = s_corners[ALPHA ? wave : 0u];
	bool alphaOn = false, textured = false;
	float fw = 0.0f, fh = 0.0f;
	unsigned long long dropped = 0, unevaluated = 0;           // per lane
	RdAlphaSlot mat = { 0u, 0.0f, TxDesc{ 0u, 0u, 0u, 0u } }; // the record of the current command's material (wave-uniform)
	if constexpr (ALPHA)
	{
		alphaOn = bothFaces && a.materials != nullptr;
		fw = (float)a.width, fh = (float)a.height;
	}

	uint32_t drawn = 0;             // per lane
	unsigned long long samples = 0; // per lane
	// the current command (wave-uniform): its chunk range, triangles in range, index base and vertex offset, transform
	uint32_t next = 0, cmdBegin = 0, cmdEnd = 0, tris = 0, firstIndex = 0, vertexOffset = 0;
	f3 q = { 0.0f, 0.0f, 0.0f };
	float qw = 1.0f, scale = 0.0f, px = 0.0f, py = 0.0f, pz = 0.0f;
	unsigned long long triFirst = 0, triEnd = 0; // VIS: the current draw's span of triangle names (wave-uniform)

	for (uint32_t k = begin; k < end; ++k)
	{
		if (k >= cmdEnd)
		{
			const uint32_t i = ri_find(a, k, next, n, lane);
			next = i + 1u;
			cmdBegin = __builtin_amdgcn_readfirstlane(i ? ri_end(a, i - 1u) : 0u);
			cmdEnd = __builtin_amdgcn_readfirstlane(ri_end(a, i));
			const NvMeshDrawCommand c = a.commands[i]; // a command with chunks draws: drawId < drawCount
			tris = __builtin_amdgcn_readfirstlane(ri_triangles(c.indexCount, c.firstIndex, a.indexCapacity));
			firstIndex = __builtin_amdgcn_readfirstlane(c.firstIndex);
			vertexOffset = __builtin_amdgcn_readfirstlane(c.vertexOffset);
			const float4* dp = reinterpret_cast<const float4*>(a.draws + __builtin_amdgcn_readfirstlane(c.drawId));
			if constexpr (VIS && !ALPHA)
			{
				const unsigned long long* op = a.triangleOffsets + __builtin_amdgcn_readfirstlane(c.drawId); // (drawId < drawCount: [drawId + 1] exists)
				triFirst = op[0], triEnd = op[1];
			}
			if constexpr (ALPHA)
			{
				triFirst = triEnd = 0; // (without a visibility target every id is 0: depth only)
				if (a.triangleOffsets)
				{
					const unsigned long long* op = a.triangleOffsets + __builtin_amdgcn_readfirstlane(c.drawId);
					triFirst = op[0], triEnd = op[1];
				}
				// the command's material, where its transform is loaded: word 11 of the draw, then rd_alpha_slot's guarded loads
				uint32_t mode = 0u;
				float factor = 0.0f;
				uint4 desc = make_uint4(0u, 0u, 0u, 0u);
				if (alphaOn)
					rd_alpha_slot(a, reinterpret_cast<const uint32_t*>(dp + 2)[3], mode, factor, desc);
				mat = RdAlphaSlot{ (uint32_t)__builtin_amdgcn_readfirstlane(mode), __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(factor))),
					                TxDesc{ (uint32_t)__builtin_amdgcn_readfirstlane(desc.x), (uint32_t)__builtin_amdgcn_readfirstlane(desc.y),
					                        (uint32_t)__builtin_amdgcn_readfirstlane(desc.z), (uint32_t)__builtin_amdgcn_readfirstlane(desc.w) } };
				textured = (mat.mode & RD_A_TEXTURED) != 0u;
			}
			const float4 d0 = dp[0], d1 = dp[1];
			q = { d1.x, d1.y, d1.z };
			qw = d1.w, scale = d0.w, px = d0.x, py = d0.y, pz = d0.z;
		}

		// ---- lane = triangle: indices, corners (mesh.vert.glsl:41-57, per corner), setup; small ones walked here, large ones queued
		const uint32_t t = (k - cmdBegin) * RI_CHUNK + lane; // (a command has < 2^26 chunks)
		unsigned long long id = 0;
		if constexpr (VIS)
			id = ri_id34(triFirst, triEnd, t);
		FaCorner fa = { 0.0f, 0.0f, 0.0f, 0u }, fb = fa, fc = fa; // ALPHA: the lane's ORIGINAL triangle, in registers
		// The two branches repeat each other's text on purpose: written as one loop over pieces, the CLIP = false instantiation compiles to other
		// code than the kernel had before the option (other registers, other schedule); kept apart, it is that kernel instruction for instruction.
		if constexpr (!CLIP)
		{
			RdTri tri;
			bool live = false, large = false;
			int4 ca = make_int4(0, 0, 0, 1), cb = ca, cc = ca;
			if (t < tris)
			{
				const unsigned long long at = (unsigned long long)firstIndex + 3ull * t; // at + 2 < indexCapacity (ri_triangles)
				const uint32_t va = a.indices[at] + vertexOffset, vb = a.indices[at + 1] + vertexOffset, vc = a.indices[at + 2] + vertexOffset;
				if (va < a.vertexCapacity && vb < a.vertexCapacity && vc < a.vertexCapacity) // (0xFFFFFFFF included: no primitive restart)
				{
					ca = rd_vertex(a.globals, *reinterpret_cast<const uint2*>(a.vertices + va), q, qw, scale, px, py, pz, H);
					cb = rd_vertex(a.globals, *reinterpret_cast<const uint2*>(a.vertices + vb), q, qw, scale, px, py, pz, H);
					cc = rd_vertex(a.globals, *reinterpret_cast<const uint2*>(a.vertices + vc), q, qw, scale, px, py, pz, H);
					live = rd_setup_corners(ca, cb, cc, bothFaces, W, H, tri);
					if constexpr (ALPHA)
						if (textured)
						{
							fa = ri_corner(a.globals, a.vertices + va, q, qw, scale, px, py, pz);
							fb = ri_corner(a.globals, a.vertices + vb, q, qw, scale, px, py, pz);
							fc = ri_corner(a.globals, a.vertices + vc, q, qw, scale, px, py, pz);
						}
				}
			}
			if (live)
			{
				drawn += 1;
				if (tri.x0 <= tri.x1 && tri.y0 <= tri.y1)
				{
					const uint32_t boxPixels = (uint32_t)(tri.x1 - tri.x0 + 1) * (uint32_t)(tri.y1 - tri.y0 + 1);
					large = boxPixels > a.smallLimit;
					if (!large)
						for (int32_t y = tri.y0; y <= tri.y1; ++y)
							for (int32_t x = tri.x0; x <= tri.x1; ++x)
							{
								if constexpr (ALPHA)
									ri_sample_alpha(a, tri, mat, fa, fb, fc, x, y, fw, fh, vis, id, samples, dropped, unevaluated);
								else
									samples += ri_sample<VIS>(tri, x, y, a.width, a.depth, vis, id) ? 1u : 0u;
							}
				}
			}
			const uint64_t qb = __ballot(large);
			rd_lds_order(); // the previous chunk's queue readers are done
			if (large)
			{
				const uint32_t slot = (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(qb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)qb, 0u));
				queue[slot][0] = ca;
				queue[slot][1] = cb;
				queue[slot][2] = cc;
				if constexpr (VIS)
					queueIds[slot] = id;
				if constexpr (ALPHA)
					if (textured)
						queueCorners[slot][0] = ri_corner_word(fa), queueCorners[slot][1] = ri_corner_word(fb), queueCorners[slot][2] = ri_corner_word(fc);
			}
			rd_lds_order();

			// ---- large triangles, the whole wave: lane = pixel of an 8 x 8 stamp
			const uint32_t queued = (uint32_t)__builtin_popcountll(qb);
			for (uint32_t e = 0; e < queued; ++e)
			{
				RdTri tq;
				unsigned long long idq = 0;
				if constexpr (VIS)
					idq = queueIds[e];
				FaCorner ea = { 0.0f, 0.0f, 0.0f, 0u }, eb = ea, ec = ea; // ALPHA: the queued triangle's corners
				if constexpr (ALPHA)
					if (textured)
						ea = rd_corner(queueCorners[e][0]), eb = rd_corner(queueCorners[e][1]), ec = rd_corner(queueCorners[e][2]);
				rd_setup_corners(queue[e][0], queue[e][1], queue[e][2], bothFaces, W, H, tq); // (true: it was queued; same inputs, same bits)
				const uint32_t sw = (uint32_t)(tq.x1 - tq.x0) / 8u + 1u, sh = (uint32_t)(tq.y1 - tq.y0) / 8u + 1u;
				const int32_t lx = (int32_t)(lane & 7u), ly = (int32_t)(lane >> 3);
				for (uint32_t sy = 0; sy < sh; ++sy)
				{
					const int32_t y = tq.y0 + (int32_t)sy * 8 + ly;
					for (uint32_t sx = 0; sx < sw; ++sx)
					{
						const int32_t x = tq.x0 + (int32_t)sx * 8 + lx;
						if constexpr (ALPHA)
						{
							if (x <= tq.x1 && y <= tq.y1)
								ri_sample_alpha(a, tq, mat, ea, eb, ec, x, y, fw, fh, vis, idq, samples, dropped, unevaluated);
						}
						else if (x <= tq.x1 && y <= tq.y1)
							samples += ri_sample<VIS>(tq, x, y, a.width, a.depth, vis, idq) ? 1u : 0u;
					}
				}
			}
		}
		else
		{
			uint32_t pieces = 0;
			int4 p0 = make_int4(0, 0, 0, 1), p1 = p0, p2 = p0, p3 = p0;
			if (t < tris)
			{
				const unsigned long long at = (unsigned long long)firstIndex + 3ull * t; // at + 2 < indexCapacity (ri_triangles)
				const uint32_t va = a.indices[at] + vertexOffset, vb = a.indices[at + 1] + vertexOffset, vc = a.indices[at + 2] + vertexOffset;
				if (va < a.vertexCapacity && vb < a.vertexCapacity && vc < a.vertexCapacity) // (0xFFFFFFFF included: no primitive restart)
				{
					const uint2 ra = *reinterpret_cast<const uint2*>(a.vertices + va), rb = *reinterpret_cast<const uint2*>(a.vertices + vb);
					const uint2 rc = *reinterpret_cast<const uint2*>(a.vertices + vc);
					float4 ka, kb, kc;
					const int4 ca = rd_vertex_clip(a.globals, ra, q, qw, scale, px, py, pz, H, ka);
					const int4 cb = rd_vertex_clip(a.globals, rb, q, qw, scale, px, py, pz, H, kb);
					const int4 cc = rd_vertex_clip(a.globals, rc, q, qw, scale, px, py, pz, H, kc);
					pieces = rd_clip(a.globals, ca, cb, cc, ka, kb, kc, H, p0, p1, p2, p3);
					if constexpr (ALPHA)
						if (textured) // (the ORIGINAL triangle's corners, not a piece's: the visibility word names that triangle)
						{
							fa = ri_corner(a.globals, a.vertices + va, q, qw, scale, px, py, pz);
							fb = ri_corner(a.globals, a.vertices + vb, q, qw, scale, px, py, pz);
							fc = ri_corner(a.globals, a.vertices + vc, q, qw, scale, px, py, pz);
						}
				}
			}
			for (uint32_t p = 0; p < 2u; ++p)
			{
				if (!__ballot(p < pieces)) // (wave-uniform)
					break;
				RdTri tri;
				bool large = false;
				const int4 cb = rd_sel(p != 0u, p2, p1), cc = rd_sel(p != 0u, p3, p2);
				const bool live = p < pieces && rd_setup_corners(p0, cb, cc, bothFaces, W, H, tri);
				if (live)
				{
					drawn += 1;
					if (tri.x0 <= tri.x1 && tri.y0 <= tri.y1)
					{
						const uint32_t boxPixels = (uint32_t)(tri.x1 - tri.x0 + 1) * (uint32_t)(tri.y1 - tri.y0 + 1);
						large = boxPixels > a.smallLimit;
						if (!large)
							for (int32_t y = tri.y0; y <= tri.y1; ++y)
								for (int32_t x = tri.x0; x <= tri.x1; ++x)
								{
									if constexpr (ALPHA)
										ri_sample_alpha(a, tri, mat, fa, fb, fc, x, y, fw, fh, vis, id, samples, dropped, unevaluated);
									else
										samples += ri_sample<VIS>(tri, x, y, a.width, a.depth, vis, id) ? 1u : 0u;
								}
					}
				}
				const uint64_t qb = __ballot(large);
				rd_lds_order(); // the previous queue's readers are done
				if (large)
				{
					const uint32_t slot = (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(qb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)qb, 0u));
					queue[slot][0] = p0;
					queue[slot][1] = cb;
					queue[slot][2] = cc;
					if constexpr (VIS)
						queueIds[slot] = id;
					if constexpr (ALPHA)
						if (textured)
							queueCorners[slot][0] = ri_corner_word(fa), queueCorners[slot][1] = ri_corner_word(fb), queueCorners[slot][2] = ri_corner_word(fc);
				}
				rd_lds_order();

				// ---- large pieces, the whole wave: lane = pixel of an 8 x 8 stamp
				const uint32_t queued = (uint32_t)__builtin_popcountll(qb);
				for (uint32_t e = 0; e < queued; ++e)
				{
					RdTri tq;
					unsigned long long idq = 0;
					if constexpr (VIS)
						idq = queueIds[e];
					FaCorner ea = { 0.0f, 0.0f, 0.0f, 0u }, eb = ea, ec = ea; // ALPHA: the corners of the ORIGINAL triangle of the queued piece
					if constexpr (ALPHA)
						if (textured)
							ea = rd_corner(queueCorners[e][0]), eb = rd_corner(queueCorners[e][1]), ec = rd_corner(queueCorners[e][2]);
					rd_setup_corners(queue[e][0], queue[e][1], queue[e][2], bothFaces, W, H, tq); // (true: it was queued; same inputs, same bits)
					const uint32_t sw = (uint32_t)(tq.x1 - tq.x0) / 8u + 1u, sh = (uint32_t)(tq.y1 - tq.y0) / 8u + 1u;
					const int32_t lx = (int32_t)(lane & 7u), ly = (int32_t)(lane >> 3);
					for (uint32_t sy = 0; sy < sh; ++sy)
					{
						const int32_t y = tq.y0 + (int32_t)sy * 8 + ly;
						for (uint32_t sx = 0; sx < sw; ++sx)
						{
							const int32_t x = tq.x0 + (int32_t)sx * 8 + lx;
							if constexpr (ALPHA)
							{
								if (x <= tq.x1 && y <= tq.y1)
									ri_sample_alpha(a, tq, mat, ea, eb, ec, x, y, fw, fh, vis, idq, samples, dropped, unevaluated);
							}
							else if (x <= tq.x1 && y <= tq.y1)
								samples += ri_sample<VIS>(tq, x, y, a.width, a.depth, vis, idq) ? 1u : 0u;
						}
					}
				}
			}
		}
	}

	// totals 2-3: per-workgroup partial sums, plain stores (0 in slots 0-1: the scan launch added those); launch_raster_totals adds them up
	__shared__ unsigned long long s_tot[RI_WAVES][ALPHA ? 4 : 2];
	unsigned long long d = drawn, smp = samples;
	for (int o = 32; o > 0; o >>= 1)
	{
		d += __shfl_xor(d, o, 64);
		smp += __shfl_xor(smp, o, 64);
		if constexpr (ALPHA)
		{
			dropped += __shfl_xor(dropped, o, 64);
			unevaluated += __shfl_xor(unevaluated, o, 64);
		}
	}
	if (lane == 0)
	{
		s_tot[wave][0] = d;
		s_tot[wave][1] = smp;
		if constexpr (ALPHA)
		{
			s_tot[wave][2] = dropped;
			s_tot[wave][3] = unevaluated;
		}
	}
	__syncthreads();
	// ALPHA: two more partial sums, {dropped, unevaluated}, from threads 4 and 5 (the four below keep their statements)
	if constexpr (ALPHA)
		if (threadIdx.x >= 4 && threadIdx.x < 6 && a.alphaPartials)
		{
			unsigned long long t = 0;
#pragma unroll
			for (int k = 0; k < RI_WAVES; ++k)
				t += s_tot[k][threadIdx.x - 2];
			a.alphaPartials[(size_t)blockIdx.x * 2 + (threadIdx.x - 4)] = t;
		}
	if (threadIdx.x < 4)
	{
		unsigned long long t = 0;
		if (threadIdx.x >= 2)
#pragma unroll
			for (int k = 0; k < RI_WAVES; ++k)
				t += s_tot[k][threadIdx.x - 2];
		a.partials[(size_t)blockIdx.x * 4 + threadIdx.x] = t;
	}
}

// The launches of one pass, for every ARGS: the count and scan launches every indexed raster starts with, the kernel by near clip, then the
// totals launches the caller asked for
template <typename ARGS>
int launch_rasterindexed_as(hipStream_t stream, ARGS a, void* scratch, uint32_t gridBlocks, bool nearClip)
{
	launch_rasterindexed_prepare(stream, a, scratch);
	gridBlocks = gridBlocks / 8 * RI_BLOCKS_PER_CU; // the caller passes 8 workgroups per CU, the size of `partials` and `alphaPartials`
	if (nearClip)
		hipLaunchKernelGGL((rasterindexed_kernel<true, ARGS>), dim3(gridBlocks), dim3(RI_THREADS), 0, stream, a);
	else
		hipLaunchKernelGGL((rasterindexed_kernel<false, ARGS>), dim3(gridBlocks), dim3(RI_THREADS), 0, stream, a);
	hipError_t e = hipGetLastError();
	if (e == hipSuccess && a.totals)
		e = (hipError_t)launch_raster_totals(stream, a.partials, gridBlocks, a.totals, 4);
	if constexpr (ARGS::ALPHA)
		if (e == hipSuccess && a.alphaTotals)
			e = (hipError_t)launch_raster_totals(stream, a.alphaPartials, gridBlocks, a.alphaTotals, 2);
	return (int)e;
}

} // namespace nv
