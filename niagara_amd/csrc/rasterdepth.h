// rasterdepth.h — the kernel of the depth rasteriser of the visible clusters as ONE text for its entry points:
// rasterdepth.hip instantiates rasterdepth_kernel<CLIP, STABLE> (nv_rasterdepth) and rasterdepth_alpha.hip and rasterdepth_blocks.hip
// rasterdepth_kernel<CLIP, STABLE, true, RasterSetArgs<SET>> (nv_rasterdepth_textured, nv_rasterdepth_blocks: covered samples of a post-pass
// launch also pass the fragment's alpha test against a texture set of residency SET, texmath.h's TxDecoded or TxBlocks, §4.21).  ALPHA only adds
// statements under `if constexpr (ALPHA)`, so the four kernels of nv_rasterdepth keep their instruction streams.  rasterdepth.hip's header
// describes the shape.  The launch of every instantiation is launch_rasterdepth_as below.
#pragma once
#include "raster.h"
#include "fragalpha.h"
#include "launch.h"

namespace nv
{

constexpr int RD_WAVES = 4;
constexpr int RD_THREADS = RD_WAVES * 64;
constexpr uint32_t RD_CHUNK = 64; // slots whose headers a wave fetches together (lane = slot)
#ifndef RD_BLOCKS_PER_CU
#define RD_BLOCKS_PER_CU 6 // <= 8: the partial totals are sized for 8 workgroups per CU (context.hip)
#endif

// the id of triangle t in the visibility word: slot << 7 | t, or the stable form's id34 (raster.h)
template <bool STABLE>
NV_DEV auto rd_id(uint32_t index, uint32_t mvi, uint32_t t)
{
	if constexpr (STABLE)
		return ((unsigned long long)mvi << 7 | t) + 1ull;
	else
		return index << 7 | t;
}

// ---- ALPHA: what a slot's material says about its covered samples, wave-uniform
constexpr uint32_t RD_A_TEXTURED = 1u;    // alpha-tested: albedo.a = diffuseFactor.a x the albedo texel's .a, per sample
constexpr uint32_t RD_A_DROP_ALL = 2u;    // albedo.a = diffuseFactor.a < 0.5, constant over the slot: every covered sample is dropped
constexpr uint32_t RD_A_UNEVALUATED = 4u; // materialIndex past the table (opaque), or the albedo texture named cannot be sampled (absent, §4.18)

struct RdAlphaSlot
{
	uint32_t mode; // RD_A_*; 0: albedo.a = diffuseFactor.a >= 0.5 (or NaN), or the launch does not test
	float factor;  // diffuseFactor.a
	TxDesc desc;   // RD_A_TEXTURED: the albedo texture's descriptor, accepted by the set (TxTable::desc): its four words, whatever the set calls them
};

// The slot record of a draw's material.  Every load is behind the check that keeps it inside the caller's tables.
// ARGS = RasterSetArgs<SET>
template <typename ARGS>
NV_DEV void rd_alpha_slot(const ARGS& a, uint32_t materialIndex, uint32_t& mode, float& factor, uint4& desc)
{
	mode = RD_A_UNEVALUATED;
	if (materialIndex >= a.materialCount)
		return;
	const uint4* mp = reinterpret_cast<const uint4*>(a.materials + materialIndex);
	const uint32_t albedoTexture = mp[0].x;
	factor = reinterpret_cast<const float4*>(mp + 1)->w;
	mode = 0u;
	if (albedoTexture != 0u) // mesh.frag.glsl:63
	{
		typename ARGS::Set::Desc d;
		if (a.tx.desc(albedoTexture, d))
		{
			const auto& [w0, w1, w2, w3] = d;
			mode = RD_A_TEXTURED;
			desc = make_uint4(w0, w1, w2, w3);
			return;
		}
		mode = RD_A_UNEVALUATED;
	}
	mode |= fa_discard(factor) ? RD_A_DROP_ALL : 0u;
}

// rd_sample with the fragment's alpha test between the coverage and the atomics: the attribute pass's arithmetic (fragalpha.h) for the
// ORIGINAL triangle's corners (ca, cb, cc: stored order) at this pixel, the albedo texture sampled from `texels`, the buffer of a set of
// residency SET.  A dropped sample loads, compares and writes nothing.
template <bool STABLE, class SET, class ID>
NV_DEV void rd_sample_alpha(const RdTri& t, const RdAlphaSlot& m, const typename SET::Unit* __restrict__ texels, const FaCorner& ca, const FaCorner& cb,
                            const FaCorner& cc, int32_t px, int32_t py, uint32_t W, float fw, float fh, uint32_t* __restrict__ depth,
                            unsigned long long* __restrict__ vis, ID id, unsigned long long& kept, unsigned long long& dropped, unsigned long long& unevaluated)
{
	int64_t wb, wc;
	if (!rd_covered(t, px, py, wb, wc))
		return;
	bool drop = (m.mode & RD_A_DROP_ALL) != 0u;
	if (m.mode & RD_A_TEXTURED)
	{
		const float fx = (float)px + 0.5f, fy = (float)py + 0.5f;
		float l0, l1, l2;
		fa_bary(ca, cb, cc, fx, fy, fw, fh, l0, l1, l2);
		const float u = va_mix(l0, l1, l2, half_bits_to_float(ca.uv & 0xffffu), half_bits_to_float(cb.uv & 0xffffu), half_bits_to_float(cc.uv & 0xffffu));
		const float v = va_mix(l0, l1, l2, half_bits_to_float(ca.uv >> 16), half_bits_to_float(cb.uv >> 16), half_bits_to_float(cc.uv >> 16));
		float dudx, dvdx, dudy, dvdy;
		fa_uv_steps(ca, cb, cc, (uint32_t)px, (uint32_t)py, fx, fy, fw, fh, u, v, dudx, dvdx, dudy, dvdy);
		const TxF4 c = SET::sample(texels, typename SET::Desc{ m.desc.offset, m.desc.width, m.desc.height, m.desc.levels }, u, v, dudx, dvdx, dudy, dvdy);
		drop = fa_discard(fa_alpha(m.factor, c.w));
	}
	if (!drop)
		rd_write<STABLE>(t, wb, wc, px, py, W, depth, vis, id);
	kept += drop ? 0u : 1u;
	dropped += drop ? 1u : 0u;
	unevaluated += (m.mode & RD_A_UNEVALUATED) != 0u ? 1u : 0u;
}

NV_DEV FaCorner rd_corner(float4 v) { return FaCorner{ v.x, v.y, v.z, __float_as_uint(v.w) }; }

// ARGS = RasterArgs (ALPHA = false) or RasterSetArgs<SET> (ALPHA = true)
template <bool CLIP, bool STABLE, bool ALPHA = false, typename ARGS = RasterArgs>
__global__ __launch_bounds__(RD_THREADS) void rasterdepth_kernel(ARGS a)
{
	constexpr uint32_t PIECES = CLIP ? 2u : 1u; // pieces of a triangle at most
	__shared__ int4 s_vtx[RD_WAVES][64];       // per vertex of the current slot: X, Y, z bits, reject (CLIP: | RD_OUTSIDE)
	__shared__ float4 s_clip[RD_WAVES][64];    // CLIP only: clip x, y, w and d = w - z (NaN: a non-finite component)
	__shared__ float4 s_attr[RD_WAVES][64];    // ALPHA only: clip x, y, w and the packed texcoord tu | tv << 16
	__shared__ uint32_t s_queue[RD_WAVES][96 * PIECES]; // large pieces of the current slot: t | piece << 7 | ia << 8 | ib << 16 | ic << 24

	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t gx = a.cc4[1], gz = a.cc4[3];
	const uint32_t slots = gx * a.cc4[2] * gz;
	const uint32_t numWaves = gridDim.x * RD_WAVES;
	const uint32_t w = blockIdx.x * RD_WAVES + wave;
	const uint32_t per = (slots + numWaves - 1) / numWaves; // contiguous slots per wave
	const uint32_t begin = w * per < slots ? w * per : slots;
	const uint32_t end = begin + per < slots ? begin + per : slots;
	const int32_t W = (int32_t)a.width, H = (int32_t)a.height;
	const bool bothFaces = a.globals.cullData.postPass != 0;
	const uint8_t* data8 = reinterpret_cast<const uint8_t*>(a.meshletData);
	const uint16_t* data16 = reinterpret_cast<const uint16_t*>(a.meshletData);
	int4* vtx = s_vtx[wave];
	uint32_t* queue = s_queue[wave];
	float4* cvx = nullptr;
	if constexpr (CLIP)
		cvx = s_clip[wave];

	// ALPHA: the test applies in a post-pass launch that has a material table; otherwise every slot's mode is 0 and the kernel writes nv_rasterdepth's bits
	float4* attr = nullptr;
	bool alphaOn = false;
	float fw = 0.0f, fh = 0.0f;
	unsigned long long dropped = 0, unevaluated = 0; // per lane
	if constexpr (ALPHA)
	{
		attr = s_attr[wave];
		alphaOn = bothFaces && a.materials != nullptr;
		fw = (float)a.width, fh = (float)a.height;
	}

	uint32_t clusters = 0, triangles = 0; // wave-uniform
	uint32_t drawn = 0;                   // per lane
	unsigned long long samples = 0;       // per lane

	for (uint32_t chunk = begin; chunk < end; chunk += RD_CHUNK)
	{
		const uint32_t cnt = end - chunk < RD_CHUNK ? end - chunk : RD_CHUNK;
		// lane = slot: grid position -> index (the mesh shader's x + 256 y + CLUSTER_TILE z) -> cluster index -> command -> headers
		uint32_t hIndex = 0, hCi = ~0u, hDataOffset = 0, hBaseVertex = 0, hCounts = 0;
		uint32_t hMvi = 0; // STABLE only: the cluster's meshlet-visibility index, command.meshletVisibilityOffset + lane (the bit nv_clustercull keeps for it)
		float4 hD0 = make_float4(0, 0, 0, 0), hD1 = make_float4(0, 0, 0, 1);
		uint32_t hMode = 0; // ALPHA only: the slot record of the draw's material
		float hFactor = 0.0f;
		uint4 hDesc = make_uint4(0, 0, 0, 0);
		if (lane < cnt)
		{
			const uint32_t k = chunk + lane, x = k % gx, r = k / gx;
			hIndex = x + (r / gz) * 256u + (r % gz) * NV_CLUSTER_TILE;
			hCi = a.clusterIndices[hIndex];
		}
		if (hCi != ~0u)
		{
			const uint32_t* cmd = reinterpret_cast<const uint32_t*>(a.commands + (hCi & 0xffffffu));
			const uint32_t drawId = cmd[0], taskOffset = cmd[1];
			const uint32_t* mw = reinterpret_cast<const uint32_t*>(a.meshlets + taskOffset + (hCi >> 24));
			hDataOffset = mw[3];
			hBaseVertex = mw[4];
			hCounts = mw[5] & 0xffffffu; // vertexCount | triangleCount << 8 | shortRefs << 16
			if constexpr (STABLE)
				hMvi = cmd[4] + (hCi >> 24);
			const float4* dp = reinterpret_cast<const float4*>(a.draws + drawId);
			hD0 = dp[0];
			hD1 = dp[1];
			if constexpr (ALPHA)
				if (alphaOn)
					rd_alpha_slot(a, reinterpret_cast<const uint32_t*>(dp + 2)[3], hMode, hFactor, hDesc); // (word 11: draw.materialIndex)
		}

		for (uint32_t s = 0; s < cnt; ++s)
		{
			const uint32_t ci = rd_rl(hCi, s);
			if (ci == ~0u)
				continue;
			const uint32_t index = rd_rl(hIndex, s);
			const uint32_t dataOffset = rd_rl(hDataOffset, s), baseVertex = rd_rl(hBaseVertex, s), counts = rd_rl(hCounts, s);
			const uint32_t vcRaw = counts & 0xffu, tcRaw = counts >> 8 & 0xffu, shortRefs = (counts >> 16 & 0xffu) == 1u;
			const uint32_t ve = vcRaw < 64u ? vcRaw : 64u, te = tcRaw < 96u ? tcRaw : 96u;
			const uint32_t indexOffset = dataOffset + (shortRefs ? (vcRaw + 1) / 2 : vcRaw);
			clusters += 1;
			triangles += tcRaw;
			// STABLE: a cluster whose index does not fit the word's 27 bits writes depth and no visibility word
			uint32_t mvi = 0;
			unsigned long long* vis = a.visibility;
			if constexpr (STABLE)
			{
				mvi = rd_rl(hMvi, s);
				vis = mvi < RD_STABLE_MVI_END ? vis : nullptr;
			}

			RdAlphaSlot slot = { 0u, 0.0f, TxDesc{ 0u, 0u, 0u, 0u } };
			if constexpr (ALPHA)
				slot = RdAlphaSlot{ rd_rl(hMode, s), __uint_as_float(rd_rl(__float_as_uint(hFactor), s)),
					                TxDesc{ rd_rl(hDesc.x, s), rd_rl(hDesc.y, s), rd_rl(hDesc.z, s), rd_rl(hDesc.w, s) } };
			const bool textured = ALPHA && (slot.mode & RD_A_TEXTURED) != 0u; // (wave-uniform)

			rd_lds_order(); // the previous slot's readers are done
			// ---- vertex stage, lane = vertex (nv_trianglecull's arithmetic, src/shaders/meshlet.mesh.glsl:121-160)
			const f3 q = { __uint_as_float(rd_rl(__float_as_uint(hD1.x), s)), __uint_as_float(rd_rl(__float_as_uint(hD1.y), s)),
			               __uint_as_float(rd_rl(__float_as_uint(hD1.z), s)) };
			const float qw = __uint_as_float(rd_rl(__float_as_uint(hD1.w), s)), scale = __uint_as_float(rd_rl(__float_as_uint(hD0.w), s));
			const float px = __uint_as_float(rd_rl(__float_as_uint(hD0.x), s)), py = __uint_as_float(rd_rl(__float_as_uint(hD0.y), s));
			const float pz = __uint_as_float(rd_rl(__float_as_uint(hD0.z), s));
			if (lane < ve)
			{
				const uint32_t ref = shortRefs ? (uint32_t)data16[dataOffset * 2 + lane] : a.meshletData[dataOffset + lane];
				uint2 pv;
				if constexpr (ALPHA)
				{
					// the whole record: its fourth word is the texcoord.  rd_clip_position again: the same statements, the bits both stages share
					const uint4 pv4 = *reinterpret_cast<const uint4*>(a.vertices + ref + baseVertex);
					pv = make_uint2(pv4.x, pv4.y);
					if (textured)
					{
						float clip[4];
						rd_clip_position(a.globals, pv, q, qw, scale, px, py, pz, clip);
						attr[lane] = make_float4(clip[0], clip[1], clip[3], __uint_as_float(pv4.w));
					}
				}
				else
					pv = *reinterpret_cast<const uint2*>(a.vertices + ref + baseVertex);
				if constexpr (CLIP)
				{
					float4 cv;
					vtx[lane] = rd_vertex_clip(a.globals, pv, q, qw, scale, px, py, pz, H, cv);
					cvx[lane] = cv;
				}
				else
					vtx[lane] = rd_vertex(a.globals, pv, q, qw, scale, px, py, pz, H);
			}
			rd_lds_order();

			// ---- triangle setup, lane = triangle; small ones are walked here by their own lane, large ones queued
			uint32_t queued = 0; // wave-uniform
			for (uint32_t tb = 0; tb < te; tb += 64)
			{
				// The two branches repeat each other's text on purpose: written as one loop over pieces, the CLIP = false instantiation compiles to other
				// code than the kernel had before the option (other registers, other schedule); kept apart, it is that kernel instruction for instruction.
				if constexpr (!CLIP)
				{
					const uint32_t t = tb + lane;
					RdTri tri;
					bool live = false, large = false;
					uint32_t ia = 0, ib = 0, ic = 0;
					if (t < te)
					{
						const uint32_t o = indexOffset * 4 + t * 3;
						ia = data8[o], ib = data8[o + 1], ic = data8[o + 2];
						live = rd_setup(vtx, ia, ib, ic, ve, bothFaces, W, H, tri);
					}
					if (live)
					{
						drawn += 1;
						if (tri.x0 <= tri.x1 && tri.y0 <= tri.y1)
						{
							const uint32_t n = (uint32_t)(tri.x1 - tri.x0 + 1) * (uint32_t)(tri.y1 - tri.y0 + 1);
							large = n > a.smallLimit;
							if (!large)
							{
								const auto id = rd_id<STABLE>(index, mvi, t);
								if constexpr (ALPHA)
								{
									FaCorner ca = { 0.0f, 0.0f, 0.0f, 0u }, cb = ca, cc = ca;
									if (textured)
										ca = rd_corner(attr[ia]), cb = rd_corner(attr[ib]), cc = rd_corner(attr[ic]);
									for (int32_t py = tri.y0; py <= tri.y1; ++py)
										for (int32_t px = tri.x0; px <= tri.x1; ++px)
											rd_sample_alpha<STABLE, typename ARGS::Set>(tri, slot, a.tx.data, ca, cb, cc, px, py, a.width, fw, fh, a.depth,
											                                            STABLE ? vis : a.visibility, id, samples, dropped, unevaluated);
								}
								else
								{
									for (int32_t py = tri.y0; py <= tri.y1; ++py)
										for (int32_t px = tri.x0; px <= tri.x1; ++px)
											samples += rd_sample<STABLE>(tri, px, py, a.width, a.depth, STABLE ? vis : a.visibility, id) ? 1u : 0u;
								}
							}
						}
					}
					const uint64_t q = __ballot(large);
					if (large)
					{
						// the raw index bytes: the wave reruns rd_setup on them (same inputs, same bits)
						const uint32_t at = queued + (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(q >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)q, 0u));
						queue[at] = t | ia << 8 | ib << 16 | ic << 24;
					}
					queued += (uint32_t)__builtin_popcountll(q);
				}
				else
				{
					const uint32_t t = tb + lane;
					uint32_t ia = 0, ib = 0, ic = 0, pieces = 0;
					int4 p0 = make_int4(0, 0, 0, 1), p1 = p0, p2 = p0, p3 = p0;
					if (t < te)
					{
						const uint32_t o = indexOffset * 4 + t * 3;
						ia = data8[o], ib = data8[o + 1], ic = data8[o + 2];
						if (ia < ve && ib < ve && ic < ve)
							pieces = rd_clip(a.globals, vtx[ia], vtx[ib], vtx[ic], cvx[ia], cvx[ib], cvx[ic], H, p0, p1, p2, p3);
					}
					for (uint32_t p = 0; p < 2u; ++p)
					{
						if (!__ballot(p < pieces)) // (wave-uniform)
							break;
						RdTri tri;
						bool large = false;
						const bool live = p < pieces && rd_setup_corners(p0, rd_sel(p != 0u, p2, p1), rd_sel(p != 0u, p3, p2), bothFaces, W, H, tri);
						if (live)
						{
							drawn += 1;
							if (tri.x0 <= tri.x1 && tri.y0 <= tri.y1)
							{
								const uint32_t n = (uint32_t)(tri.x1 - tri.x0 + 1) * (uint32_t)(tri.y1 - tri.y0 + 1);
								large = n > a.smallLimit;
								if (!large)
								{
									const auto id = rd_id<STABLE>(index, mvi, t);
									if constexpr (ALPHA)
									{
										// (the ORIGINAL triangle's corners, not the piece's: the visibility word names that triangle)
										FaCorner ca = { 0.0f, 0.0f, 0.0f, 0u }, cb = ca, cc = ca;
										if (textured)
											ca = rd_corner(attr[ia]), cb = rd_corner(attr[ib]), cc = rd_corner(attr[ic]);
										for (int32_t py = tri.y0; py <= tri.y1; ++py)
											for (int32_t px = tri.x0; px <= tri.x1; ++px)
												rd_sample_alpha<STABLE, typename ARGS::Set>(tri, slot, a.tx.data, ca, cb, cc, px, py, a.width, fw, fh, a.depth,
												                                            STABLE ? vis : a.visibility, id, samples, dropped, unevaluated);
									}
									else
									{
										for (int32_t py = tri.y0; py <= tri.y1; ++py)
											for (int32_t px = tri.x0; px <= tri.x1; ++px)
												samples += rd_sample<STABLE>(tri, px, py, a.width, a.depth, STABLE ? vis : a.visibility, id) ? 1u : 0u;
									}
								}
							}
						}
						const uint64_t q = __ballot(large);
						if (large)
						{
							// the raw index bytes: the wave reruns the setup on them (same inputs, same bits)
							const uint32_t at = queued + (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(q >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)q, 0u));
							queue[at] = t | p << 7 | ia << 8 | ib << 16 | ic << 24; // (t < 96; at < 96 * PIECES: each (t, p) once)
						}
						queued += (uint32_t)__builtin_popcountll(q);
					}
				}
			}
			rd_lds_order();

			// ---- large triangles, the whole wave: lane = pixel of an 8 x 8 stamp
			for (uint32_t k = 0; k < queued; ++k)
			{
				const uint32_t e = queue[k];
				RdTri tri;
				decltype(rd_id<STABLE>(0u, 0u, 0u)) id;
				if constexpr (CLIP)
				{
					const uint32_t ia = e >> 8 & 0xffu, ib = e >> 16 & 0xffu, ic = e >> 24; // (< ve: it was queued)
					const bool second = (e & 0x80u) != 0u;
					int4 p0, p1, p2, p3;
					rd_clip(a.globals, vtx[ia], vtx[ib], vtx[ic], cvx[ia], cvx[ib], cvx[ic], H, p0, p1, p2, p3);
					rd_setup_corners(p0, rd_sel(second, p2, p1), rd_sel(second, p3, p2), bothFaces, W, H, tri); // (true: it was queued)
					id = rd_id<STABLE>(index, mvi, e & 0x7fu);
				}
				else
				{
					rd_setup(vtx, e >> 8 & 0xffu, e >> 16 & 0xffu, e >> 24, ve, bothFaces, W, H, tri); // (true: it was queued)
					id = rd_id<STABLE>(index, mvi, e & 0xffu);
				}
				FaCorner ca = { 0.0f, 0.0f, 0.0f, 0u }, cb = ca, cc = ca;
				if constexpr (ALPHA)
					if (textured) // (the index bytes are at the same place of the entry in both forms; < ve: it was queued)
						ca = rd_corner(attr[e >> 8 & 0xffu]), cb = rd_corner(attr[e >> 16 & 0xffu]), cc = rd_corner(attr[e >> 24]);
				const uint32_t sw = (uint32_t)(tri.x1 - tri.x0) / 8u + 1u, sh = (uint32_t)(tri.y1 - tri.y0) / 8u + 1u;
				const int32_t lx = (int32_t)(lane & 7u), ly = (int32_t)(lane >> 3);
				for (uint32_t sy = 0; sy < sh; ++sy)
				{
					const int32_t py = tri.y0 + (int32_t)sy * 8 + ly;
					for (uint32_t sx = 0; sx < sw; ++sx)
					{
						const int32_t px = tri.x0 + (int32_t)sx * 8 + lx;
						if constexpr (ALPHA)
						{
							if (px <= tri.x1 && py <= tri.y1)
								rd_sample_alpha<STABLE, typename ARGS::Set>(tri, slot, a.tx.data, ca, cb, cc, px, py, a.width, fw, fh, a.depth,
								                                            STABLE ? vis : a.visibility, id, samples, dropped, unevaluated);
						}
						else if (px <= tri.x1 && py <= tri.y1)
							samples += rd_sample<STABLE>(tri, px, py, a.width, a.depth, STABLE ? vis : a.visibility, id) ? 1u : 0u;
					}
				}
			}
		}
	}

	// totals: per-workgroup partial sums, plain stores; rasterdepth_totals_kernel (rasterdepth.hip) adds them up (ALPHA: two more, dropped and unevaluated samples)
	constexpr int TOTALS = ALPHA ? 6 : 4;
	__shared__ unsigned long long s_tot[RD_WAVES][TOTALS];
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
		s_tot[wave][0] = clusters;
		s_tot[wave][1] = triangles;
		s_tot[wave][2] = d;
		s_tot[wave][3] = smp;
		if constexpr (ALPHA)
		{
			s_tot[wave][TOTALS - 2] = dropped;
			s_tot[wave][TOTALS - 1] = unevaluated;
		}
	}
	__syncthreads();
	if (threadIdx.x < TOTALS)
	{
		unsigned long long t = 0;
#pragma unroll
		for (int k = 0; k < RD_WAVES; ++k)
			t += s_tot[k][threadIdx.x];
		if (threadIdx.x < 4)
			a.partials[(size_t)blockIdx.x * 4 + threadIdx.x] = t;
		if constexpr (ALPHA)
			if (threadIdx.x >= 4 && a.alphaPartials)
				a.alphaPartials[(size_t)blockIdx.x * 2 + (threadIdx.x - 4)] = t;
	}
}

// The launch of one pass, for every ARGS: the kernel by near clip and id form, then the totals launches the caller asked for
template <bool ALPHA, typename ARGS>
int launch_rasterdepth_as(hipStream_t stream, const ARGS& a, uint32_t gridBlocks, bool nearClip, bool stableIds)
{
	gridBlocks = gridBlocks / 8 * RD_BLOCKS_PER_CU; // the caller passes 8 workgroups per CU, the size of `partials` and `alphaPartials`
	// (the stable form differs only in the visibility word: without a visibility target the launch is the default kernel)
	if (stableIds && a.visibility)
	{
		if (nearClip)
			hipLaunchKernelGGL((rasterdepth_kernel<true, true, ALPHA, ARGS>), dim3(gridBlocks), dim3(RD_THREADS), 0, stream, a);
		else
			hipLaunchKernelGGL((rasterdepth_kernel<false, true, ALPHA, ARGS>), dim3(gridBlocks), dim3(RD_THREADS), 0, stream, a);
	}
	else if (nearClip)
		hipLaunchKernelGGL((rasterdepth_kernel<true, false, ALPHA, ARGS>), dim3(gridBlocks), dim3(RD_THREADS), 0, stream, a);
	else
		hipLaunchKernelGGL((rasterdepth_kernel<false, false, ALPHA, ARGS>), dim3(gridBlocks), dim3(RD_THREADS), 0, stream, a);
	hipError_t e = hipGetLastError();
	if (e == hipSuccess && a.totals)
		e = (hipError_t)launch_raster_totals(stream, a.partials, gridBlocks, a.totals, 4);
	if constexpr (ALPHA)
		if (e == hipSuccess && a.alphaTotals)
			e = (hipError_t)launch_raster_totals(stream, a.alphaPartials, gridBlocks, a.alphaTotals, 2);
	return (int)e;
}

} // namespace nv
