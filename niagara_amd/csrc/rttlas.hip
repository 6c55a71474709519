// rttlas.hip — nv_rt_tlas_build for gfx950: the shadow trace's TLAS rebuilt on the device from the current draw records, so
// that moving draws do not go through the host.  The DEFINITION is rttlas.h (one text with nv_rt_tlas_build_host): which draws cast, their
// fp64 boxes, the Morton key, the order (key, drawId) and the binary radix tree of the strings key << 32 | k.  The tree is unique, so this
// file's construction (Karras, HPG 2012: every inner node finds its range from neighbouring strings) and the host's recursion give the same
// bytes.  shadowtrace.hip is untouched: it reads tlasNodes, tlasOff, instOff and padOrigin from the device header, which the last launch
// here rewrites.
//
// Shape.  NO launch hands data from one workgroup to another: every dependency is a launch boundary.
//   1 instances   a lane per draw: casting rule, fp64 box, cO; the middles' min / max and the largest cO by integer atomics on order-preserving
//                 bits, pre-aggregated per wave, one counter per 64-byte line (min / max do not depend on the order: the bytes are deterministic)
//   2 keys        a lane per draw: the key (TL_KEY_NONE for a draw that does not cast: it sorts to the end), and the number n of casters
//   3 sort        stable LSD radix sort of (key, draw) pairs, 8 bits x 4 passes, each: per-workgroup digit counts / one workgroup scans them /
//                 a stable scatter whose ranks are taken in LDS.  The pairs start in ascending draw order: stable = the (key, drawId) order
//   4 tree        a lane per inner node: range and split from clz of neighbouring strings; a parent link (parent << 1 | is-left-child) per node
//   5 pyramid     aligned min / max blocks over the sorted leaf boxes, 9 levels per launch in LDS (depthreduce.hip's manner)
//   6 emit        a lane per node: pos = 2 l + left-child edges above it (a walk along parent links, capped at TL_MAX_DEPTH steps), the box of
//                 [l, r] from at most 2 log2 n aligned pyramid blocks, the RtNode as two 16-byte stores; a leaf's lane writes its RtInstance
//   7 header      one lane: tlasNodes, instances, tlasOff, instOff, padOrigin, drawCount (plain vector stores)
// All grids are sized by drawCount (the host does not know n); lanes beyond n leave.  Nothing is read that this build did not write: the
// scratch may hold anything (a smaller build behind a larger one, 0xAB poison).
//
// Why a rebuilt TLAS passes nv_rt_scene_validate by construction: a node over [l, r] has pos = 2 l + lefts and skip = pos + 2 (r - l + 1) - 1,
// so skip > pos (r >= l); the subtree of a node occupies [pos, skip) and lies inside its parent's, the root's is [0, 2 n - 1), so
// skip <= 2 n - 1 = tlasNodes; a leaf word is 1 << RT_LEAF_SHIFT | k with k < n = instances: count 1, first in range; an instance's blas is a
// meshIndex the casting rule held below meshCount.  The emit lanes also refuse to store outside [0, 2 n - 1) whatever the links hold.
#include <hip/hip_runtime.h>

#include "rttlas.h"
#include "launch.h"

namespace nv
{

constexpr int TL_THREADS = 256;
constexpr uint32_t TL_SORT_KEYS = 2048; // keys per workgroup of the sort's histogram and scatter launches
constexpr uint32_t TL_SORT_CHUNKS = TL_SORT_KEYS / TL_THREADS;
constexpr uint32_t TL_PYR_STEP = 9;               // pyramid levels per launch
constexpr uint32_t TL_PYR_BLOCK = 1u << TL_PYR_STEP; // entries of the source level per workgroup
constexpr uint32_t TL_NONE = 0xffffffffu;         // the root's parent link
// counters: one per 64-byte line (16 words)
constexpr uint32_t TL_C_MIDLO = 0, TL_C_MIDHI = 3, TL_C_PAD = 6, TL_C_COUNT = 7, TL_C_LINES = 8, TL_C_WORDS = 16;

struct TlasArgs
{
	unsigned char* scene; // the allocation: static blob (header first), dynamic sections, scratch
	const NvMeshDraw* __restrict__ draws;
	uint32_t drawCount;
	uint32_t tlasOff, instOff; // the dynamic sections
	uint32_t* counters;
	RtF4* boxes; // per draw: {lo, casts} {hi, 0}
	uint32_t *keysA, *keysB, *idxA, *idxB;
	uint32_t* hist; // [workgroup][256] digit counts, then [256] digit bases
	uint2* range;   // per inner node
	uint32_t *parentInner, *parentLeaf;
	RtF4* pyramid; // level j at entry 2 P - (2 P >> j), P >> j entries of two RtF4
	uint32_t pyramidP;
	uint32_t sortGroups;
};

__device__ inline uint32_t tl_count(const TlasArgs& a) // the number of casters, never above drawCount
{
	const uint32_t n = a.counters[TL_C_COUNT * TL_C_WORDS];
	return n < a.drawCount ? n : a.drawCount;
}

// ---- 1 instances

__global__ __launch_bounds__(TL_THREADS) void tlas_instances_kernel(TlasArgs a)
{
	const uint32_t i = blockIdx.x * TL_THREADS + threadIdx.x;
	const RtHeader* h = reinterpret_cast<const RtHeader*>(a.scene);
	bool casts = false;
	double cO = 0.0;
	TlBox b = { { 0.0f, 0.0f, 0.0f }, { 0.0f, 0.0f, 0.0f } };
	if (i < a.drawCount)
	{
		const NvMeshDraw d = a.draws[i];
		if (tl_draw_casts(d, h->meshCount))
		{
			const RtBlas e = reinterpret_cast<const RtBlas*>(a.scene + h->tableOff)[d.meshIndex];
			if (e.nodeCount != 0u)
			{
				const RtF4* rn = reinterpret_cast<const RtF4*>(a.scene + h->blasOff) + 2u * (size_t)e.nodeFirst;
				const RtF4 rlo = rn[0], rhi = rn[1];
				const TlBox root = { { rlo.x, rlo.y, rlo.z }, { rhi.x, rhi.y, rhi.z } };
				b = tl_instance_box(d, root, e.maxAbs, &cO);
				casts = true;
			}
		}
		RtF4 lo = { b.lo[0], b.lo[1], b.lo[2], 0.0f }, hi = { b.hi[0], b.hi[1], b.hi[2], 0.0f };
		lo.w = __uint_as_float(casts ? 1u : 0u);
		a.boxes[2u * (size_t)i] = lo;
		a.boxes[2u * (size_t)i + 1u] = hi;
	}
	uint32_t mlo0 = 0xffffffffu, mlo1 = 0xffffffffu, mlo2 = 0xffffffffu, mhi0 = 0u, mhi1 = 0u, mhi2 = 0u;
	unsigned long long pad = 0ull; // cO >= 0: its bits order as unsigned integers
	if (casts)
	{
		mlo0 = mhi0 = tl_ord(tl_mid(b.lo[0], b.hi[0]));
		mlo1 = mhi1 = tl_ord(tl_mid(b.lo[1], b.hi[1]));
		mlo2 = mhi2 = tl_ord(tl_mid(b.lo[2], b.hi[2]));
		pad = (unsigned long long)__double_as_longlong(cO);
	}
	for (int m = 32; m >= 1; m >>= 1)
	{
		mlo0 = min(mlo0, (uint32_t)__shfl_xor((int)mlo0, m));
		mlo1 = min(mlo1, (uint32_t)__shfl_xor((int)mlo1, m));
		mlo2 = min(mlo2, (uint32_t)__shfl_xor((int)mlo2, m));
		mhi0 = max(mhi0, (uint32_t)__shfl_xor((int)mhi0, m));
		mhi1 = max(mhi1, (uint32_t)__shfl_xor((int)mhi1, m));
		mhi2 = max(mhi2, (uint32_t)__shfl_xor((int)mhi2, m));
		const unsigned long long o = (unsigned long long)__shfl_xor((long long)pad, m);
		pad = o > pad ? o : pad;
	}
	if ((threadIdx.x & 63u) == 0u && mhi0 != 0u) // a wave with a caster
	{
		atomicMin(&a.counters[(TL_C_MIDLO + 0u) * TL_C_WORDS], mlo0);
		atomicMin(&a.counters[(TL_C_MIDLO + 1u) * TL_C_WORDS], mlo1);
		atomicMin(&a.counters[(TL_C_MIDLO + 2u) * TL_C_WORDS], mlo2);
		atomicMax(&a.counters[(TL_C_MIDHI + 0u) * TL_C_WORDS], mhi0);
		atomicMax(&a.counters[(TL_C_MIDHI + 1u) * TL_C_WORDS], mhi1);
		atomicMax(&a.counters[(TL_C_MIDHI + 2u) * TL_C_WORDS], mhi2);
		atomicMax(reinterpret_cast<unsigned long long*>(&a.counters[TL_C_PAD * TL_C_WORDS]), pad);
	}
}

// ---- 2 keys

__global__ __launch_bounds__(TL_THREADS) void tlas_keys_kernel(TlasArgs a)
{
	const uint32_t i = blockIdx.x * TL_THREADS + threadIdx.x;
	bool casts = false;
	if (i < a.drawCount)
	{
		const RtF4 lo = a.boxes[2u * (size_t)i], hi = a.boxes[2u * (size_t)i + 1u];
		casts = __float_as_uint(lo.w) == 1u;
		uint32_t key = TL_KEY_NONE;
		if (casts)
		{
			const float midLo[3] = { tl_unord(a.counters[(TL_C_MIDLO + 0u) * TL_C_WORDS]), tl_unord(a.counters[(TL_C_MIDLO + 1u) * TL_C_WORDS]),
				                     tl_unord(a.counters[(TL_C_MIDLO + 2u) * TL_C_WORDS]) };
			const float midHi[3] = { tl_unord(a.counters[(TL_C_MIDHI + 0u) * TL_C_WORDS]), tl_unord(a.counters[(TL_C_MIDHI + 1u) * TL_C_WORDS]),
				                     tl_unord(a.counters[(TL_C_MIDHI + 2u) * TL_C_WORDS]) };
			const TlBox b = { { lo.x, lo.y, lo.z }, { hi.x, hi.y, hi.z } };
			key = tl_key(b, midLo, midHi);
		}
		a.keysA[i] = key;
		a.idxA[i] = i;
	}
	const unsigned long long m = __ballot(casts);
	if ((threadIdx.x & 63u) == 0u && m != 0ull)
		atomicAdd(&a.counters[TL_C_COUNT * TL_C_WORDS], (uint32_t)__popcll(m));
}

// ---- 3 sort: one pass = the three launches below on the digit (key >> shift) & 255

__global__ __launch_bounds__(TL_THREADS) void tlas_sort_count_kernel(const uint32_t* __restrict__ keys, uint32_t count, uint32_t shift, uint32_t* hist)
{
	__shared__ uint32_t digits[256];
	digits[threadIdx.x] = 0u;
	__syncthreads();
	const uint32_t base = blockIdx.x * TL_SORT_KEYS;
	for (uint32_t c = 0; c < TL_SORT_CHUNKS; ++c)
	{
		const uint32_t i = base + c * TL_THREADS + threadIdx.x;
		if (i < count)
			atomicAdd(&digits[(keys[i] >> shift) & 255u], 1u);
	}
	__syncthreads();
	hist[(size_t)blockIdx.x * 256u + threadIdx.x] = digits[threadIdx.x];
}

// one workgroup: hist[g][d] becomes the number of keys with digit d in the workgroups before g, hist[groups][d] the number of keys with a
// smaller digit
__global__ __launch_bounds__(TL_THREADS) void tlas_sort_scan_kernel(uint32_t* hist, uint32_t groups)
{
	__shared__ uint32_t sums[2][256];
	const uint32_t d = threadIdx.x;
	uint32_t total = 0u;
	for (uint32_t g = 0; g < groups; ++g)
	{
		const uint32_t v = hist[(size_t)g * 256u + d];
		hist[(size_t)g * 256u + d] = total;
		total += v;
	}
	sums[0][d] = total;
	__syncthreads();
	uint32_t cur = 0u;
	for (uint32_t step = 1u; step < 256u; step <<= 1) // inclusive scan over the digits
	{
		const uint32_t v = sums[cur][d] + (d >= step ? sums[cur][d - step] : 0u);
		sums[cur ^ 1u][d] = v;
		cur ^= 1u;
		__syncthreads();
	}
	hist[(size_t)groups * 256u + d] = sums[cur][d] - total;
}

__global__ __launch_bounds__(TL_THREADS) void tlas_sort_scatter_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ idx, uint32_t* keysOut,
                                                                       uint32_t* idxOut, uint32_t count, uint32_t shift, const uint32_t* __restrict__ hist,
                                                                       uint32_t groups)
{
	__shared__ uint32_t next[256];        // where the next key of a digit goes
	__shared__ uint32_t waveCount[4][256]; // keys per digit and wave of the current chunk
	const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
	next[tid] = hist[(size_t)groups * 256u + tid] + hist[(size_t)blockIdx.x * 256u + tid];
	const uint32_t base = blockIdx.x * TL_SORT_KEYS;
	for (uint32_t c = 0; c < TL_SORT_CHUNKS; ++c)
	{
		const uint32_t i = base + c * TL_THREADS + tid;
		const bool valid = i < count;
		const uint32_t key = valid ? keys[i] : 0u, id = valid ? idx[i] : 0u;
		const uint32_t digit = (key >> shift) & 255u;
		// the lanes of this wave with the same digit
		unsigned long long peers = __ballot(valid);
		for (uint32_t bit = 0; bit < 8u; ++bit)
		{
			const bool one = (digit >> bit) & 1u;
			const unsigned long long m = __ballot(one);
			peers &= one ? m : ~m;
		}
		const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
		waveCount[0][tid] = 0u, waveCount[1][tid] = 0u, waveCount[2][tid] = 0u, waveCount[3][tid] = 0u;
		__syncthreads();
		if (valid && rank == 0u)
			waveCount[wave][digit] = (uint32_t)__popcll(peers);
		__syncthreads();
		if (valid)
		{
			uint32_t at = next[digit] + rank;
			at += wave > 0u ? waveCount[0][digit] : 0u;
			at += wave > 1u ? waveCount[1][digit] : 0u;
			at += wave > 2u ? waveCount[2][digit] : 0u;
			if (at < count) // always, with counts taken from these keys
			{
				keysOut[at] = key;
				idxOut[at] = id;
			}
		}
		__syncthreads();
		next[tid] += (waveCount[0][tid] + waveCount[1][tid]) + (waveCount[2][tid] + waveCount[3][tid]);
	}
}

// ---- 4 tree

// the length of the common prefix of the strings of i and j, -1 outside [0, n)
__device__ inline int tl_delta(const uint32_t* __restrict__ keys, uint32_t n, uint32_t i, uint64_t si, long long j)
{
	if (j < 0 || j >= (long long)n)
		return -1;
	return __clzll((long long)(si ^ tl_string(keys[j], (uint32_t)j)));
}

__global__ __launch_bounds__(TL_THREADS) void tlas_tree_kernel(TlasArgs a)
{
	const uint32_t n = tl_count(a);
	const uint32_t i = blockIdx.x * TL_THREADS + threadIdx.x;
	if (n == 1u && i == 0u)
		a.parentLeaf[0] = TL_NONE;
	if (n < 2u || i >= n - 1u)
		return;
	const uint32_t* keys = a.keysA;
	const uint64_t si = tl_string(keys[i], i);
	const long long d = tl_delta(keys, n, i, si, (long long)i + 1) > tl_delta(keys, n, i, si, (long long)i - 1) ? 1 : -1; // never equal: the strings differ
	const int dmin = tl_delta(keys, n, i, si, (long long)i - d);
	long long lmax = 2;
	for (int it = 0; it < 32 && tl_delta(keys, n, i, si, (long long)i + lmax * d) > dmin; ++it)
		lmax *= 2;
	long long l = 0;
	for (long long t = lmax / 2; t >= 1; t /= 2)
		if (tl_delta(keys, n, i, si, (long long)i + (l + t) * d) > dmin)
			l += t;
	const long long j = (long long)i + l * d;
	const int dnode = tl_delta(keys, n, i, si, j);
	long long s = 0, t = l;
	for (int it = 0; it < 40; ++it)
	{
		t = (t + 1) / 2;
		if (tl_delta(keys, n, i, si, (long long)i + (s + t) * d) > dnode)
			s += t;
		if (t <= 1)
			break;
	}
	const long long gamma = (long long)i + s * d + (d < 0 ? -1 : 0);
	const uint32_t first = (uint32_t)(d > 0 ? (long long)i : j), last = (uint32_t)(d > 0 ? j : (long long)i);
	const uint32_t g = (uint32_t)gamma;
	if (i == 0u)
		a.parentInner[0] = TL_NONE;
	if (last >= n || g >= n - 1u) // cannot be
		return;
	a.range[i] = make_uint2(first, last);
	if (first == g)
		a.parentLeaf[g] = i << 1 | 1u;
	else
		a.parentInner[g] = i << 1 | 1u;
	if (last == g + 1u)
		a.parentLeaf[g + 1u] = i << 1;
	else
		a.parentInner[g + 1u] = i << 1;
}

// ---- 5 pyramid: level `src` -> levels src + 1 .. src + 9 (src == 0: the sorted leaf boxes are gathered into level 0 first)

__device__ inline size_t tl_level(uint32_t P, uint32_t level) { return level > 31u ? 2u * (size_t)P : 2u * (size_t)P - ((2u * (size_t)P) >> level); }

__global__ __launch_bounds__(TL_THREADS) void tlas_pyramid_kernel(TlasArgs a, uint32_t src)
{
	__shared__ RtF4 lo[TL_PYR_BLOCK], hi[TL_PYR_BLOCK];
	const uint32_t n = tl_count(a), P = a.pyramidP;
	const uint32_t entries = (uint32_t)(((uint64_t)n + (1ull << src) - 1ull) >> src); // of the source level that hold a leaf
	const uint32_t base = blockIdx.x * TL_PYR_BLOCK;
	if (base >= entries)
		return;
	const float inf = __builtin_inff();
	for (uint32_t e = threadIdx.x; e < TL_PYR_BLOCK; e += TL_THREADS)
	{
		const uint32_t g = base + e;
		const bool live = g < entries && g < (P >> src);
		size_t at = 0; // of the entry's first RtF4 in its array
		const RtF4* from = a.pyramid;
		bool read = live;
		if (src == 0u)
		{
			const uint32_t draw = live ? a.idxA[g] : 0u;
			read = live && draw < a.drawCount;
			from = a.boxes, at = 2u * (size_t)draw;
		}
		else
			at = 2u * (tl_level(P, src) + g);
		const RtF4 rl = from[read ? at : 0u], rh = from[read ? at + 1u : 1u];
		const RtF4 l = { read ? rl.x : inf, read ? rl.y : inf, read ? rl.z : inf, 0.0f }, h = { read ? rh.x : -inf, read ? rh.y : -inf, read ? rh.z : -inf, 0.0f };
		if (src == 0u && live)
		{
			a.pyramid[2u * (size_t)g] = l;
			a.pyramid[2u * (size_t)g + 1u] = h;
		}
		lo[e] = l, hi[e] = h;
	}
	for (uint32_t s = 1u; s <= TL_PYR_STEP; ++s)
	{
		__syncthreads();
		for (uint32_t t = threadIdx.x; t < (TL_PYR_BLOCK >> s); t += TL_THREADS)
		{
			const uint32_t x = t << s, y = x + (1u << (s - 1u));
			const RtF4 l = { tl_fmin(lo[x].x, lo[y].x), tl_fmin(lo[x].y, lo[y].y), tl_fmin(lo[x].z, lo[y].z), 0.0f };
			const RtF4 h = { tl_fmax(hi[x].x, hi[y].x), tl_fmax(hi[x].y, hi[y].y), tl_fmax(hi[x].z, hi[y].z), 0.0f };
			lo[x] = l, hi[x] = h;
			const uint32_t g = (base >> s) + t;
			if (src + s < 32u && g < (P >> (src + s)))
			{
				a.pyramid[2u * (tl_level(P, src + s) + g)] = l;
				a.pyramid[2u * (tl_level(P, src + s) + g) + 1u] = h;
			}
		}
	}
}

// ---- 6 emit

__global__ __launch_bounds__(TL_THREADS) void tlas_emit_kernel(TlasArgs a)
{
	const uint32_t n = tl_count(a);
	const uint32_t t = blockIdx.x * TL_THREADS + threadIdx.x;
	if (n == 0u || t >= 2u * n - 1u)
		return;
	const bool leaf = t < n;
	uint32_t l, r, p;
	if (leaf)
		l = r = t, p = a.parentLeaf[t];
	else
	{
		const uint2 lr = a.range[t - n];
		l = lr.x, r = lr.y, p = a.parentInner[t - n];
	}
	uint32_t lefts = 0u;
	for (uint32_t step = 0; step < TL_MAX_DEPTH && p != TL_NONE && (p >> 1) < n - 1u; ++step)
	{
		lefts += p & 1u;
		p = a.parentInner[p >> 1];
	}
	const uint32_t pos = tl_pos(l, lefts);
	if (l > r || r >= n || pos >= 2u * n - 1u) // cannot be: nothing is stored outside the section whatever the links hold
		return;
	const uint32_t P = a.pyramidP;
	RtF4 lo, hi;
	if (leaf)
		lo = a.pyramid[2u * (size_t)t], hi = a.pyramid[2u * (size_t)t + 1u];
	else
	{
		const float inf = __builtin_inff();
		lo = RtF4{ inf, inf, inf, 0.0f }, hi = RtF4{ -inf, -inf, -inf, 0.0f };
		uint32_t x = l, y = r + 1u;
		for (uint32_t level = 0; level < 32u && x < y; ++level) // [x, y) in entries of `level`
		{
			if (x & 1u)
			{
				if (x < (P >> level))
				{
					const RtF4 bl = a.pyramid[2u * (tl_level(P, level) + x)], bh = a.pyramid[2u * (tl_level(P, level) + x) + 1u];
					lo = RtF4{ tl_fmin(lo.x, bl.x), tl_fmin(lo.y, bl.y), tl_fmin(lo.z, bl.z), 0.0f };
					hi = RtF4{ tl_fmax(hi.x, bh.x), tl_fmax(hi.y, bh.y), tl_fmax(hi.z, bh.z), 0.0f };
				}
				++x;
			}
			if (y & 1u)
			{
				--y;
				if (y < (P >> level))
				{
					const RtF4 bl = a.pyramid[2u * (tl_level(P, level) + y)], bh = a.pyramid[2u * (tl_level(P, level) + y) + 1u];
					lo = RtF4{ tl_fmin(lo.x, bl.x), tl_fmin(lo.y, bl.y), tl_fmin(lo.z, bl.z), 0.0f };
					hi = RtF4{ tl_fmax(hi.x, bh.x), tl_fmax(hi.y, bh.y), tl_fmax(hi.z, bh.z), 0.0f };
				}
			}
			x >>= 1, y >>= 1;
		}
	}
	lo.w = __uint_as_float(tl_skip(pos, l, r));
	hi.w = __uint_as_float(leaf ? (1u << RT_LEAF_SHIFT | t) : 0u);
	RtF4* nodes = reinterpret_cast<RtF4*>(a.scene + a.tlasOff);
	nodes[2u * (size_t)pos] = lo;
	nodes[2u * (size_t)pos + 1u] = hi;
	if (leaf)
	{
		const uint32_t draw = a.idxA[t];
		if (draw >= a.drawCount)
			return;
		const RtInstance in = tl_instance(a.draws[draw], draw);
		RtF4* out = reinterpret_cast<RtF4*>(a.scene + a.instOff) + 4u * (size_t)t;
		out[0] = RtF4{ in.position[0], in.position[1], in.position[2], in.scale };
		out[1] = RtF4{ in.orientation[0], in.orientation[1], in.orientation[2], in.orientation[3] };
		out[2] = RtF4{ __uint_as_float(in.drawId), __uint_as_float(in.postPass), __uint_as_float(in.blas), 0.0f };
		out[3] = RtF4{ 0.0f, 0.0f, 0.0f, 0.0f };
	}
}

// ---- 7 header

__global__ __launch_bounds__(64) void tlas_header_kernel(TlasArgs a)
{
	if (blockIdx.x != 0u || threadIdx.x != 0u)
		return;
	const uint32_t n = tl_count(a);
	RtHeader* h = reinterpret_cast<RtHeader*>(a.scene);
	const double cOmax = __longlong_as_double((long long)*reinterpret_cast<const unsigned long long*>(&a.counters[TL_C_PAD * TL_C_WORDS]));
	h->tlasNodes = n ? 2u * n - 1u : 0u;
	h->instances = n;
	h->tlasOff = a.tlasOff;
	h->instOff = a.instOff;
	h->padOrigin = tl_pad_origin(cOmax);
	h->drawCount = a.drawCount;
}

// ---- host side

uint32_t tlas_sort_keys_per_workgroup() { return TL_SORT_KEYS; }

static uint64_t tl_align(uint64_t v) { return (v + 255u) & ~(uint64_t)255u; }

// The allocation of nv_rt_scene_reserve_dynamic: [static blob] [2 maxDraws TLAS nodes] [maxDraws instances] [scratch]; 0 when it does not
// fit the header's 32-bit offsets
uint64_t tlas_plan(uint64_t staticBytes, uint32_t maxDraws, TlasPlan* plan)
{
	uint32_t P = 1u;
	while (P < maxDraws && P < (1u << 30))
		P <<= 1;
	const uint64_t groups = ((uint64_t)maxDraws + TL_SORT_KEYS - 1u) / TL_SORT_KEYS;
	uint64_t at = tl_align(staticBytes);
	plan->tlasOff = at, at = tl_align(at + 2ull * maxDraws * sizeof(RtNode));
	plan->instOff = at, at = tl_align(at + (uint64_t)maxDraws * sizeof(RtInstance));
	plan->counters = at, at = tl_align(at + TL_C_LINES * TL_C_WORDS * 4u);
	plan->boxes = at, at = tl_align(at + (uint64_t)maxDraws * 32u);
	plan->keysA = at, at = tl_align(at + (uint64_t)maxDraws * 4u);
	plan->keysB = at, at = tl_align(at + (uint64_t)maxDraws * 4u);
	plan->idxA = at, at = tl_align(at + (uint64_t)maxDraws * 4u);
	plan->idxB = at, at = tl_align(at + (uint64_t)maxDraws * 4u);
	plan->hist = at, at = tl_align(at + (groups + 1u) * 256u * 4u);
	plan->range = at, at = tl_align(at + (uint64_t)maxDraws * 8u);
	plan->parentInner = at, at = tl_align(at + (uint64_t)maxDraws * 4u);
	plan->parentLeaf = at, at = tl_align(at + (uint64_t)maxDraws * 4u);
	plan->pyramid = at, at = tl_align(at + 2ull * P * 32u);
	plan->pyramidP = P;
	plan->maxDraws = maxDraws;
	plan->bytes = at;
	return at > 0xffffffffull ? 0u : at;
}

int launch_tlas_build(hipStream_t stream, void* scene, const TlasPlan& plan, const NvMeshDraw* draws, uint32_t drawCount)
{
	unsigned char* base = static_cast<unsigned char*>(scene);
	TlasArgs a;
	a.scene = base;
	a.draws = draws;
	a.drawCount = drawCount;
	a.tlasOff = (uint32_t)plan.tlasOff, a.instOff = (uint32_t)plan.instOff;
	a.counters = reinterpret_cast<uint32_t*>(base + plan.counters);
	a.boxes = reinterpret_cast<RtF4*>(base + plan.boxes);
	a.keysA = reinterpret_cast<uint32_t*>(base + plan.keysA), a.keysB = reinterpret_cast<uint32_t*>(base + plan.keysB);
	a.idxA = reinterpret_cast<uint32_t*>(base + plan.idxA), a.idxB = reinterpret_cast<uint32_t*>(base + plan.idxB);
	a.hist = reinterpret_cast<uint32_t*>(base + plan.hist);
	a.range = reinterpret_cast<uint2*>(base + plan.range);
	a.parentInner = reinterpret_cast<uint32_t*>(base + plan.parentInner), a.parentLeaf = reinterpret_cast<uint32_t*>(base + plan.parentLeaf);
	a.pyramid = reinterpret_cast<RtF4*>(base + plan.pyramid);
	a.pyramidP = plan.pyramidP;
	a.sortGroups = (drawCount + TL_SORT_KEYS - 1u) / TL_SORT_KEYS;
	// the min counters start at all ones, the max counters, the largest cO and the count at 0
	hipError_t e = hipMemsetAsync(a.counters, 0xff, TL_C_MIDHI * TL_C_WORDS * 4u, stream);
	if (e == hipSuccess)
		e = hipMemsetAsync(a.counters + TL_C_MIDHI * TL_C_WORDS, 0, (TL_C_LINES - TL_C_MIDHI) * TL_C_WORDS * 4u, stream);
	if (e != hipSuccess)
		return (int)e;
	if (drawCount)
	{
		const uint32_t perDraw = (drawCount + TL_THREADS - 1u) / TL_THREADS;
		hipLaunchKernelGGL(tlas_instances_kernel, dim3(perDraw), dim3(TL_THREADS), 0, stream, a);
		hipLaunchKernelGGL(tlas_keys_kernel, dim3(perDraw), dim3(TL_THREADS), 0, stream, a);
		uint32_t *kIn = a.keysA, *iIn = a.idxA, *kOut = a.keysB, *iOut = a.idxB;
		for (uint32_t shift = 0; shift < 32u; shift += 8u) // TL_KEY_NONE is bit 30: four passes, the pairs end where they began
		{
			hipLaunchKernelGGL(tlas_sort_count_kernel, dim3(a.sortGroups), dim3(TL_THREADS), 0, stream, kIn, drawCount, shift, a.hist);
			hipLaunchKernelGGL(tlas_sort_scan_kernel, dim3(1), dim3(TL_THREADS), 0, stream, a.hist, a.sortGroups);
			hipLaunchKernelGGL(tlas_sort_scatter_kernel, dim3(a.sortGroups), dim3(TL_THREADS), 0, stream, kIn, iIn, kOut, iOut, drawCount, shift, a.hist,
			                   a.sortGroups);
			uint32_t* s = kIn;
			kIn = kOut, kOut = s;
			s = iIn, iIn = iOut, iOut = s;
		}
		hipLaunchKernelGGL(tlas_tree_kernel, dim3(perDraw), dim3(TL_THREADS), 0, stream, a);
		for (uint32_t src = 0; src == 0u || (drawCount >> src) >= 2u; src += TL_PYR_STEP)
		{
			const uint32_t entries = (uint32_t)(((uint64_t)drawCount + (1ull << src) - 1ull) >> src);
			hipLaunchKernelGGL(tlas_pyramid_kernel, dim3((entries + TL_PYR_BLOCK - 1u) / TL_PYR_BLOCK), dim3(TL_THREADS), 0, stream, a, src);
		}
		hipLaunchKernelGGL(tlas_emit_kernel, dim3((2u * drawCount + TL_THREADS - 1u) / TL_THREADS), dim3(TL_THREADS), 0, stream, a);
	}
	hipLaunchKernelGGL(tlas_header_kernel, dim3(1), dim3(64), 0, stream, a);
	return (int)hipGetLastError();
}

} // namespace nv
