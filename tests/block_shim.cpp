// block_shim.cpp — host-side window onto the block bound of niagara_amd/csrc/filtermath.h (block_record, block_planes, block_outside) for
// tests/test_block_cert.py: the SAME source the kernels compile, built with g++ -ffp-contract=off at test time.  Test infrastructure.
#include <cstddef>
#include <cstdint>

#include "../niagara_amd/csrc/filtermath.h"

extern "C" {

// words: 2 x u32 per meshlet (the mirror's bounds), n meshlets per block except the last; out: 4 x u32 per block
void shim_block_records(const uint32_t* words, unsigned count, unsigned blocks, uint32_t* out)
{
	for (unsigned b = 0; b < blocks; ++b)
	{
		const unsigned first = b * 64u, n = first < count ? (count - first < 64u ? count - first : 64u) : 0u;
		const nv::BlockRecord k = nv::block_record(words + 2 * (size_t)first, n);
		float c[3] = { k.c[0], k.c[1], k.c[2] };
		__builtin_memcpy(out + 4 * (size_t)b, c, 12);
		out[4 * (size_t)b + 3] = k.dr;
	}
}

uint32_t shim_half_up(double x) { return nv::fm_half_up(x); }

// rows: n x 14 floats {fold[8], mz[3], bz, scale, tK} per test; plane: {f1, f3, znear, zfar}; recs: n x 4 u32; out: n ints (1 = outside)
void shim_block_outside(unsigned n, const float* rows, const float plane[4], const uint32_t* recs, int* out)
{
	for (unsigned i = 0; i < n; ++i)
	{
		const float* r = rows + 14 * (size_t)i;
		nv::BlockRecord k;
		__builtin_memcpy(k.c, recs + 4 * (size_t)i, 12);
		k.dr = recs[4 * (size_t)i + 3];
		const nv::BlockPlanes p = nv::block_planes(r, r + 4, r + 8, plane[0], plane[1]);
		const float thrBase = nv::block_thr_base(r[13], plane[2], plane[3]);
		out[i] = nv::block_outside(r, r + 4, r + 8, r[11], p, plane[0], plane[1], plane[2], plane[3], r[12], thrBase, k) ? 1 : 0;
	}
}
}
