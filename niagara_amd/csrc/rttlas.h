// rttlas.h — the DEFINITION of the shadow trace's rebuilt TLAS in ONE place that compiles for the device (hipcc) and for the
// host (g++), as rtmath.h does for the traversal: which draws cast, the instance record, the padded world box of an instance (fp64, rounded
// outward: moved here from rtbuild.cpp with its arithmetic unchanged, nv_rt_scene_build writes the bytes it wrote before), the 30-bit Morton key
// of an instance and the preorder position of a node.  rttlas.hip's kernels and nv_rt_tlas_build_host run the same text, and the tree above the
// leaves is unique (the binary radix tree of the sorted strings key << 32 | k), so the two builds compare with == on bytes.
//
// Build with -ffp-contract=off.  No std:: calls, no libm calls: comparisons, fabs, and single IEEE operations in the order written.
#pragma once

#include "../../include/niagara_vis.h"
#include "rtmath.h"

#if defined(__clang__)
#define NV_TL_UNROLL _Pragma("unroll")
#else
#define NV_TL_UNROLL
#endif

namespace nv
{

struct TlBox
{
	float lo[3], hi[3];
};

NV_RT double tl_min(double a, double b) { return b < a ? b : a; } // std::min
NV_RT double tl_max(double a, double b) { return a < b ? b : a; } // std::max

// the neighbours of a finite or infinite float (nextafterf towards -inf / +inf; never called with a NaN)
NV_RT float tl_next_down(float f)
{
	const uint32_t u = rt_bits(f);
	const uint32_t v = (u << 1) == 0u ? 0x80000001u : ((u >> 31) ? u + 1u : u - 1u);
	float r;
	__builtin_memcpy(&r, &v, 4);
	return r;
}
NV_RT float tl_next_up(float f)
{
	const uint32_t u = rt_bits(f);
	const uint32_t v = (u << 1) == 0u ? 0x00000001u : ((u >> 31) ? u - 1u : u + 1u);
	float r;
	__builtin_memcpy(&r, &v, 4);
	return r;
}
NV_RT float tl_round_down(double v)
{
	const float f = (float)v;
	return (double)f > v ? tl_next_down(f) : f;
}
NV_RT float tl_round_up(double v)
{
	const float f = (float)v;
	return (double)f < v ? tl_next_up(f) : f;
}

// the casting rule of include/niagara_vis.h, without the BLAS (the caller adds "its mesh's BLAS has nodes")
NV_RT bool tl_draw_casts(const NvMeshDraw& d, uint32_t meshCount)
{
	bool finite = rt_finite(d.scale);
	for (int k = 0; k < 3; ++k)
		finite = finite && rt_finite(d.position[k]);
	for (int k = 0; k < 4; ++k)
		finite = finite && rt_finite(d.orientation[k]);
	return d.meshIndex < meshCount && finite && d.scale > 0.0f && d.postPass <= 1u;
}

NV_RT RtInstance tl_instance(const NvMeshDraw& d, uint32_t drawId)
{
	RtInstance in;
	for (int k = 0; k < 3; ++k)
		in.position[k] = d.position[k];
	in.scale = d.scale;
	for (int k = 0; k < 4; ++k)
		in.orientation[k] = d.orientation[k];
	in.drawId = drawId, in.postPass = d.postPass, in.blas = d.meshIndex;
	for (int k = 0; k < 5; ++k)
		in.reserved[k] = 0u;
	return in;
}

// The padded world box of an instance whose BLAS root box is `root` (DESIGN.md §4.16 "the TLAS box").  The object-space ray is
// L (x - p), L = M / s with M the matrix of rotateQuat(., conj(q)) (any finite q, unit or not), so the instance occupies p + s M^-1 (box).
// Static padding cB + cO max|p| is added here, the traversal adds padOrigin max|o| with padOrigin >= cO.  An instance whose map is singular
// or so ill-conditioned that cO would exceed 2^-10 gets the infinite box: it is never rejected.  All of it in fp64, rounded outward.
NV_RT TlBox tl_instance_box(const NvMeshDraw& d, const TlBox& root, float maxAbs, double* cO_)
{
	const float inf = __builtin_inff();
	const TlBox everything = { { -inf, -inf, -inf }, { inf, inf, inf } };
	*cO_ = 0.0;
	const double x = -(double)d.orientation[0], y = -(double)d.orientation[1], z = -(double)d.orientation[2], w = d.orientation[3], s = d.scale;
	// v + 2 c x (c x v + w v) = (I + 2 (C C + w C)) v, C = [c]x
	const double C[3][3] = { { 0, -z, y }, { z, 0, -x }, { -y, x, 0 } };
	double M[3][3];
NV_TL_UNROLL
	for (int r = 0; r < 3; ++r)
NV_TL_UNROLL
		for (int c = 0; c < 3; ++c)
		{
			double cc = 0;
NV_TL_UNROLL
			for (int k = 0; k < 3; ++k)
				cc += C[r][k] * C[k][c];
			M[r][c] = (r == c ? 1.0 : 0.0) + 2.0 * (cc + w * C[r][c]);
		}
	const double det = M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
	                   M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
	if (!(__builtin_fabs(det) > 0.0) || !(__builtin_fabs(det) < (double)inf))
		return everything;
	double I[3][3];
NV_TL_UNROLL
	for (int r = 0; r < 3; ++r)
NV_TL_UNROLL
		for (int c = 0; c < 3; ++c)
		{
			const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3; // cofactor of (c, r)
			I[r][c] = (M[r1][c1] * M[r2][c2] - M[r1][c2] * M[r2][c1]) / det;
		}
	double nM = 0, nI = 0; // infinity norms
NV_TL_UNROLL
	for (int r = 0; r < 3; ++r)
	{
		nM = tl_max(nM, __builtin_fabs(M[r][0]) + __builtin_fabs(M[r][1]) + __builtin_fabs(M[r][2]));
		nI = tl_max(nI, __builtin_fabs(I[r][0]) + __builtin_fabs(I[r][1]) + __builtin_fabs(I[r][2]));
	}
	const double Qa = __builtin_fabs(x) + __builtin_fabs(y) + __builtin_fabs(z), rotAbs = 1.0 + 2.0 * Qa * (Qa + __builtin_fabs(w)), kappa = nM * nI,
	             u = (double)RT_U, K = (double)RT_PAD_K;
	const double cO = u * (K * kappa + 16.0 * rotAbs * nI * (1.0 + kappa));
	const double cB = u * s * (double)maxAbs * nI * (K + 16.0 * rotAbs * nI);
	if (!(cO <= 0.0009765625) || !(cB < (double)inf))
		return everything;
	const double pmax = tl_max(tl_max(__builtin_fabs((double)d.position[0]), __builtin_fabs((double)d.position[1])), __builtin_fabs((double)d.position[2]));
	const double pad = (cB + cO * pmax) * 1.0000001;
	double lo[3] = { (double)inf, (double)inf, (double)inf }, hi[3] = { -(double)inf, -(double)inf, -(double)inf };
NV_TL_UNROLL
	for (int corner = 0; corner < 8; ++corner)
	{
		const double c[3] = { corner & 1 ? root.hi[0] : root.lo[0], corner & 2 ? root.hi[1] : root.lo[1], corner & 4 ? root.hi[2] : root.lo[2] };
NV_TL_UNROLL
		for (int r = 0; r < 3; ++r)
		{
			const double v = (double)d.position[r] + s * ((I[r][0] * c[0] + I[r][1] * c[1]) + I[r][2] * c[2]);
			lo[r] = tl_min(lo[r], v);
			hi[r] = tl_max(hi[r], v);
		}
	}
	TlBox b;
	bool nan = false;
NV_TL_UNROLL
	for (int r = 0; r < 3; ++r)
	{
		// the fp64 evaluation above errs by a few 2^-53 of its terms: far inside the padding's slack (RT_PAD_K is > 2 x what the analysis needs)
		b.lo[r] = tl_round_down(lo[r] - pad), b.hi[r] = tl_round_up(hi[r] + pad);
		nan = nan || !(b.lo[r] <= b.hi[r]);
	}
	if (nan)
		return everything;
	*cO_ = cO;
	return b;
}

// the floor of the scene's largest cO, and the header's padOrigin from that maximum
NV_RT double tl_pad_floor() { return (double)RT_PAD_K * (double)RT_U; }
NV_RT float tl_pad_origin(double cOmax) { return tl_round_up(tl_max(tl_pad_floor(), cOmax) * 1.0000001); }

// ---- min and max of box coordinates and middles (never NaN): by the order-preserving bit pattern, so that -0 < +0 and the result does not
// depend on the order of the operands — an atomic min / max over integers, a pyramid and a pairwise union give the same bits
NV_RT uint32_t tl_ord(float f)
{
	const uint32_t u = rt_bits(f);
	return (u >> 31) ? ~u : u | 0x80000000u;
}
NV_RT float tl_unord(uint32_t o)
{
	const uint32_t u = (o >> 31) ? o & 0x7fffffffu : ~o;
	float r;
	__builtin_memcpy(&r, &u, 4);
	return r;
}
NV_RT float tl_fmin(float a, float b) { return tl_ord(b) < tl_ord(a) ? b : a; }
NV_RT float tl_fmax(float a, float b) { return tl_ord(b) > tl_ord(a) ? b : a; }

// ---- the key

// the sort key of a box along an axis: its middle (0 for a middle that is not finite: such a box is never rejected, where it sorts is free)
NV_RT float tl_mid(float lo, float hi)
{
	const float m = lo * 0.5f + hi * 0.5f;
	return rt_finite(m) ? m : 0.0f;
}

// The cell 0..1023 of the middle m within the scene's middle range [lo, hi] (lo <= m <= hi, all finite).  Halves first: hi - lo may overflow,
// hi/2 - lo/2 cannot.  Rounding is monotone, so num <= ext and t is in [0, 1]; the two selects make the conversion defined whatever comes in
// (a NaN becomes 0).  An axis with !(hi > lo), or whose halved extent rounds to 0, gives 0.
NV_RT uint32_t tl_cell(float m, float lo, float hi)
{
	if (!(hi > lo))
		return 0u;
	const float ext = hi * 0.5f - lo * 0.5f;
	if (!(ext > 0.0f))
		return 0u;
	const float num = m * 0.5f - lo * 0.5f;
	const float t = num / ext;
	float c = t * 1024.0f;
	c = c > 0.0f ? c : 0.0f;
	c = c < 1023.0f ? c : 1023.0f;
	return (uint32_t)c;
}

NV_RT uint32_t tl_spread3(uint32_t v) // 10 bits -> every third bit
{
	v = (v | v << 16) & 0x030000ffu;
	v = (v | v << 8) & 0x0300f00fu;
	v = (v | v << 4) & 0x030c30c3u;
	v = (v | v << 2) & 0x09249249u;
	return v;
}
NV_RT uint32_t tl_morton(uint32_t qx, uint32_t qy, uint32_t qz) { return tl_spread3(qx) << 2 | tl_spread3(qy) << 1 | tl_spread3(qz); }

constexpr uint32_t TL_KEY_NONE = 1u << 30; // the key of a draw that does not cast: above every caster's, it sorts behind them

// midLo / midHi: the min / max of the instances' middles per axis
NV_RT uint32_t tl_key(const TlBox& b, const float* midLo, const float* midHi)
{
	return tl_morton(tl_cell(tl_mid(b.lo[0], b.hi[0]), midLo[0], midHi[0]), tl_cell(tl_mid(b.lo[1], b.hi[1]), midLo[1], midHi[1]),
	                 tl_cell(tl_mid(b.lo[2], b.hi[2]), midLo[2], midHi[2]));
}

// ---- the tree: the binary radix tree of the n distinct strings key[k] << 32 | k over the sorted instances k (Karras, HPG 2012)

NV_RT uint64_t tl_string(uint32_t key, uint32_t k) { return (uint64_t)key << 32 | k; }

// Layout (§4.16's preorder with skip links): a node over the leaves [l, r] at `lefts` left-child edges below the root sits at 2 l + lefts
// (in front of it lie its ancestors and the complete subtrees over the leaves [0, l): 2 l nodes less one per right-child edge, plus one
// per edge), and the index behind its subtree is pos + 2 (r - l + 1) - 1.
NV_RT uint32_t tl_pos(uint32_t l, uint32_t lefts) { return 2u * l + lefts; }
NV_RT uint32_t tl_skip(uint32_t pos, uint32_t l, uint32_t r) { return pos + 2u * (r - l + 1u) - 1u; }
constexpr uint32_t TL_MAX_DEPTH = 64; // the strings have 64 bits: a longer walk along parent links is cut off


// where nv_rt_scene_reserve_dynamic puts things in its one allocation (byte offsets; rttlas.hip tlas_plan)
struct TlasPlan
{
	uint64_t bytes, tlasOff, instOff, counters, boxes, keysA, keysB, idxA, idxB, hist, range, parentInner, parentLeaf, pyramid;
	uint32_t pyramidP, maxDraws; // maxDraws == 0: no reservation
};

} // namespace nv
