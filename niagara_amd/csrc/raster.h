// raster.h — the raster rules both depth rasterisers share: the vertex stage to snapped screen space, the triangle
// setup (rejection, facing, top-left flags, pixel box) and the per-sample coverage / depth / atomic.  rasterdepth.hip (the cluster path) and
// rasterindexed.hip (the indexed-draw path) use these statements and nothing else for what they write, so the same triangle under the same
// draw writes the same bits through either path; tests/raster_ref.c restates them one sample at a time.  With NV_OPT_RASTER_NEAR_CLIP both
// kernels also share rd_clip, the near-plane rule (tests/raster_clip_ref.c).  There is no clipping against the guard band or the viewport.
#pragma once

#include "cullmath.h"
#include "launch.h"

namespace nv
{

constexpr float RD_GUARD = 2097152.0f; // 2^21 pixels: every edge-function product stays below 2^62

NV_DEV uint32_t rd_rl(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }

// the wave is the workgroup of the reference's mesh shader: its LDS accesses are ordered, the compiler is told so
NV_DEV void rd_lds_order()
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a triangle ready to walk: corners with A > 0 (b and c swapped for a front face), top-left flags, 1 / A, pixel box (inclusive)
struct RdTri
{
	int32_t ax, ay, bx, by, cx, cy;
	float za, dzb, dzc, inv;
	int32_t x0, x1, y0, y1;
	uint32_t topLeft; // bit 0: a->b, bit 1: b->c, bit 2: c->a
};

// One vertex (the first 8 bytes of its record: fp16 x, y, z) under the draw {position, scale, orientation q.xyz, qw} to clip space.
// nv_trianglecull's arithmetic (src/shaders/meshlet.mesh.glsl:121-160; mesh.vert.glsl:41-57 computes the same).
NV_DEV void rd_clip_position(const NvGlobals& g, uint2 pv, f3 q, float qw, float scale, float px, float py, float pz, float clip[4])
{
	const f3 position = { half_bits_to_float(pv.x & 0xffffu), half_bits_to_float(pv.x >> 16), half_bits_to_float(pv.y & 0xffffu) };
	const f3 rot = rotate_quat(position, q, qw);
	const float wx = rot.x * scale + px, wy = rot.y * scale + py, wz = rot.z * scale + pz;
	const float* V = g.cullData.view;
	const float* P = g.projection;
	float v4[4];
#pragma unroll
	for (int r = 0; r < 4; ++r) // view * vec4(wpos, 1): c3 * 1.0f is c3 exactly
		v4[r] = ((V[r] * wx + V[4 + r] * wy) + V[8 + r] * wz) + V[12 + r];
#pragma unroll
	for (int r = 0; r < 4; ++r)
		clip[r] = ((P[r] * v4[0] + P[4 + r] * v4[1]) + P[8 + r] * v4[2]) + P[12 + r] * v4[3];
}

// A clip-space position to snapped screen space: X, Y with 8 sub-pixel bits (row 0 at the top), the bits of z = clip.z / clip.w, and 1 in
// .w when no triangle of it is drawn.
NV_DEV int4 rd_snap(const NvGlobals& g, const float clip[4], int32_t H)
{
	const float sx = ((clip[0] / clip[3]) * 0.5f + 0.5f) * g.screenWidth;
	const float sy = ((clip[1] / clip[3]) * 0.5f + 0.5f) * g.screenHeight;
	const float z = clip[2] / clip[3];
	// behind or in front of the near plane (NaN included), non-finite, or outside the guard band: no triangle of it is drawn
	const bool bad = !(clip[3] > 0.0f && clip[2] <= clip[3]) || !(__builtin_fabsf(sx) < RD_GUARD) || !(__builtin_fabsf(sy) < RD_GUARD);
	const int32_t X = bad ? 0 : (int32_t)__builtin_rintf(sx * 256.0f);
	const int32_t Y = bad ? 0 : H * 256 - (int32_t)__builtin_rintf(sy * 256.0f); // viewport flipped: row 0 at the top
	return make_int4(X, Y, __float_as_int(z), bad ? 1 : 0);
}

// One vertex to snapped screen space (rd_clip_position, then rd_snap).
NV_DEV int4 rd_vertex(const NvGlobals& g, uint2 pv, f3 q, float qw, float scale, float px, float py, float pz, int32_t H)
{
	float clip[4];
	rd_clip_position(g, pv, q, qw, scale, px, py, pz, clip);
	return rd_snap(g, clip, H);
}

// ---- near-plane clipping (NV_OPT_RASTER_NEAR_CLIP, DESIGN.md §4.10 "Near-plane clipping")
constexpr int32_t RD_OUTSIDE = 2; // bit 1 of a snapped vertex's .w: the vertex fails clip.w > 0 && clip.z <= clip.w (then bit 0 is set as well)

// rd_vertex for the clipping kernels: .w also carries RD_OUTSIDE, and `cv` receives what a crossing edge needs: clip x, y, w and
// d = clip.w - clip.z, with NaN in place of d when one of the four clip components is not finite (d is NaN by itself only then).
NV_DEV int4 rd_vertex_clip(const NvGlobals& g, uint2 pv, f3 q, float qw, float scale, float px, float py, float pz, int32_t H, float4& cv)
{
	float clip[4];
	rd_clip_position(g, pv, q, qw, scale, px, py, pz, clip);
	int4 s = rd_snap(g, clip, H);
	const bool inside = clip[3] > 0.0f && clip[2] <= clip[3];
	const bool finite = __builtin_fabsf(clip[0]) < __builtin_inff() && __builtin_fabsf(clip[1]) < __builtin_inff() &&
	                    __builtin_fabsf(clip[2]) < __builtin_inff() && __builtin_fabsf(clip[3]) < __builtin_inff();
	s.w |= inside ? 0 : RD_OUTSIDE;
	cv = make_float4(clip[0], clip[1], clip[3], finite ? clip[3] - clip[2] : __builtin_nanf(""));
	return s;
}

// c ? a : b per component: a conditional between two vector lvalues selects an address, and what it points to then lives in scratch memory
NV_DEV int4 rd_sel(bool c, int4 a, int4 b) { return make_int4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w); }
NV_DEV float4 rd_sel(bool c, float4 a, float4 b) { return make_float4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w); }

// The vertex where the edge from the inside end `i` to the outside end `o` meets the near plane, snapped: always computed from the inside
// end, so both triangles that share the edge get the same bits.  Its depth is 1 (it lies on the plane); .w = 1 when it is rejected.
NV_DEV int4 rd_clip_vertex(const NvGlobals& g, float4 i, float4 o, int32_t H)
{
	const float t = i.w / (i.w - o.w);
	const float x = i.x + t * (o.x - i.x), y = i.y + t * (o.y - i.y), w = i.z + t * (o.z - i.z);
	const float sx = ((x / w) * 0.5f + 0.5f) * g.screenWidth;
	const float sy = ((y / w) * 0.5f + 0.5f) * g.screenHeight;
	const bool bad = !(w > 0.0f) || !(__builtin_fabsf(sx) < RD_GUARD) || !(__builtin_fabsf(sy) < RD_GUARD); // (NaN and infinity included)
	const int32_t X = bad ? 0 : (int32_t)__builtin_rintf(sx * 256.0f);
	const int32_t Y = bad ? 0 : H * 256 - (int32_t)__builtin_rintf(sy * 256.0f);
	return make_int4(X, Y, __float_as_int(1.0f), bad ? 1 : 0);
}

// The triangle (s0, s1, s2) of rd_vertex_clip's results (c0, c1, c2 their clip records) against the near plane.  Returns the number of
// pieces, 0-2, and the polygon p0..p3 in the triangle's winding: piece 0 is (p0, p1, p2), piece 1 is (p0, p2, p3).  Three inside vertices
// give the triangle itself as piece 0.  The walk is Sutherland-Hodgman's over v0->v1, v1->v2, v2->v0 written out per case, with selects
// instead of indexed arrays (which would live in scratch memory): with r the one outside vertex (or the one inside vertex), R0 = v[r],
// R1 = v[r + 1], R2 = v[r + 2] and N1, N2 the two new vertices, the polygon is a rotation of (N1, R1, R2, N2) (or of (R0, N1, N2)).
NV_DEV uint32_t rd_clip(const NvGlobals& g, int4 s0, int4 s1, int4 s2, float4 c0, float4 c1, float4 c2, int32_t H, int4& p0, int4& p1, int4& p2,
                        int4& p3)
{
	const uint32_t out = (s0.w & RD_OUTSIDE ? 1u : 0u) | (s1.w & RD_OUTSIDE ? 2u : 0u) | (s2.w & RD_OUTSIDE ? 4u : 0u);
	p0 = s0, p1 = s1, p2 = s2, p3 = s2;
	if (out == 0u)
		return 1u;
	if (out == 7u)
		return 0u;
	// all twelve clip components finite, and every outside vertex strictly beyond the plane (a caller's projection may give w <= 0 with z <= w)
	const bool ok = c0.w == c0.w && c1.w == c1.w && c2.w == c2.w && (!(out & 1u) || c0.w < 0.0f) && (!(out & 2u) || c1.w < 0.0f) &&
	                (!(out & 4u) || c2.w < 0.0f);
	if (!ok)
		return 0u;
	const bool one = (out & (out - 1u)) == 0u;          // one vertex outside: a quad; else one vertex inside: a triangle
	const uint32_t sel = one ? out : out ^ 7u;          // the bit of vertex r
	const uint32_t r = sel == 1u ? 0u : (sel == 2u ? 1u : 2u);
	const bool r0 = r == 0u, r1 = r == 1u;
	const int4 S0 = rd_sel(r0, s0, rd_sel(r1, s1, s2)), S1 = rd_sel(r0, s1, rd_sel(r1, s2, s0)), S2 = rd_sel(r0, s2, rd_sel(r1, s0, s1));
	const float4 C0 = rd_sel(r0, c0, rd_sel(r1, c1, c2)), C1 = rd_sel(r0, c1, rd_sel(r1, c2, c0)), C2 = rd_sel(r0, c2, rd_sel(r1, c0, c1));
	// one outside (R0): N1 on R1 -> R0, N2 on R2 -> R0.  One inside (R0): N1 on R0 -> R1, N2 on R0 -> R2.
	const int4 N1 = rd_clip_vertex(g, rd_sel(one, C1, C0), rd_sel(one, C0, C1), H);
	const int4 N2 = rd_clip_vertex(g, rd_sel(one, C2, C0), rd_sel(one, C0, C2), H);
	if ((N1.w | N2.w) != 0) // a rejected new vertex rejects the whole triangle, never one piece alone
		return 0u;
	const int4 I0 = make_int4(S0.x, S0.y, S0.z, S0.w & 1), I1 = make_int4(S1.x, S1.y, S1.z, S1.w & 1), I2 = make_int4(S2.x, S2.y, S2.z, S2.w & 1);
	if (one)
	{
		// (N1, R1, R2, N2) from the walk's first emitted vertex: r = 0 starts at N1, r = 1 at R2 (= v0), r = 2 at R1 (= v0)
		p0 = rd_sel(r0, N1, rd_sel(r1, I2, I1));
		p1 = rd_sel(r0, I1, rd_sel(r1, N2, I2));
		p2 = rd_sel(r0, I2, rd_sel(r1, N1, N2));
		p3 = rd_sel(r0, N2, rd_sel(r1, I1, N1));
		return 2u;
	}
	// (R0, N1, N2): r = 0 starts at R0 (= v0), r = 1 and r = 2 at N2 (the crossing of the first edge that has one)
	p0 = rd_sel(r0, I0, N2);
	p1 = rd_sel(r0, N1, I0);
	p2 = rd_sel(r0, N2, N1);
	p3 = p2;
	return 1u;
}

NV_DEV int64_t rd_edge(int32_t px, int32_t py, int32_t qx, int32_t qy, int32_t sx, int32_t sy)
{
	// every difference is below 2^30 in magnitude (guard band, viewport <= 16384): 32 x 32 -> 64-bit products
	return (int64_t)(qx - px) * (int64_t)(sy - py) - (int64_t)(qy - py) * (int64_t)(sx - px);
}

NV_DEV bool rd_top_left(int32_t px, int32_t py, int32_t qx, int32_t qy)
{
	const int32_t dx = qx - px, dy = qy - py;
	return dy < 0 || (dy == 0 && dx > 0);
}

NV_DEV int32_t rd_floor256(int32_t v) { return v >> 8; } // arithmetic shift: floor(v / 256)

// Setup of the triangle with snapped corners (a, b, c) as rd_vertex returns them.  Returns false when it is not drawn (a rejected corner,
// zero area, or a back face with back-face culling on); `tri` then is left undefined.
NV_DEV bool rd_setup_corners(int4 a, int4 b, int4 c, bool bothFaces, int32_t W, int32_t H, RdTri& tri)
{
	if ((a.w | b.w | c.w) != 0)
		return false;
	int64_t A = (int64_t)(b.x - a.x) * (int64_t)(c.y - a.y) - (int64_t)(b.y - a.y) * (int64_t)(c.x - a.x);
	if (A == 0 || (A > 0 && !bothFaces))
		return false;
	if (A < 0) // front face (counter-clockwise in y-up space): wind it so that A > 0
	{
		const int4 s = b;
		b = c, c = s, A = -A;
	}
	tri.ax = a.x, tri.ay = a.y, tri.bx = b.x, tri.by = b.y, tri.cx = c.x, tri.cy = c.y;
	const float za = __int_as_float(a.z), zb = __int_as_float(b.z), zc = __int_as_float(c.z);
	tri.za = za, tri.dzb = zb - za, tri.dzc = zc - za;
	tri.inv = 1.0f / (float)A;
	tri.topLeft = (rd_top_left(a.x, a.y, b.x, b.y) ? 1u : 0u) | (rd_top_left(b.x, b.y, c.x, c.y) ? 2u : 0u) | (rd_top_left(c.x, c.y, a.x, a.y) ? 4u : 0u);
	const int32_t xmin = min(min(a.x, b.x), c.x), xmax = max(max(a.x, b.x), c.x);
	const int32_t ymin = min(min(a.y, b.y), c.y), ymax = max(max(a.y, b.y), c.y);
	// pixel centres x * 256 + 128 inside [xmin, xmax]; |X|, |Y| < 2^29 + 2^22: no overflow
	tri.x0 = max(rd_floor256(xmin - 128 + 255), 0), tri.x1 = min(rd_floor256(xmax - 128), W - 1);
	tri.y0 = max(rd_floor256(ymin - 128 + 255), 0), tri.y1 = min(rd_floor256(ymax - 128), H - 1);
	return true;
}

// Setup of triangle (ia, ib, ic) from a meshlet's snapped vertices: as rd_setup_corners, and false for an index at or past the vertex count.
NV_DEV bool rd_setup(const int4* vtx, uint32_t ia, uint32_t ib, uint32_t ic, uint32_t ve, bool bothFaces, int32_t W, int32_t H, RdTri& tri)
{
	if (ia >= ve || ib >= ve || ic >= ve)
		return false;
	return rd_setup_corners(vtx[ia], vtx[ib], vtx[ic], bothFaces, W, H, tri);
}

// The stable form of the visibility word (NV_OPT_RASTER_VISIBILITY_ID 1): bits(z) << 34 | id34, id34 = ((mvi << 7) | triangle) + 1.  rd_sample clamps
// z to [0, 1] with NaN -> 0, so bits(z) <= 0x3F800000 < 2^30 and the shift loses nothing; mvi < RD_STABLE_MVI_END keeps id34 below 2^34.
constexpr uint32_t RD_STABLE_SHIFT = 34;
constexpr uint32_t RD_STABLE_MVI_END = (1u << 27) - 1u;

// One pixel centre, first half: coverage by the edge functions and the top-left rule; wb, wc: the edge values the depth is interpolated with
NV_DEV bool rd_covered(const RdTri& t, int32_t px, int32_t py, int64_t& wb, int64_t& wc)
{
	const int32_t sx = px * 256 + 128, sy = py * 256 + 128;
	const int64_t wa = rd_edge(t.bx, t.by, t.cx, t.cy, sx, sy);
	wb = rd_edge(t.cx, t.cy, t.ax, t.ay, sx, sy);
	wc = rd_edge(t.ax, t.ay, t.bx, t.by, sx, sy);
	return (wa > 0 || (wa == 0 && (t.topLeft & 2u))) && (wb > 0 || (wb == 0 && (t.topLeft & 4u))) && (wc > 0 || (wc == 0 && (t.topLeft & 1u)));
}

// One pixel centre, second half: the depth of a covered sample and the atomics (vis: optional).  STABLE = false: the word is
// bits(z) << 32 | id (ID = uint32_t, slot << 7 | triangle); STABLE = true: bits(z) << 34 | id (ID = 64 bits, id34).
template <bool STABLE = false, class ID = uint32_t>
NV_DEV void rd_write(const RdTri& t, int64_t wb, int64_t wc, int32_t px, int32_t py, uint32_t W, uint32_t* __restrict__ depth, unsigned long long* __restrict__ vis,
                     ID id)
{
	float z = (t.za + ((float)wb * t.inv) * t.dzb) + ((float)wc * t.inv) * t.dzc;
	z = z > 0.0f ? z : 0.0f; // (NaN -> 0)
	z = z < 1.0f ? z : 1.0f;
	const uint32_t bits = __float_as_uint(z);
	const size_t at = (size_t)py * W + (size_t)px;
	if (bits > depth[at])
		atomicMax(depth + at, bits);
	if (vis)
	{
		const unsigned long long v = (unsigned long long)bits << (STABLE ? RD_STABLE_SHIFT : 32u) | id;
		if (v > vis[at])
			atomicMax(vis + at, v);
	}
}

// One pixel centre: rd_covered, then rd_write.  Returns whether the sample is covered.
template <bool STABLE = false, class ID = uint32_t>
NV_DEV bool rd_sample(const RdTri& t, int32_t px, int32_t py, uint32_t W, uint32_t* __restrict__ depth, unsigned long long* __restrict__ vis, ID id)
{
	int64_t wb, wc;
	if (!rd_covered(t, px, py, wb, wc))
		return false;
	rd_write<STABLE>(t, wb, wc, px, py, W, depth, vis, id);
	return true;
}

} // namespace nv
