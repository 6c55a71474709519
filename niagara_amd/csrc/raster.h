// raster.h — the raster rules both depth rasterisers share: the vertex stage to snapped screen space, the triangle
// setup (rejection, facing, top-left flags, pixel box) and the per-sample coverage / depth / atomic.  rasterdepth.hip (the cluster path) and
// rasterindexed.hip (the indexed-draw path) use these statements and nothing else for what they write, so the same triangle under the same
// draw writes the same bits through either path; tests/raster_ref.c restates them one sample at a time.
#pragma once

#include "cullmath.h"
#include "args.h"

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

// One vertex (the first 8 bytes of its record: fp16 x, y, z) under the draw {position, scale, orientation q.xyz, qw} to snapped screen
// space: X, Y with 8 sub-pixel bits (row 0 at the top), the bits of z = clip.z / clip.w, and 1 in .w when no triangle of it is drawn.
// nv_trianglecull's arithmetic (src/shaders/meshlet.mesh.glsl:121-160; mesh.vert.glsl:41-57 computes the same).
NV_DEV int4 rd_vertex(const NvGlobals& g, uint2 pv, f3 q, float qw, float scale, float px, float py, float pz, int32_t H)
{
	const f3 position = { half_bits_to_float(pv.x & 0xffffu), half_bits_to_float(pv.x >> 16), half_bits_to_float(pv.y & 0xffffu) };
	const f3 rot = rotate_quat(position, q, qw);
	const float wx = rot.x * scale + px, wy = rot.y * scale + py, wz = rot.z * scale + pz;
	const float* V = g.cullData.view;
	const float* P = g.projection;
	float v4[4], clip[4];
#pragma unroll
	for (int r = 0; r < 4; ++r) // view * vec4(wpos, 1): c3 * 1.0f is c3 exactly
		v4[r] = ((V[r] * wx + V[4 + r] * wy) + V[8 + r] * wz) + V[12 + r];
#pragma unroll
	for (int r = 0; r < 4; ++r)
		clip[r] = ((P[r] * v4[0] + P[4 + r] * v4[1]) + P[8 + r] * v4[2]) + P[12 + r] * v4[3];
	const float sx = ((clip[0] / clip[3]) * 0.5f + 0.5f) * g.screenWidth;
	const float sy = ((clip[1] / clip[3]) * 0.5f + 0.5f) * g.screenHeight;
	const float z = clip[2] / clip[3];
	// behind or in front of the near plane (NaN included), non-finite, or outside the guard band: no triangle of it is drawn
	const bool bad = !(clip[3] > 0.0f && clip[2] <= clip[3]) || !(__builtin_fabsf(sx) < RD_GUARD) || !(__builtin_fabsf(sy) < RD_GUARD);
	const int32_t X = bad ? 0 : (int32_t)__builtin_rintf(sx * 256.0f);
	const int32_t Y = bad ? 0 : H * 256 - (int32_t)__builtin_rintf(sy * 256.0f); // viewport flipped: row 0 at the top
	return make_int4(X, Y, __float_as_int(z), bad ? 1 : 0);
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

// One pixel centre: coverage, depth, and the atomics (vis: optional).  Returns whether the sample is covered.
NV_DEV bool rd_sample(const RdTri& t, int32_t px, int32_t py, uint32_t W, uint32_t* __restrict__ depth, unsigned long long* __restrict__ vis, uint32_t id)
{
	const int32_t sx = px * 256 + 128, sy = py * 256 + 128;
	const int64_t wa = rd_edge(t.bx, t.by, t.cx, t.cy, sx, sy);
	const int64_t wb = rd_edge(t.cx, t.cy, t.ax, t.ay, sx, sy);
	const int64_t wc = rd_edge(t.ax, t.ay, t.bx, t.by, sx, sy);
	const bool covered = (wa > 0 || (wa == 0 && (t.topLeft & 2u))) && (wb > 0 || (wb == 0 && (t.topLeft & 4u))) && (wc > 0 || (wc == 0 && (t.topLeft & 1u)));
	if (!covered)
		return false;
	float z = (t.za + ((float)wb * t.inv) * t.dzb) + ((float)wc * t.inv) * t.dzc;
	z = z > 0.0f ? z : 0.0f; // (NaN -> 0)
	z = z < 1.0f ? z : 1.0f;
	const uint32_t bits = __float_as_uint(z);
	const size_t at = (size_t)py * W + (size_t)px;
	if (bits > depth[at])
		atomicMax(depth + at, bits);
	if (vis)
	{
		const unsigned long long v = (unsigned long long)bits << 32 | id;
		if (v > vis[at])
			atomicMax(vis + at, v);
	}
	return true;
}

// adds the per-workgroup partial sums of a launch (4 x u64 per workgroup) to the caller's four totals (one workgroup; rasterdepth.hip)
int launch_raster_totals(hipStream_t stream, const unsigned long long* partials, uint32_t blocks, unsigned long long* totals);

} // namespace nv
