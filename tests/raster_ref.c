/* raster_ref.c — CPU reference of nv_rasterdepth (include/niagara_vis.h), the depth-only rasteriser of the visible clusters.
 *
 * Test infrastructure: compiled by tests/raster_ref.py with the oracle's floating-point flags (-O2 -ffp-contract=off -fno-fast-math
 * -msse2 -mfpmath=sse) and loaded through ctypes.  It restates the rule set of DESIGN.md §4.10 one sample at a time, in the order a
 * reader checks it against the text; the HIP kernel must equal it bit for bit.  The vertex stage is orc_trianglecull's arithmetic
 * (oracle/oracle.c), restated here so that the test of the two can compare them. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define MAXVTX 64u
#define MAXTRI 96u
#define CLUSTER_TILE 16u
#define GUARD 2097152.0f /* 2^21 pixels */

typedef struct
{
	uint16_t center[4];
	int8_t cone[4];
	uint32_t dataOffset, baseVertex;
	uint8_t vertexCount, triangleCount, shortRefs, padding;
} Meshlet;
typedef struct
{
	float position[3], scale, orientation[4];
	uint32_t meshIndex, meshletVisibilityOffset, postPass, materialIndex;
} Draw;
typedef struct
{
	uint32_t drawId, taskOffset, taskCount, lateDrawVisibility, meshletVisibilityOffset;
} Command;
typedef struct
{
	uint16_t vx, vy, vz, tp;
	uint32_t np;
	uint16_t tu, tv;
} Vertex;
typedef struct
{
	float projection[16];
	float view[16];
	float P00, P11, znear, zfar, frustum[4], lodTarget, pyramidWidth, pyramidHeight;
	uint32_t drawCount;
	int32_t cullingEnabled, lodEnabled, occlusionEnabled, clusterOcclusionEnabled, clusterBackfaceEnabled;
	uint32_t postPass, pad_[2];
	float screenWidth, screenHeight, pad2_[2];
} Globals;

typedef struct
{
	int32_t X, Y; /* snapped, 8 sub-pixel bits, row 0 at the top */
	float z;      /* clip.z / clip.w */
	int bad;      /* behind / in front of the near plane, non-finite or outside the guard band */
} Vtx;

static float f16(uint16_t h)
{
	uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu, u;
	float f;
	if (e == 0)
	{
		if (m == 0)
		{
			memcpy(&f, &sign, 4);
			return f;
		}
		f = (float)m * 5.9604644775390625e-8f; /* 2^-24, exact */
		return sign ? -f : f;
	}
	u = e == 31 ? sign | 0x7f800000u | (m << 13) : sign | ((e + 112u) << 23) | (m << 13);
	memcpy(&f, &u, 4);
	return f;
}

static uint32_t fbits(float f)
{
	uint32_t u;
	memcpy(&u, &f, 4);
	return u;
}

/* orc_rotate_quat: v + 2 cross(q.xyz, cross(q.xyz, v) + q.w v) */
static void rotate_quat(const float v[3], const float q[4], float out[3])
{
	float t[3], u[3];
	t[0] = q[1] * v[2] - v[1] * q[2];
	t[1] = q[2] * v[0] - v[2] * q[0];
	t[2] = q[0] * v[1] - v[0] * q[1];
	t[0] = t[0] + q[3] * v[0];
	t[1] = t[1] + q[3] * v[1];
	t[2] = t[2] + q[3] * v[2];
	u[0] = q[1] * t[2] - t[1] * q[2];
	u[1] = q[2] * t[0] - t[2] * q[0];
	u[2] = q[0] * t[1] - t[0] * q[1];
	out[0] = v[0] + 2.0f * u[0];
	out[1] = v[1] + 2.0f * u[1];
	out[2] = v[2] + 2.0f * u[2];
}

/* one vertex: screen x, y, clip w and z = clip.z / clip.w (orc_trianglecull's arithmetic, src/shaders/meshlet.mesh.glsl:121-160);
 * returns whether the vertex is inside the near half-space: clip.w > 0 && clip.z <= clip.w (NaN: no) */
static int vertex_stage(const Globals* g, const Draw* d, const Vertex* v, float out[4])
{
	const float* P = g->projection;
	const float* V = g->view;
	float position[3] = { f16(v->vx), f16(v->vy), f16(v->vz) };
	float rot[3], wpos[3], v4[4], clip[4];
	rotate_quat(position, d->orientation, rot);
	for (int k = 0; k < 3; ++k)
		wpos[k] = rot[k] * d->scale + d->position[k];
	for (int r = 0; r < 4; ++r)
		v4[r] = ((V[r] * wpos[0] + V[4 + r] * wpos[1]) + V[8 + r] * wpos[2]) + V[12 + r] * 1.0f;
	for (int r = 0; r < 4; ++r)
		clip[r] = ((P[r] * v4[0] + P[4 + r] * v4[1]) + P[8 + r] * v4[2]) + P[12 + r] * v4[3];
	out[0] = ((clip[0] / clip[3]) * 0.5f + 0.5f) * g->screenWidth;
	out[1] = ((clip[1] / clip[3]) * 0.5f + 0.5f) * g->screenHeight;
	out[2] = clip[3];
	out[3] = clip[2] / clip[3];
	return clip[3] > 0.0f && clip[2] <= clip[3];
}

static Vtx snap(const float r[4], int inFront, uint32_t H)
{
	Vtx o;
	float sx = r[0], sy = r[1];
	o.z = r[3];
	o.bad = !inFront || !isfinite(sx) || !isfinite(sy) || !(fabsf(sx) < GUARD) || !(fabsf(sy) < GUARD);
	o.X = o.bad ? 0 : (int32_t)rintf(sx * 256.0f);
	o.Y = o.bad ? 0 : (int32_t)(H * 256u) - (int32_t)rintf(sy * 256.0f);
	return o;
}

/* floor(v / 256) */
static int64_t fdiv256(int64_t v) { return v >= 0 ? v / 256 : -((-v + 255) / 256); }

static int64_t edge(const Vtx* p, const Vtx* q, int64_t sx, int64_t sy)
{
	return (int64_t)(q->X - p->X) * (sy - p->Y) - (int64_t)(q->Y - p->Y) * (sx - p->X);
}

static int top_left(const Vtx* p, const Vtx* q)
{
	int32_t dx = q->X - p->X, dy = q->Y - p->Y;
	return dy < 0 || (dy == 0 && dx > 0);
}

static int covers(int64_t e, int tl) { return e > 0 || (e == 0 && tl); }

/* the slot's meshlet, or 0 for a padding entry */
static const Meshlet* slot_meshlet(const Command* commands, const Meshlet* meshlets, uint32_t ci, uint32_t* drawId)
{
	if (ci == ~0u)
		return 0;
	const Command* c = &commands[ci & 0xffffffu];
	*drawId = c->drawId;
	return &meshlets[c->taskOffset + (ci >> 24)];
}

static uint32_t vertex_ref(const uint32_t* data, const Meshlet* m, uint32_t i)
{
	const uint16_t* d16 = (const uint16_t*)data;
	return m->shortRefs == 1 ? (uint32_t)d16[m->dataOffset * 2 + i] + m->baseVertex : data[m->dataOffset + i] + m->baseVertex;
}

/* Per slot of the grid and vertex i < 64: {sx, sy, clip w, z}, zero past min(vertexCount, 64) and for padding slots (the test compares
 * the first three with orc_trianglecull's decisions) */
void rr_vertices(const Globals* g, const Command* commands, const Draw* draws, const Meshlet* meshlets, const uint32_t* data, const Vertex* vertices,
                 const uint32_t* cib, const uint32_t* cc4, float* out4, uint32_t capacity)
{
	for (uint32_t y = 0; y < cc4[2]; ++y)
		for (uint32_t z = 0; z < cc4[3]; ++z)
			for (uint32_t x = 0; x < cc4[1]; ++x)
			{
				uint32_t index = x + y * 256 + z * CLUSTER_TILE, drawId = 0;
				if (index >= capacity)
					continue;
				float* o = out4 + (size_t)index * MAXVTX * 4;
				memset(o, 0, MAXVTX * 4 * sizeof(float));
				const Meshlet* m = slot_meshlet(commands, meshlets, cib[index], &drawId);
				if (!m)
					continue;
				uint32_t ve = m->vertexCount < MAXVTX ? m->vertexCount : MAXVTX;
				for (uint32_t i = 0; i < ve; ++i)
				{
					float r[4];
					vertex_stage(g, &draws[drawId], &vertices[vertex_ref(data, m, i)], r);
					o[i * 4 + 0] = r[0];
					o[i * 4 + 1] = r[1];
					o[i * 4 + 2] = r[2];
					o[i * 4 + 3] = r[3];
				}
			}
}

/* nv_rasterdepth on the CPU.  depth: width x height fp32 bits (row 0 = top), visibility: optional, totals4: accumulated. */
void rr_rasterdepth(const Globals* g, const Command* commands, const Draw* draws, const Meshlet* meshlets, const uint32_t* data,
                    const Vertex* vertices, const uint32_t* cib, const uint32_t* cc4, uint32_t* depth, uint32_t W, uint32_t H, uint64_t* visibility,
                    uint64_t* totals4)
{
	const uint8_t* d8 = (const uint8_t*)data;
	const int bothFaces = g->postPass != 0;
	for (uint32_t y = 0; y < cc4[2]; ++y)
		for (uint32_t z = 0; z < cc4[3]; ++z)
			for (uint32_t x = 0; x < cc4[1]; ++x)
			{
				uint32_t index = x + y * 256 + z * CLUSTER_TILE, drawId = 0;
				const Meshlet* m = slot_meshlet(commands, meshlets, cib[index], &drawId);
				if (!m)
					continue;
				uint32_t ve = m->vertexCount < MAXVTX ? m->vertexCount : MAXVTX;
				uint32_t te = m->triangleCount < MAXTRI ? m->triangleCount : MAXTRI;
				uint32_t indexOffset = m->dataOffset + (m->shortRefs == 1 ? (m->vertexCount + 1u) / 2u : m->vertexCount);
				Vtx vs[MAXVTX];
				for (uint32_t i = 0; i < ve; ++i)
				{
					float r[4];
					int inFront = vertex_stage(g, &draws[drawId], &vertices[vertex_ref(data, m, i)], r);
					vs[i] = snap(r, inFront, H);
				}
				totals4[0] += 1;
				totals4[1] += m->triangleCount;
				for (uint32_t t = 0; t < te; ++t)
				{
					uint32_t o = indexOffset * 4 + t * 3;
					uint32_t ia = d8[o], ib = d8[o + 1], ic = d8[o + 2];
					if (ia >= ve || ib >= ve || ic >= ve)
						continue;
					const Vtx *a = &vs[ia], *b = &vs[ib], *c = &vs[ic];
					if (a->bad || b->bad || c->bad)
						continue;
					int64_t A = (int64_t)(b->X - a->X) * (c->Y - a->Y) - (int64_t)(b->Y - a->Y) * (c->X - a->X);
					if (A == 0 || (A > 0 && !bothFaces))
						continue;
					if (A < 0)
					{
						const Vtx* s = b;
						b = c, c = s, A = -A;
					}
					totals4[2] += 1;
					int tab = top_left(a, b), tbc = top_left(b, c), tca = top_left(c, a);
					int32_t xmin = a->X < b->X ? a->X : b->X, xmax = a->X > b->X ? a->X : b->X;
					int32_t ymin = a->Y < b->Y ? a->Y : b->Y, ymax = a->Y > b->Y ? a->Y : b->Y;
					xmin = c->X < xmin ? c->X : xmin, xmax = c->X > xmax ? c->X : xmax;
					ymin = c->Y < ymin ? c->Y : ymin, ymax = c->Y > ymax ? c->Y : ymax;
					float inv = 1.0f / (float)A;
					/* the samples (x * 256 + 128, y * 256 + 128) inside the bounding box, clipped to the viewport */
					int64_t px0 = fdiv256((int64_t)xmin - 128 + 255), px1 = fdiv256((int64_t)xmax - 128);
					int64_t py0 = fdiv256((int64_t)ymin - 128 + 255), py1 = fdiv256((int64_t)ymax - 128);
					px0 = px0 > 0 ? px0 : 0, py0 = py0 > 0 ? py0 : 0;
					px1 = px1 < (int64_t)W - 1 ? px1 : (int64_t)W - 1, py1 = py1 < (int64_t)H - 1 ? py1 : (int64_t)H - 1;
					for (int64_t py = py0; py <= py1; ++py)
					{
						int64_t sy = py * 256 + 128;
						for (int64_t px = px0; px <= px1; ++px)
						{
							int64_t sx = px * 256 + 128;
							int64_t wa = edge(b, c, sx, sy), wb = edge(c, a, sx, sy), wc = edge(a, b, sx, sy);
							if (!covers(wa, tbc) || !covers(wb, tca) || !covers(wc, tab))
								continue;
							totals4[3] += 1;
							float zz = (a->z + ((float)wb * inv) * (b->z - a->z)) + ((float)wc * inv) * (c->z - a->z);
							zz = zz > 0.0f ? zz : 0.0f;
							zz = zz < 1.0f ? zz : 1.0f;
							uint32_t bits = fbits(zz);
							size_t at = (size_t)py * W + (size_t)px;
							if (bits > depth[at])
								depth[at] = bits;
							if (visibility)
							{
								uint64_t id = (uint64_t)bits << 32 | (uint64_t)index << 7 | t;
								if (id > visibility[at])
									visibility[at] = id;
							}
						}
					}
				}
			}
}
