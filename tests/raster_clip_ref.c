/* raster_clip_ref.c — CPU reference of nv_rasterdepth and nv_rasterdepth_indexed with NV_OPT_RASTER_NEAR_CLIP (include/niagara_vis.h).
 *
 * Test infrastructure: compiled by tests/raster_clip_ref.py with raster_ref.c's flags.  It includes tests/raster_indexed_ref.c (which includes
 * tests/raster_ref.c), so the vertex stage, the snap, the edge functions and the coverage rule are the same statements as the unclipped
 * references; what it adds is the near-plane rule of DESIGN.md §4.10 ("Near-plane clipping"), written from that text one triangle at a time:
 * a plain Sutherland-Hodgman walk over arrays, not the kernels' case table.  With nearClip = 0 it is the unclipped rule. */
#include "raster_indexed_ref.c"

typedef struct
{
	Vtx s;          /* the vertex as the unclipped rule sees it */
	float x, y, w;  /* clip x, y, w */
	float d;        /* clip.w - clip.z */
	int inside;     /* clip.w > 0 && clip.z <= clip.w */
	int finite;     /* all four clip components finite */
} CVtx;

/* stats4 (optional), per triangle with both inside and outside vertices: [0] how many, [1] clipped into a polygon, [2] refused for a
 * non-finite component or an outside vertex with d >= 0, [3] refused for a rejected new vertex */
enum
{
	ST_CROSSING,
	ST_CLIPPED,
	ST_REFUSED_RULE,
	ST_REFUSED_VERTEX
};

/* vertex_stage's clip-space position (the same arithmetic, kept next to it so that a reader can compare them) */
static void clip_position(const Globals* g, const Draw* d, const Vertex* v, float clip[4])
{
	const float* P = g->projection;
	const float* V = g->view;
	float position[3] = { f16(v->vx), f16(v->vy), f16(v->vz) };
	float rot[3], wpos[3], v4[4];
	rotate_quat(position, d->orientation, rot);
	for (int k = 0; k < 3; ++k)
		wpos[k] = rot[k] * d->scale + d->position[k];
	for (int r = 0; r < 4; ++r)
		v4[r] = ((V[r] * wpos[0] + V[4 + r] * wpos[1]) + V[8 + r] * wpos[2]) + V[12 + r] * 1.0f;
	for (int r = 0; r < 4; ++r)
		clip[r] = ((P[r] * v4[0] + P[4 + r] * v4[1]) + P[8 + r] * v4[2]) + P[12 + r] * v4[3];
}

static CVtx clip_vertex(const Globals* g, const Draw* d, const Vertex* v, uint32_t H)
{
	CVtx o;
	float r[4], clip[4];
	int inFront = vertex_stage(g, d, v, r);
	o.s = snap(r, inFront, H);
	clip_position(g, d, v, clip);
	o.x = clip[0], o.y = clip[1], o.w = clip[3];
	o.d = clip[3] - clip[2];
	o.inside = clip[3] > 0.0f && clip[2] <= clip[3];
	o.finite = isfinite(clip[0]) && isfinite(clip[1]) && isfinite(clip[2]) && isfinite(clip[3]);
	return o;
}

/* the vertex where the edge between the inside end I and the outside end O meets the near plane, always from I towards O; 0 when rejected */
static int new_vertex(const Globals* g, const CVtx* I, const CVtx* O, uint32_t H, Vtx* out)
{
	float t = I->d / (I->d - O->d);
	float x = I->x + t * (O->x - I->x);
	float y = I->y + t * (O->y - I->y);
	float w = I->w + t * (O->w - I->w);
	float sx = ((x / w) * 0.5f + 0.5f) * g->screenWidth;
	float sy = ((y / w) * 0.5f + 0.5f) * g->screenHeight;
	if (!(w > 0.0f) || !isfinite(sx) || !isfinite(sy) || !(fabsf(sx) < GUARD) || !(fabsf(sy) < GUARD))
		return 0;
	out->X = (int32_t)rintf(sx * 256.0f);
	out->Y = (int32_t)(H * 256u) - (int32_t)rintf(sy * 256.0f);
	out->z = 1.0f; /* on the near plane */
	out->bad = 0;
	return 1;
}

/* the polygon of triangle v[0..2]: 0 (not drawn), 3 or 4 vertices in the triangle's winding */
static int clip_polygon(const Globals* g, const CVtx v[3], int nearClip, uint32_t H, Vtx poly[4], uint64_t* stats4)
{
	int outside = !v[0].inside + !v[1].inside + !v[2].inside;
	if (outside == 0 || !nearClip) /* as without the option: a vertex that is not inside is `bad` and rejects the triangle */
	{
		poly[0] = v[0].s, poly[1] = v[1].s, poly[2] = v[2].s;
		return 3;
	}
	if (outside == 3)
		return 0;
	if (stats4)
		stats4[ST_CROSSING] += 1;
	for (int k = 0; k < 3; ++k)
		if (!v[k].finite || (!v[k].inside && !(v[k].d < 0.0f)))
		{
			if (stats4)
				stats4[ST_REFUSED_RULE] += 1;
			return 0;
		}
	int n = 0;
	for (int k = 0; k < 3; ++k)
	{
		const CVtx *a = &v[k], *b = &v[(k + 1) % 3];
		if (a->inside)
			poly[n++] = a->s;
		if (a->inside != b->inside && !new_vertex(g, a->inside ? a : b, a->inside ? b : a, H, &poly[n++]))
		{
			if (stats4)
				stats4[ST_REFUSED_VERTEX] += 1;
			return 0;
		}
	}
	if (stats4)
		stats4[ST_CLIPPED] += 1;
	return n;
}

/* one piece: rr_rasterdepth's rules for a triangle of snapped corners (rejection, facing from its own area, top-left, box, depth), with the
 * visibility word of the original triangle */
static void draw_piece(const Vtx* a, const Vtx* b, const Vtx* c, int bothFaces, uint32_t W, uint32_t H, uint32_t* depth, uint64_t* visibility,
                       uint64_t id, uint64_t* totals4)
{
	if (a->bad || b->bad || c->bad)
		return;
	int64_t A = (int64_t)(b->X - a->X) * (c->Y - a->Y) - (int64_t)(b->Y - a->Y) * (c->X - a->X);
	if (A == 0 || (A > 0 && !bothFaces))
		return;
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
				uint64_t word = (uint64_t)bits << 32 | id;
				if (word > visibility[at])
					visibility[at] = word;
			}
		}
	}
}

/* one triangle: its polygon, then the fan (p0, p1, p2), (p0, p2, p3) */
static void draw_triangle(const Globals* g, const CVtx v[3], int nearClip, int bothFaces, uint32_t W, uint32_t H, uint32_t* depth,
                          uint64_t* visibility, uint64_t id, uint64_t* totals4, uint64_t* stats4)
{
	Vtx poly[4];
	int n = clip_polygon(g, v, nearClip, H, poly, stats4);
	if (n >= 3)
		draw_piece(&poly[0], &poly[1], &poly[2], bothFaces, W, H, depth, visibility, id, totals4);
	if (n == 4)
		draw_piece(&poly[0], &poly[2], &poly[3], bothFaces, W, H, depth, visibility, id, totals4);
}

/* nv_rasterdepth on the CPU with NV_OPT_RASTER_NEAR_CLIP = nearClip.  Arguments as rr_rasterdepth; stats4: optional (see above). */
void rc_rasterdepth(const Globals* g, const Command* commands, const Draw* draws, const Meshlet* meshlets, const uint32_t* data,
                    const Vertex* vertices, const uint32_t* cib, const uint32_t* cc4, uint32_t* depth, uint32_t W, uint32_t H, uint64_t* visibility,
                    uint64_t* totals4, int nearClip, uint64_t* stats4)
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
				CVtx vs[MAXVTX];
				for (uint32_t i = 0; i < ve; ++i)
					vs[i] = clip_vertex(g, &draws[drawId], &vertices[vertex_ref(data, m, i)], H);
				totals4[0] += 1;
				totals4[1] += m->triangleCount;
				for (uint32_t t = 0; t < te; ++t)
				{
					uint32_t o = indexOffset * 4 + t * 3;
					uint32_t ia = d8[o], ib = d8[o + 1], ic = d8[o + 2];
					if (ia >= ve || ib >= ve || ic >= ve)
						continue;
					CVtx v[3] = { vs[ia], vs[ib], vs[ic] };
					draw_triangle(g, v, nearClip, bothFaces, W, H, depth, visibility, (uint64_t)index << 7 | t, totals4, stats4);
				}
			}
}

/* nv_rasterdepth_indexed on the CPU with NV_OPT_RASTER_NEAR_CLIP = nearClip.  Arguments as rr_rasterdepth_indexed. */
void rc_rasterdepth_indexed(const Globals* g, const DrawCommand* commands, const uint32_t* count, const Draw* draws, uint32_t drawCount,
                            const uint32_t* indices, uint32_t indexCapacity, const Vertex* vertices, uint32_t vertexCapacity, uint32_t* depth,
                            uint32_t W, uint32_t H, uint64_t* totals4, int nearClip, uint64_t* stats4)
{
	const int bothFaces = g->postPass != 0;
	uint32_t n = count[0] < drawCount ? count[0] : drawCount;
	for (uint32_t i = 0; i < n; ++i)
	{
		const DrawCommand* c = &commands[i];
		if (c->instanceCount == 0 || c->drawId >= drawCount)
			continue;
		totals4[0] += 1;
		totals4[1] += c->indexCount / 3;
		for (uint32_t t = 0; t < c->indexCount / 3; ++t)
		{
			uint64_t at = (uint64_t)c->firstIndex + 3u * (uint64_t)t;
			if (at + 2 >= indexCapacity)
				break;
			uint32_t id[3];
			int skip = 0;
			for (int k = 0; k < 3; ++k)
			{
				id[k] = indices[at + k] + c->vertexOffset;
				skip |= id[k] >= vertexCapacity;
			}
			if (skip)
				continue;
			CVtx v[3];
			for (int k = 0; k < 3; ++k)
				v[k] = clip_vertex(g, &draws[c->drawId], &vertices[id[k]], H);
			draw_triangle(g, v, nearClip, bothFaces, W, H, depth, 0, 0, totals4, stats4);
		}
	}
}
