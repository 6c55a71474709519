/* raster_indexed_ref.c — CPU reference of nv_rasterdepth_indexed (include/niagara_vis.h): the depth raster of the indexed draws of niagara's
 * classic path (vkCmdDrawIndexedIndirectCount through mesh.vert.glsl, src/niagara.cpp:1680-1694).
 *
 * Test infrastructure: compiled by tests/raster_indexed_ref.py with raster_ref.c's flags.  It includes tests/raster_ref.c, so the vertex stage,
 * the snap, the edge functions and the coverage rule are the same statements as the cluster path's reference; what it adds is how a draw
 * command names its triangles and the skip rules of DESIGN.md §4.11, one triangle at a time. */
#include "raster_ref.c"

typedef struct
{
	uint32_t drawId, indexCount, instanceCount, firstIndex, vertexOffset, firstInstance;
} DrawCommand;

/* one triangle of snapped corners: rr_rasterdepth's rules (rejection, facing, top-left, box, depth) without a visibility word */
static void raster_triangle(const Vtx* a, const Vtx* b, const Vtx* c, int bothFaces, uint32_t W, uint32_t H, uint32_t* depth, uint64_t* totals4)
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
		}
	}
}

/* nv_rasterdepth_indexed on the CPU.  depth: width x height fp32 bits (row 0 = top), totals4: accumulated. */
void rr_rasterdepth_indexed(const Globals* g, const DrawCommand* commands, const uint32_t* count, const Draw* draws, uint32_t drawCount,
                            const uint32_t* indices, uint32_t indexCapacity, const Vertex* vertices, uint32_t vertexCapacity, uint32_t* depth,
                            uint32_t W, uint32_t H, uint64_t* totals4)
{
	const int bothFaces = g->postPass != 0;
	uint32_t n = count[0] < drawCount ? count[0] : drawCount;
	for (uint32_t i = 0; i < n; ++i)
	{
		const DrawCommand* c = &commands[i];
		if (c->instanceCount == 0 || c->drawId >= drawCount) /* instanceCount > 1 draws the same depth again */
			continue;
		totals4[0] += 1;
		totals4[1] += c->indexCount / 3;
		for (uint32_t t = 0; t < c->indexCount / 3; ++t)
		{
			uint64_t at = (uint64_t)c->firstIndex + 3u * (uint64_t)t;
			if (at + 2 >= indexCapacity) /* an index position at or past the buffer's end: this triangle and every later one */
				break;
			uint32_t v[3];
			int skip = 0;
			for (int k = 0; k < 3; ++k)
			{
				v[k] = indices[at + k] + c->vertexOffset; /* mod 2^32 */
				skip |= v[k] >= vertexCapacity;       /* 0xFFFFFFFF included: no primitive restart */
			}
			if (skip)
				continue;
			Vtx vs[3];
			for (int k = 0; k < 3; ++k)
			{
				float r[4];
				int inFront = vertex_stage(g, &draws[c->drawId], &vertices[v[k]], r);
				vs[k] = snap(r, inFront, H);
			}
			raster_triangle(&vs[0], &vs[1], &vs[2], bothFaces, W, H, depth, totals4);
		}
	}
}
