/* visbuffer_ref.c — CPU reference of the frame-stable visibility buffer: nv_rasterdepth with
 * NV_OPT_RASTER_VISIBILITY_ID 1, nv_visibility_resolve and nv_visibility_merge (include/niagara_vis.h).
 *
 * Test infrastructure: compiled by tests/visbuffer_ref.py with raster_ref.c's flags.  It includes tests/raster_clip_ref.c (which includes
 * tests/raster_ref.c through raster_indexed_ref.c), so the vertex stage, the snap, the near-plane rule, the edge functions and the coverage
 * rule are the same statements as the other references.  The stable word is NOT obtained by remapping the slot-form output: ties between
 * two samples of equal depth go to the larger id, and the order of the ids differs between the two forms — the sample loop and its
 * maximum are restated here with the stable word. */
#include "raster_clip_ref.c"

#define VB_SHIFT 34
#define VB_MVI_END ((1u << 27) - 1u)

typedef struct
{
	float center[3], radius;
	uint32_t vertexOffset, vertexCount, ommIndexData, ommIndexBase, lodCount, lodRT, padding[2];
	struct
	{
		uint32_t indexOffset, indexCount, meshletOffset, meshletCount;
		float error;
	} lods[8];
} Mesh;

typedef struct
{
	float view[16];
	float P00, P11, znear, zfar, frustum[4], lodTarget, pyramidWidth, pyramidHeight;
	uint32_t drawCount;
	int32_t cullingEnabled, lodEnabled, occlusionEnabled, clusterOcclusionEnabled, clusterBackfaceEnabled;
	uint32_t postPass, pad_[2];
} Cull;

typedef struct
{
	uint32_t drawId, meshletIndex, triangle, depthBits;
} VisRecord;

/* draw_piece (raster_clip_ref.c) with the stable word: vis may be 0 (the cluster cannot be named: depth only) */
static void vb_piece(const Vtx* a, const Vtx* b, const Vtx* c, int bothFaces, uint32_t W, uint32_t H, uint32_t* depth, uint64_t* vis, uint64_t id34,
                     uint64_t* totals4)
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
			zz = zz > 0.0f ? zz : 0.0f; /* NaN -> 0 */
			zz = zz < 1.0f ? zz : 1.0f;
			uint32_t bits = fbits(zz); /* <= 0x3F800000 < 2^30 */
			size_t at = (size_t)py * W + (size_t)px;
			if (bits > depth[at])
				depth[at] = bits;
			if (vis)
			{
				uint64_t word = (uint64_t)bits << VB_SHIFT | id34;
				if (word > vis[at])
					vis[at] = word;
			}
		}
	}
}

/* nv_rasterdepth with NV_OPT_RASTER_VISIBILITY_ID 1 and NV_OPT_RASTER_NEAR_CLIP = nearClip.  Arguments as rc_rasterdepth; `visibility` is the
 * frame's target (loaded, not cleared). */
void vb_rasterdepth(const Globals* g, const Command* commands, const Draw* draws, const Meshlet* meshlets, const uint32_t* data,
                    const Vertex* vertices, const uint32_t* cib, const uint32_t* cc4, uint32_t* depth, uint32_t W, uint32_t H, uint64_t* visibility,
                    uint64_t* totals4, int nearClip)
{
	const uint8_t* d8 = (const uint8_t*)data;
	const int bothFaces = g->postPass != 0;
	for (uint32_t y = 0; y < cc4[2]; ++y)
		for (uint32_t z = 0; z < cc4[3]; ++z)
			for (uint32_t x = 0; x < cc4[1]; ++x)
			{
				uint32_t index = x + y * 256 + z * CLUSTER_TILE, drawId = 0;
				uint32_t ci = cib[index];
				const Meshlet* m = slot_meshlet(commands, meshlets, ci, &drawId);
				if (!m)
					continue;
				/* the bit nv_clustercull keeps for this cluster: the same in every pass of the frame and on every rank */
				uint32_t mvi = commands[ci & 0xffffffu].meshletVisibilityOffset + (ci >> 24);
				uint64_t* vis = visibility && mvi < VB_MVI_END ? visibility : 0;
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
					uint64_t id34 = (((uint64_t)mvi << 7) | t) + 1;
					Vtx poly[4];
					int n = clip_polygon(g, v, nearClip, H, poly, 0);
					if (n >= 3)
						vb_piece(&poly[0], &poly[1], &poly[2], bothFaces, W, H, depth, vis, id34, totals4);
					if (n == 4)
						vb_piece(&poly[0], &poly[2], &poly[3], bothFaces, W, H, depth, vis, id34, totals4);
				}
			}
}

/* drawcull.comp.glsl:73-75 and :104-112 for one draw: the LOD the draw-level cull selects under `cd` */
static uint32_t vb_lod(const Cull* cd, const Draw* d, const Mesh* mesh)
{
	uint32_t lodIndex = 0;
	if (cd->lodEnabled != 1)
		return 0;
	float rc[3], wc[3], c[3];
	rotate_quat(mesh->center, d->orientation, rc);
	for (int k = 0; k < 3; ++k)
		wc[k] = rc[k] * d->scale + d->position[k];
	for (int r = 0; r < 3; ++r)
		c[r] = ((cd->view[r] * wc[0] + cd->view[4 + r] * wc[1]) + cd->view[8 + r] * wc[2]) + cd->view[12 + r];
	float radius = mesh->radius * d->scale;
	float len = sqrtf((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) - radius;
	float distance = len < 0.0f ? 0.0f : len; /* max(len, 0) */
	float threshold = distance * cd->lodTarget / d->scale;
	for (uint32_t i = 1; i < mesh->lodCount && i < 8; ++i)
		if (mesh->lods[i].error < threshold)
			lodIndex = i;
	return lodIndex;
}

/* nv_visibility_resolve on the CPU, one pixel at a time, a linear scan for the draw.  Every output is optional. */
void vb_resolve(const Cull* cd, const uint64_t* vis, uint32_t n, const Draw* draws, uint32_t drawCount, const Mesh* meshes, uint32_t meshCount,
                VisRecord* records, uint32_t* seen, uint32_t* drawPixels, uint64_t* totals4)
{
	for (uint32_t i = 0; i < n; ++i)
	{
		uint64_t word = vis[i];
		VisRecord r = { 0xffffffffu, 0, 0, 0 };
		if (word != 0)
		{
			uint64_t id34 = word & (((uint64_t)1 << VB_SHIFT) - 1);
			int ok = id34 != 0;
			uint32_t mvi = (uint32_t)((id34 - 1) >> 7), tri = (uint32_t)((id34 - 1) & 127);
			uint32_t d = 0xffffffffu, meshlet = 0;
			if (ok)
			{
				for (uint32_t k = 0; k < drawCount; ++k) /* the largest k with offset[k] <= mvi */
					if (draws[k].meshletVisibilityOffset <= mvi)
						d = k;
				ok = d != 0xffffffffu && draws[d].meshIndex < meshCount && tri < 96;
			}
			if (ok)
			{
				const Mesh* mesh = &meshes[draws[d].meshIndex];
				uint32_t lod = vb_lod(cd, &draws[d], mesh);
				uint32_t local = mvi - draws[d].meshletVisibilityOffset;
				ok = local < mesh->lods[lod].meshletCount;
				meshlet = mesh->lods[lod].meshletOffset + local;
			}
			if (totals4)
			{
				totals4[0] += 1;
				totals4[1] += ok ? 0 : 1;
			}
			if (ok)
			{
				r.drawId = d, r.meshletIndex = meshlet, r.triangle = tri, r.depthBits = (uint32_t)(word >> VB_SHIFT);
				if (seen)
					seen[mvi >> 5] |= 1u << (mvi & 31);
				if (drawPixels)
					drawPixels[d] += 1;
			}
			else
				r.drawId = r.meshletIndex = r.triangle = r.depthBits = 0xffffffffu;
		}
		if (records)
			records[i] = r;
	}
}

/* One triangle of one meshlet under one draw, alone: the samples it covers with their depth bits (the check that a resolved record names
 * geometry that is really there; both faces, as the post pass draws them).  zbits: W x H, cleared by the caller, receives the depth bits. */
void vb_single_triangle(const Globals* g, const Draw* draw, const Meshlet* m, const uint32_t* data, const Vertex* vertices, uint32_t t, int nearClip,
                        uint32_t W, uint32_t H, uint32_t* zbits)
{
	const uint8_t* d8 = (const uint8_t*)data;
	uint64_t tot[4] = { 0, 0, 0, 0 };
	uint32_t ve = m->vertexCount < MAXVTX ? m->vertexCount : MAXVTX;
	uint32_t te = m->triangleCount < MAXTRI ? m->triangleCount : MAXTRI;
	uint32_t indexOffset = m->dataOffset + (m->shortRefs == 1 ? (m->vertexCount + 1u) / 2u : m->vertexCount);
	if (t >= te)
		return;
	uint32_t o = indexOffset * 4 + t * 3;
	uint32_t ia = d8[o], ib = d8[o + 1], ic = d8[o + 2];
	if (ia >= ve || ib >= ve || ic >= ve)
		return;
	CVtx v[3] = { clip_vertex(g, draw, &vertices[vertex_ref(data, m, ia)], H), clip_vertex(g, draw, &vertices[vertex_ref(data, m, ib)], H),
		          clip_vertex(g, draw, &vertices[vertex_ref(data, m, ic)], H) };
	Vtx poly[4];
	int n = clip_polygon(g, v, nearClip, H, poly, 0);
	if (n >= 3)
		vb_piece(&poly[0], &poly[1], &poly[2], 1, W, H, zbits, 0, 0, tot);
	if (n == 4)
		vb_piece(&poly[0], &poly[2], &poly[3], 1, W, H, zbits, 0, 0, tot);
}
