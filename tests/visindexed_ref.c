/* visindexed_ref.c — CPU reference of the visibility buffer of the indexed draws: nv_rasterdepth_indexed_visibility and
 * nv_visibility_resolve_indexed (include/niagara_vis.h).
 *
 * Test infrastructure: compiled by tests/visindexed_ref.py with raster_ref.c's flags.  It includes tests/visbuffer_ref.c, and through it
 * tests/raster_clip_ref.c, tests/raster_indexed_ref.c and tests/raster_ref.c: the vertex stage, the snap, the near-plane rule, the sample loop
 * with the stable 64-bit word (vb_piece) and the LOD select (vb_lod) are the same statements as the other references; what it adds is the
 * name of a triangle of an indexed draw — tri34 = offsets[drawId] + t — and its inverse, one triangle and one pixel at a time. */
#include "visbuffer_ref.c"

#define VI_TRI34_END ((((uint64_t)1) << VB_SHIFT) - 1)

typedef struct
{
	uint32_t drawId, indexPosition, vertexOffset, depthBits;
} VisIndexedRecord;

/* nv_rasterdepth_indexed_visibility on the CPU with NV_OPT_RASTER_NEAR_CLIP = nearClip: rc_rasterdepth_indexed's loop, and the word.
 * offsets: drawCount + 1 entries (on a shard: the full array's pointer advanced by the rank's first draw); visibility: loaded, not cleared. */
void vi_rasterdepth_indexed(const Globals* g, const DrawCommand* commands, const uint32_t* count, const Draw* draws, uint32_t drawCount,
                            const uint32_t* indices, uint32_t indexCapacity, const Vertex* vertices, uint32_t vertexCapacity, uint32_t* depth,
                            uint32_t W, uint32_t H, uint64_t* totals4, int nearClip, const uint64_t* offsets, uint64_t* visibility)
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
			/* the triangle's name: the draw's, not the command's; outside the draw's span or the 34 bits: depth only */
			uint64_t tri34 = offsets[c->drawId] + t;
			uint64_t* vis = tri34 < offsets[c->drawId + 1] && tri34 < VI_TRI34_END ? visibility : 0;
			Vtx poly[4];
			int pn = clip_polygon(g, v, nearClip, H, poly, 0);
			if (pn >= 3)
				vb_piece(&poly[0], &poly[1], &poly[2], bothFaces, W, H, depth, vis, tri34 + 1, totals4);
			if (pn == 4)
				vb_piece(&poly[0], &poly[2], &poly[3], bothFaces, W, H, depth, vis, tri34 + 1, totals4);
		}
	}
}

/* nv_visibility_resolve_indexed on the CPU, one pixel at a time, a linear scan for the draw.  Every output is optional. */
void vi_resolve(const Cull* cd, const uint64_t* vis, uint32_t n, const Draw* draws, uint32_t drawCount, const Mesh* meshes, uint32_t meshCount,
                const uint64_t* offsets, VisIndexedRecord* records, uint32_t* drawPixels, uint64_t* totals4)
{
	for (uint32_t i = 0; i < n; ++i)
	{
		uint64_t word = vis[i];
		VisIndexedRecord r = { 0xffffffffu, 0, 0, 0 };
		if (word != 0)
		{
			uint64_t id34 = word & (((uint64_t)1 << VB_SHIFT) - 1);
			uint64_t tri34 = id34 - 1;
			int ok = id34 != 0 && tri34 < offsets[drawCount];
			uint32_t d = 0xffffffffu;
			if (ok)
			{
				for (uint32_t k = 0; k < drawCount; ++k) /* the largest k with offsets[k] <= tri34 */
					if (offsets[k] <= tri34)
						d = k;
				ok = d != 0xffffffffu && draws[d].meshIndex < meshCount;
			}
			if (ok)
			{
				const Mesh* mesh = &meshes[draws[d].meshIndex];
				uint32_t lod = vb_lod(cd, &draws[d], mesh);
				uint64_t t = tri34 - offsets[d];
				uint64_t at = (uint64_t)mesh->lods[lod].indexOffset + 3 * t;
				ok = t < mesh->lods[lod].indexCount / 3 && at + 2 <= 0xffffffffull;
				r.drawId = d, r.indexPosition = (uint32_t)at, r.vertexOffset = mesh->vertexOffset, r.depthBits = (uint32_t)(word >> VB_SHIFT);
			}
			if (totals4)
			{
				totals4[0] += 1;
				totals4[1] += ok ? 0 : 1;
			}
			if (ok)
			{
				if (drawPixels)
					drawPixels[d] += 1;
			}
			else
				r.drawId = r.indexPosition = r.vertexOffset = r.depthBits = 0xffffffffu;
		}
		if (records)
			records[i] = r;
	}
}
