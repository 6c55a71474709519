/* visattr_indexed_ref.c — CPU restatement of nv_visibility_attributes_indexed (include/niagara_vis.h).
 *
 * Test infrastructure: compiled by tests/visattr_indexed_ref.py with raster_ref.c's flags, in fp32 and with -DREAL=double, as its parent is.
 * It includes tests/visattr_ref.c and restates only what the indexed pass adds: which three vertices a record names (mesh.vert.glsl reads
 * gl_VertexIndex = indices[indexPosition + k] + vertexOffset, mod 2^32) and when the record is invalid.  Everything behind the three fetched
 * vertices is va_attributes itself (va_vertex and its per-pixel statements, one copy): every valid record is handed to it as a
 * one-triangle meshlet that names the same three vertices in the same order, every invalid one as a record that names no meshlet. */
#include "visattr_ref.c"
#include <stdlib.h>

typedef struct
{
	uint32_t drawId, indexPosition, vertexOffset, depthBits;
} VisIndexedRecord;

/* the three vertices an indexed record names, validated; 0 when the record is invalid (the material rule is va_triangle's) */
static int vai_triangle(const VisIndexedRecord* r, uint32_t drawCount, const uint32_t* indices, uint32_t indexCapacity, uint32_t vertexCapacity,
                        uint32_t vi[3])
{
	if (r->drawId >= drawCount)
		return 0;
	if ((uint64_t)r->indexPosition + 2 >= (uint64_t)indexCapacity)
		return 0;
	for (int k = 0; k < 3; ++k)
	{
		vi[k] = indices[(uint64_t)r->indexPosition + k] + r->vertexOffset; /* mod 2^32 */
		if (vi[k] >= vertexCapacity)
			return 0;
	}
	return 1;
}

/* nv_visibility_attributes_indexed: va_attributes' outputs and extras */
void vai_attributes(const Globals* g, const VisIndexedRecord* records, uint32_t W, uint32_t H, const Draw* draws, uint32_t drawCount,
                    const uint32_t* indices, uint32_t indexCapacity, const Vertex* vertices, uint32_t vertexCapacity, const Material* materials,
                    uint32_t materialCount, REAL* vals, uint32_t* ids, uint32_t* gb0, uint32_t* gb1, uint64_t* totals4, uint8_t* flags, REAL* chan)
{
	size_t n = (size_t)W * H;
	VisRecord* rec = (VisRecord*)calloc(n ? n : 1, sizeof(VisRecord));
	Meshlet* meshlets = (Meshlet*)calloc(n ? n : 1, sizeof(Meshlet));
	uint32_t* data = (uint32_t*)calloc(n ? 4 * n : 1, sizeof(uint32_t));
	for (size_t i = 0; i < n; ++i)
	{
		const VisIndexedRecord* r = &records[i];
		uint32_t vi[3];
		rec[i].drawId = r->drawId; /* 0xFFFFFFFF: no sample */
		rec[i].meshletIndex = 0xffffffffu;
		rec[i].triangle = 0;
		rec[i].depthBits = r->depthBits;
		if (r->drawId == 0xffffffffu || !vai_triangle(r, drawCount, indices, indexCapacity, vertexCapacity, vi))
			continue;
		/* meshlet i: three 32-bit vertex references, then the index bytes 0, 1, 2 */
		meshlets[i].dataOffset = (uint32_t)(4 * i), meshlets[i].baseVertex = 0;
		meshlets[i].vertexCount = 3, meshlets[i].triangleCount = 1, meshlets[i].shortRefs = 0;
		data[4 * i] = vi[0], data[4 * i + 1] = vi[1], data[4 * i + 2] = vi[2];
		data[4 * i + 3] = 0u | 1u << 8 | 2u << 16;
		rec[i].meshletIndex = (uint32_t)i;
	}
	va_attributes(g, rec, W, H, draws, drawCount, meshlets, (uint32_t)n, data, (uint32_t)(4 * n), vertices, vertexCapacity, materials, materialCount, vals,
	              ids, gb0, gb1, totals4, flags, chan);
	free(rec), free(meshlets), free(data);
}
