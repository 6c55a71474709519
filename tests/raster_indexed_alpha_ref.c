/* raster_indexed_alpha_ref.c — CPU restatement of nv_rasterdepth_indexed_textured (include/niagara_vis.h): the indexed raster
 * with a visibility word whose covered samples of a post-pass launch also pass the fragment's alpha test.
 *
 * Test infrastructure: compiled by tests/raster_indexed_alpha_ref.py with raster_ref.c's flags.  It includes tests/visindexed_ref.c and copies
 * nothing of it: the command loop below is vi_rasterdepth_indexed's, and every piece is drawn by vb_piece ITSELF into a private target of
 * the piece's box, so coverage, the top-left rule, the depth of a sample and the totals' third word are that function's statements.  What
 * this file adds sits between that private target and the caller's: a covered sample asks raster_alpha_ref.c's -DRA_FRAGMENT library
 * (ra_fragment_alpha, through a function pointer: texture_ref.c's statements) for its alpha and is kept or dropped by §4.24's rule per
 * command before it touches depth or visibility. */
#include "visindexed_ref.c"
#include <stdlib.h>

/* src/shaders/mesh.h:80-90 and NvTextureDesc, as far as the rule reads them (the layouts ra_fragment_alpha takes) */
typedef struct
{
	uint32_t albedoTexture, normalTexture, specularTexture, emissiveTexture;
	float diffuseFactor[4], specularFactor[4], emissiveFactor[3];
	uint32_t padding;
} RiaMaterial;
typedef struct
{
	uint32_t offset, width, height, levels;
} RiaDesc;

typedef int (*RiaFragment)(const Globals*, const Draw*, const Vertex*, const Vertex*, const Vertex*, uint32_t, uint32_t, uint32_t, uint32_t,
                           const RiaMaterial*, const RiaDesc*, uint32_t, const uint32_t*, uint64_t, float*);

/* one covered sample.  status: ra_fragment_alpha's (0 no albedo texture, 1 sampled, 2 named but not sampled), 3 = materialIndex past the
 * table, 4 = the launch does not test */
typedef struct
{
	uint32_t px, py, command, triangle, keep, status;
	float alpha;
} RiaSample;

typedef struct
{
	const RiaMaterial* materials; /* optional */
	uint32_t materialCount;
	const RiaDesc* descs;
	uint32_t textureCount;
	const uint32_t* texels;
	uint64_t texelWords;
	RiaFragment fragment;
	int32_t nearClip;
	uint64_t* alphaTotals2; /* dropped, unevaluated */
	RiaSample* log;         /* optional */
	uint64_t logCapacity, logCount; /* logCount keeps counting past the capacity */
} RiaParams;

typedef struct
{
	const Globals* g;
	const Draw* draw;
	const Vertex* v[3]; /* the ORIGINAL triangle's corners, stored order */
	uint32_t command, triangle;
	int test;           /* the launch tests (postPass != 0 and a material table) */
} RiaTri;

/* one piece: vb_piece into the private target (box: a zeroed W x H pair), then sample by sample the rule and the caller's targets */
static void ria_piece(const Vtx* a, const Vtx* b, const Vtx* c, int bothFaces, uint32_t W, uint32_t H, uint32_t* depth, uint64_t* vis, uint64_t id34,
                      uint64_t* totals4, const RiaTri* t, RiaParams* p, uint32_t* boxDepth, uint64_t* boxVis)
{
	uint64_t tot[4] = { 0, 0, 0, 0 };
	vb_piece(a, b, c, bothFaces, W, H, boxDepth, boxVis, 1, tot); /* id 1: a covered sample's private word is never 0 */
	totals4[2] += tot[2];
	if (tot[3] == 0)
		return;
	/* the rows and columns the piece can have touched: its corners' pixels, clamped (a drawn piece has no bad corner) */
	int64_t x0 = a->X, x1 = a->X, y0 = a->Y, y1 = a->Y;
	const Vtx* vs[2] = { b, c };
	for (int k = 0; k < 2; ++k)
	{
		x0 = vs[k]->X < x0 ? vs[k]->X : x0, x1 = vs[k]->X > x1 ? vs[k]->X : x1;
		y0 = vs[k]->Y < y0 ? vs[k]->Y : y0, y1 = vs[k]->Y > y1 ? vs[k]->Y : y1;
	}
	x0 = fdiv256(x0) - 1, x1 = fdiv256(x1) + 1, y0 = fdiv256(y0) - 1, y1 = fdiv256(y1) + 1;
	x0 = x0 > 0 ? x0 : 0, y0 = y0 > 0 ? y0 : 0;
	x1 = x1 < (int64_t)W - 1 ? x1 : (int64_t)W - 1, y1 = y1 < (int64_t)H - 1 ? y1 : (int64_t)H - 1;
	uint64_t seen = 0;
	for (int64_t py = y0; py <= y1; ++py)
		for (int64_t px = x0; px <= x1; ++px)
		{
			size_t at = (size_t)py * W + (size_t)px;
			uint64_t word = boxVis[at];
			if (word == 0)
				continue;
			boxVis[at] = 0, boxDepth[at] = 0;
			seen += 1;
			uint32_t bits = (uint32_t)(word >> VB_SHIFT);
			/* ---- §4.24: the fragment's alpha test (mesh.frag.glsl:88), per command */
			int keep = 1, status = 4;
			float alpha = 1.0f;
			if (t->test)
			{
				uint32_t mi = t->draw->materialIndex;
				if (mi >= p->materialCount)
				{
					status = 3;
					p->alphaTotals2[1] += 1;
				}
				else
				{
					status = p->fragment(t->g, t->draw, t->v[0], t->v[1], t->v[2], W, H, (uint32_t)px, (uint32_t)py, &p->materials[mi], p->descs,
					                     p->textureCount, p->texels, p->texelWords, &alpha);
					if (status == 2)
						p->alphaTotals2[1] += 1;
					keep = !(alpha < 0.5f); /* a NaN alpha keeps the sample */
				}
			}
			if (p->log)
			{
				if (p->logCount < p->logCapacity)
				{
					RiaSample s = { (uint32_t)px, (uint32_t)py, t->command, t->triangle, (uint32_t)keep, (uint32_t)status, alpha };
					p->log[p->logCount] = s;
				}
				p->logCount += 1;
			}
			if (!keep)
			{
				p->alphaTotals2[0] += 1;
				continue;
			}
			totals4[3] += 1;
			if (bits > depth[at])
				depth[at] = bits;
			if (vis)
			{
				uint64_t w = (uint64_t)bits << VB_SHIFT | id34;
				if (w > vis[at])
					vis[at] = w;
			}
		}
	if (seen != tot[3]) /* the box missed a covered sample: the restatement itself is wrong */
		abort();
}

/* nv_rasterdepth_indexed_textured on the CPU.  The arguments of vi_rasterdepth_indexed; offsets / visibility optional as a pair. */
void ria_rasterdepth_indexed(const Globals* g, const DrawCommand* commands, const uint32_t* count, const Draw* draws, uint32_t drawCount,
                             const uint32_t* indices, uint32_t indexCapacity, const Vertex* vertices, uint32_t vertexCapacity, uint32_t* depth,
                             uint32_t W, uint32_t H, uint64_t* totals4, const uint64_t* offsets, uint64_t* visibility, RiaParams* p)
{
	const int bothFaces = g->postPass != 0;
	const int test = g->postPass != 0 && p->materials != 0;
	uint32_t* boxDepth = (uint32_t*)calloc((size_t)W * H, sizeof(uint32_t));
	uint64_t* boxVis = (uint64_t*)calloc((size_t)W * H, sizeof(uint64_t));
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
			uint64_t* vis = 0;
			uint64_t tri34 = 0;
			if (offsets && visibility)
			{
				tri34 = offsets[c->drawId] + t;
				vis = tri34 < offsets[c->drawId + 1] && tri34 < VI_TRI34_END ? visibility : 0;
			}
			RiaTri tri = { g, &draws[c->drawId], { &vertices[id[0]], &vertices[id[1]], &vertices[id[2]] }, i, t, test };
			Vtx poly[4];
			int pn = clip_polygon(g, v, p->nearClip, H, poly, 0);
			if (pn >= 3)
				ria_piece(&poly[0], &poly[1], &poly[2], bothFaces, W, H, depth, vis, tri34 + 1, totals4, &tri, p, boxDepth, boxVis);
			if (pn == 4)
				ria_piece(&poly[0], &poly[2], &poly[3], bothFaces, W, H, depth, vis, tri34 + 1, totals4, &tri, p, boxDepth, boxVis);
		}
	}
	free(boxDepth), free(boxVis);
}

unsigned ria_sample_bytes(void) { return (unsigned)sizeof(RiaSample); }
unsigned ria_params_bytes(void) { return (unsigned)sizeof(RiaParams); }
