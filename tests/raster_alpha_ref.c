/* raster_alpha_ref.c — CPU restatement of nv_rasterdepth_textured (include/niagara_vis.h): nv_rasterdepth whose covered samples
 * of a post-pass launch also pass the fragment's alpha test.
 *
 * Test infrastructure: compiled by tests/raster_alpha_ref.py with raster_ref.c's flags (fp32, -ffp-contract=off), as TWO libraries of this
 * one file, because raster_clip_ref.c and texture_ref.c both include raster_ref.c and cannot share a translation unit:
 *   - with -DRA_FRAGMENT it includes texture_ref.c and exports ra_fragment_alpha: albedo.a of one fragment, taken with texture_ref.c's own
 *     statements (va_vertex, tr_bary, va_mix, tr_sample) in tr_attributes' order — not a third copy of the sampler or the barycentrics;
 *   - without it, it includes raster_clip_ref.c (and with it raster_ref.c) and walks sample by sample as they do: vertex stage, snap, clip
 *     polygon, edge functions and the top-left rule are their statements; a covered sample asks the first library (a function pointer) for
 *     its alpha and is kept or dropped by §4.20's rule before it touches either target. */
#ifdef RA_FRAGMENT
#include "texture_ref.c"

/* albedo.a (mesh.frag.glsl:62-64) of the fragment of triangle (v0, v1, v2: stored order) of draw d at pixel (px, py).  Returns 0: the material
 * names no albedo texture (alpha = diffuseFactor.a); 1: sampled; 2: named, not sampled (tr_sample refused: alpha = diffuseFactor.a) */
int ra_fragment_alpha(const Globals* g, const Draw* d, const Vertex* v0, const Vertex* v1, const Vertex* v2, uint32_t W, uint32_t H, uint32_t px,
                      uint32_t py, const Material* m, const TexDesc* descs, uint32_t textureCount, const uint32_t* texels, uint64_t texelWords, float* alpha)
{
	Corner c[3];
	va_vertex(g, d, v0, &c[0]);
	va_vertex(g, d, v1, &c[1]);
	va_vertex(g, d, v2, &c[2]);
	REAL fx = (REAL)px + K(0.5f), fy = (REAL)py + K(0.5f), l[3], lx[3], ly[3];
	tr_bary(c, fx, fy, W, H, l);
	REAL uv[2], dx[2] = { 0, 0 }, dy[2] = { 0, 0 }, s[4];
	for (int k = 0; k < 2; ++k)
		uv[k] = va_mix(l, c[0].uv[k], c[1].uv[k], c[2].uv[k]);
	if (!tr_bary(c, (REAL)(px + 1) + K(0.5f), fy, W, H, lx))
		for (int k = 0; k < 2; ++k)
			dx[k] = va_mix(lx, c[0].uv[k], c[1].uv[k], c[2].uv[k]) - uv[k];
	if (!tr_bary(c, fx, (REAL)(py + 1) + K(0.5f), W, H, ly))
		for (int k = 0; k < 2; ++k)
			dy[k] = va_mix(ly, c[0].uv[k], c[1].uv[k], c[2].uv[k]) - uv[k];
	REAL a = (REAL)m->diffuseFactor[3];
	int status = 0;
	if (m->albedoTexture > 0)
	{
		if (tr_sample(descs, textureCount, texels, texelWords, m->albedoTexture, uv, dx, dy, s))
			a = a * s[3], status = 1;
		else
			status = 2;
	}
	*alpha = (float)a;
	return status;
}

#else
#include "raster_clip_ref.c"

/* src/shaders/mesh.h:80-90 and NvTextureDesc, as far as the rule reads them */
typedef struct
{
	uint32_t albedoTexture, normalTexture, specularTexture, emissiveTexture;
	float diffuseFactor[4], specularFactor[4], emissiveFactor[3];
	uint32_t padding;
} RaMaterial;
typedef struct
{
	uint32_t offset, width, height, levels;
} RaDesc;

typedef int (*RaFragment)(const Globals*, const Draw*, const Vertex*, const Vertex*, const Vertex*, uint32_t, uint32_t, uint32_t, uint32_t, const RaMaterial*,
                          const RaDesc*, uint32_t, const uint32_t*, uint64_t, float*);

/* one covered sample, for the tests that compare sample by sample */
typedef struct
{
	uint32_t px, py, index, drawId, meshlet, triangle, keep, status; /* status: ra_fragment_alpha's, 3 = materialIndex past the table, 4 = the launch does not test */
	float alpha;
} RaSample;

enum
{
	RA_SLOTS_TESTED,      /* slots whose material's albedo texture is sampled */
	RA_SLOTS_CONSTANT,    /* slots without an albedo texture */
	RA_SLOTS_ABSENT,      /* slots whose albedo texture is past the table or fails the descriptor rule */
	RA_SLOTS_OPAQUE,      /* slots whose materialIndex is past the table */
	RA_TESTED_SAMPLES,    /* covered samples of tested slots */
	RA_UNDECIDED,         /* of those, |alpha - 0.5| <= B */
	RA_TESTED_SMALL,      /* pieces of tested slots whose box holds 1 .. smallLimit centres */
	RA_TESTED_LARGE,      /* ... more than smallLimit */
	RA_TESTED_CUT_STAMPS, /* large pieces of tested slots whose box is no multiple of 8 in width AND in height */
	RA_TESTED_CLIPPED,    /* pieces of tested slots that come from a clipped triangle */
	RA_NAN_ALPHA,         /* covered samples whose alpha is NaN (kept) */
	RA_COUNTERS
};

typedef struct
{
	const RaMaterial* materials; /* optional */
	uint32_t materialCount;
	const RaDesc* descs;
	uint32_t textureCount;
	const uint32_t* texels;
	uint64_t texelWords;
	RaFragment fragment;
	int32_t nearClip, stable;
	int32_t band;     /* 1: a tested sample with |alpha - 0.5| <= B (§4.20) is UNDECIDED; `policy` then says what becomes of it */
	int32_t policy;   /* 0: the rule; 1: every undecided sample dropped; 2: every undecided sample kept */
	uint32_t smallLimit; /* for the counters only: the restatement has one path */
	uint64_t* alphaTotals2; /* dropped, unevaluated */
	uint64_t* counters;     /* RA_COUNTERS */
	uint8_t* undecidedMask; /* optional, W x H: 1 where an undecided sample covers the pixel */
	RaSample* log;          /* optional */
	uint64_t logCapacity, logCount; /* logCount keeps counting past the capacity */
} RaParams;

typedef struct
{
	const Globals* g;
	const Draw* draw;
	const Vertex* v[3]; /* the ORIGINAL triangle's corners, stored order */
	uint32_t index, drawId, meshlet, triangle;
	int test;           /* the launch tests (postPass != 0 and a material table) */
	int tested;         /* the slot's albedo texture is sampled */
	int clipped;
	double B;
} RaTri;

/* draw_piece (raster_clip_ref.c) with the alpha test between the coverage and the targets; word: the visibility word's low part, shift: 32 or 34 */
static void ra_piece(const Vtx* a, const Vtx* b, const Vtx* c, int bothFaces, uint32_t W, uint32_t H, uint32_t* depth, uint64_t* visibility, uint64_t id,
                     int shift, uint64_t* totals4, const RaTri* t, RaParams* p)
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
	if (t->tested && px0 <= px1 && py0 <= py1)
	{
		uint64_t n = (uint64_t)(px1 - px0 + 1) * (uint64_t)(py1 - py0 + 1);
		p->counters[n > p->smallLimit ? RA_TESTED_LARGE : RA_TESTED_SMALL] += 1;
		if (n > p->smallLimit && (px1 - px0 + 1) % 8 != 0 && (py1 - py0 + 1) % 8 != 0)
			p->counters[RA_TESTED_CUT_STAMPS] += 1;
		p->counters[RA_TESTED_CLIPPED] += t->clipped ? 1 : 0;
	}
	for (int64_t py = py0; py <= py1; ++py)
	{
		int64_t sy = py * 256 + 128;
		for (int64_t px = px0; px <= px1; ++px)
		{
			int64_t sx = px * 256 + 128;
			int64_t wa = edge(b, c, sx, sy), wb = edge(c, a, sx, sy), wc = edge(a, b, sx, sy);
			if (!covers(wa, tbc) || !covers(wb, tca) || !covers(wc, tab))
				continue;
			size_t at = (size_t)py * W + (size_t)px;
			/* ---- §4.20: the fragment's alpha test (mesh.frag.glsl:88) */
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
					status = p->fragment(t->g, t->draw, t->v[0], t->v[1], t->v[2], W, H, (uint32_t)px, (uint32_t)py, &p->materials[mi], p->descs, p->textureCount,
					                     p->texels, p->texelWords, &alpha);
					if (status == 2)
						p->alphaTotals2[1] += 1;
					keep = !(alpha < 0.5f); /* a NaN alpha keeps the sample */
					if (alpha != alpha)
						p->counters[RA_NAN_ALPHA] += 1;
					if (status == 1)
					{
						p->counters[RA_TESTED_SAMPLES] += 1;
						if (p->band && fabs((double)alpha - 0.5) <= t->B)
						{
							p->counters[RA_UNDECIDED] += 1;
							if (p->undecidedMask)
								p->undecidedMask[at] = 1;
							keep = p->policy == 1 ? 0 : p->policy == 2 ? 1 : keep;
						}
					}
				}
			}
			if (p->log)
			{
				if (p->logCount < p->logCapacity)
				{
					RaSample s = { (uint32_t)px, (uint32_t)py, t->index, t->drawId, t->meshlet, t->triangle, (uint32_t)keep, (uint32_t)status, alpha };
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
			float zz = (a->z + ((float)wb * inv) * (b->z - a->z)) + ((float)wc * inv) * (c->z - a->z);
			zz = zz > 0.0f ? zz : 0.0f;
			zz = zz < 1.0f ? zz : 1.0f;
			uint32_t bits = fbits(zz);
			if (bits > depth[at])
				depth[at] = bits;
			if (visibility)
			{
				uint64_t word = (uint64_t)bits << shift | id;
				if (word > visibility[at])
					visibility[at] = word;
			}
		}
	}
}

/* nv_rasterdepth_textured on the CPU.  The first thirteen arguments as rr_rasterdepth. */
void ra_rasterdepth(const Globals* g, const Command* commands, const Draw* draws, const Meshlet* meshlets, const uint32_t* data, const Vertex* vertices,
                    const uint32_t* cib, const uint32_t* cc4, uint32_t* depth, uint32_t W, uint32_t H, uint64_t* visibility, uint64_t* totals4, RaParams* p)
{
	const uint8_t* d8 = (const uint8_t*)data;
	const int bothFaces = g->postPass != 0;
	const int test = g->postPass != 0 && p->materials != 0;
	for (uint32_t y = 0; y < cc4[2]; ++y)
		for (uint32_t z = 0; z < cc4[3]; ++z)
			for (uint32_t x = 0; x < cc4[1]; ++x)
			{
				uint32_t index = x + y * 256 + z * CLUSTER_TILE, drawId = 0;
				uint32_t ci = cib[index];
				const Meshlet* m = slot_meshlet(commands, meshlets, ci, &drawId);
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
				/* the slot's road (§4.20 "Per slot") */
				RaTri t = { g, &draws[drawId], { 0, 0, 0 }, index, drawId, commands[ci & 0xffffffu].taskOffset + (ci >> 24), 0, test, 0, 0, 0.0 };
				if (test)
				{
					uint32_t mi = draws[drawId].materialIndex;
					if (mi >= p->materialCount)
						p->counters[RA_SLOTS_OPAQUE] += 1;
					else if (!(p->materials[mi].albedoTexture > 0))
						p->counters[RA_SLOTS_CONSTANT] += 1;
					else
					{
						/* whether the texture can be sampled is tr_sample's decision, sample by sample; the slot is classified by asking it once */
						uint32_t id = p->materials[mi].albedoTexture;
						float alpha;
						int status = ve ? p->fragment(g, &draws[drawId], &vertices[vertex_ref(data, m, 0)], &vertices[vertex_ref(data, m, 0)],
						                              &vertices[vertex_ref(data, m, 0)], W, H, 0, 0, &p->materials[mi], p->descs, p->textureCount, p->texels,
						                              p->texelWords, &alpha)
						                : 2;
						t.tested = status == 1;
						p->counters[t.tested ? RA_SLOTS_TESTED : RA_SLOTS_ABSENT] += 1;
						if (t.tested) /* §4.18's counted bound for this texture, plus the product with the factor */
							t.B = (3.0 * ((double)p->descs[id].width + (double)p->descs[id].height) + 32.0) / 16777216.0 + 1.0 / 16777216.0;
					}
				}
				/* the visibility word: slot << 7 | triangle, or the stable form (visbuffer_ref.c) */
				uint32_t mvi = commands[ci & 0xffffffu].meshletVisibilityOffset + (ci >> 24);
				uint64_t* vis = visibility;
				if (p->stable && !(mvi < (1u << 27) - 1u))
					vis = 0;
				for (uint32_t tr = 0; tr < te; ++tr)
				{
					uint32_t o = indexOffset * 4 + tr * 3;
					uint32_t ia = d8[o], ib = d8[o + 1], ic = d8[o + 2];
					if (ia >= ve || ib >= ve || ic >= ve)
						continue;
					CVtx v[3] = { vs[ia], vs[ib], vs[ic] };
					t.v[0] = &vertices[vertex_ref(data, m, ia)], t.v[1] = &vertices[vertex_ref(data, m, ib)], t.v[2] = &vertices[vertex_ref(data, m, ic)];
					t.triangle = tr;
					uint64_t id = p->stable ? (((uint64_t)mvi << 7) | tr) + 1 : (uint64_t)index << 7 | tr;
					Vtx poly[4];
					int n = clip_polygon(g, v, p->nearClip, H, poly, 0);
					t.clipped = n >= 3 && !(v[0].inside && v[1].inside && v[2].inside) && p->nearClip;
					if (n >= 3)
						ra_piece(&poly[0], &poly[1], &poly[2], bothFaces, W, H, depth, vis, id, p->stable ? 34 : 32, totals4, &t, p);
					if (n == 4)
						ra_piece(&poly[0], &poly[2], &poly[3], bothFaces, W, H, depth, vis, id, p->stable ? 34 : 32, totals4, &t, p);
				}
			}
}

unsigned ra_sample_bytes(void) { return (unsigned)sizeof(RaSample); }
unsigned ra_params_bytes(void) { return (unsigned)sizeof(RaParams); }
#endif
