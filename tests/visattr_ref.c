/* visattr_ref.c — CPU restatement of nv_visibility_attributes (include/niagara_vis.h), one pixel at a time.
 *
 * Test infrastructure: compiled by tests/visattr_ref.py with raster_ref.c's flags, twice: as it stands (REAL = float: every statement one
 * IEEE fp32 operation, the bits the HIP kernel must write) and with -DREAL=double (the same statements in fp64 from the same fp32 / fp16
 * inputs and the same fp32 constants: the yardstick of the accuracy checks).  raster_ref.c is included for the record layouts, f16 and fbits;
 * the arithmetic is restated here in REAL.  tests/test_shading_vs_ref.py holds this file's fp32 build bit for bit
 * to the reference's unpackTBN and mesh.frag.glsl executed by oracle/_ref. */
#include "raster_ref.c"
#include <tgmath.h>

#ifndef REAL
#define REAL float
#endif
#define K(x) ((REAL)(x)) /* a constant of the shaders: the fp32 value in both builds */

typedef struct
{
	uint32_t drawId, meshletIndex, triangle, depthBits;
} VisRecord;

/* src/shaders/mesh.h:80-90 */
typedef struct
{
	uint32_t albedoTexture, normalTexture, specularTexture, emissiveTexture;
	float diffuseFactor[4], specularFactor[4], emissiveFactor[3];
	uint32_t padding;
} Material;

typedef struct
{
	REAL clip[4]; /* x, y, z, w */
	REAL uv[2], n[3], t[4], w[3];
} Corner;

/* src/shaders/math.h:46-49 rotateQuat, cross() per the GLSL spec */
static void va_rotate(const REAL v[3], const float qf[4], REAL out[3])
{
	REAL q[4] = { qf[0], qf[1], qf[2], qf[3] }, t[3], u[3];
	t[0] = q[1] * v[2] - v[1] * q[2];
	t[1] = q[2] * v[0] - v[2] * q[0];
	t[2] = q[0] * v[1] - v[0] * q[1];
	t[0] = t[0] + q[3] * v[0];
	t[1] = t[1] + q[3] * v[1];
	t[2] = t[2] + q[3] * v[2];
	u[0] = q[1] * t[2] - t[1] * q[2];
	u[1] = q[2] * t[0] - t[2] * q[0];
	u[2] = q[0] * t[1] - t[0] * q[1];
	out[0] = v[0] + K(2.0f) * u[0];
	out[1] = v[1] + K(2.0f) * u[1];
	out[2] = v[2] + K(2.0f) * u[2];
}

/* normalize(v), DESIGN.md §4.13: v / sqrt((x x + y y) + z z) per component */
static void va_normalize(REAL v[3])
{
	REAL l = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
	v[0] = v[0] / l, v[1] = v[1] / l, v[2] = v[2] / l;
}

/* src/shaders/math.h:60-67 decodeOct */
static void va_decode_oct(REAL ex, REAL ey, REAL v[3])
{
	v[0] = ex, v[1] = ey, v[2] = (K(1.0f) - fabs(ex)) - fabs(ey);
	REAL t = -v[2] < K(0.0f) ? K(0.0f) : -v[2]; /* max(-v.z, 0) */
	v[0] = v[0] + (v[0] >= K(0.0f) ? -t : t);
	v[1] = v[1] + (v[1] >= K(0.0f) ? -t : t);
	va_normalize(v);
}

/* src/shaders/math.h:104-109 unpackTBN */
static void va_unpack_tbn(uint32_t np, uint32_t tp, REAL normal[3], REAL tangent[4])
{
	for (int k = 0; k < 3; ++k)
		normal[k] = (REAL)(int32_t)(np >> (10 * k) & 1023u) / K(511.0f) - K(1.0f);
	va_decode_oct((REAL)(int32_t)(tp & 255u) / K(127.0f) - K(1.0f), (REAL)(int32_t)(tp >> 8 & 255u) / K(127.0f) - K(1.0f), tangent);
	tangent[3] = (np & (1u << 30)) != 0 ? K(-1.0f) : K(1.0f);
}

/* src/shaders/math.h:52-58 encodeOct */
static void va_encode_oct(const REAL nrm[3], REAL e[2])
{
	REAL inv = K(1.0f) / ((fabs(nrm[0]) + fabs(nrm[1])) + fabs(nrm[2]));
	REAL ox = nrm[0] * inv, oy = nrm[1] * inv;
	REAL sx = nrm[0] >= K(0.0f) ? K(1.0f) : K(-1.0f), sy = nrm[1] >= K(0.0f) ? K(1.0f) : K(-1.0f);
	e[0] = nrm[2] <= K(0.0f) ? (K(1.0f) - fabs(oy)) * sx : ox;
	e[1] = nrm[2] <= K(0.0f) ? (K(1.0f) - fabs(ox)) * sy : oy;
}

/* src/shaders/math.h:74-77 tosrgb, one component */
static REAL va_tosrgb(REAL c) { return pow(c, K(1.0f) / K(2.2f)); }

/* thin exported wrappers over the helpers above, for tests/test_shading_vs_ref.py (arrays of n arguments) */
void va_x_unpack_tbn(const uint32_t* np, const uint32_t* tp, uint32_t n, REAL* normal3, REAL* tangent4)
{
	for (uint32_t i = 0; i < n; ++i)
		va_unpack_tbn(np[i], tp[i], normal3 + 3 * (size_t)i, tangent4 + 4 * (size_t)i);
}
void va_x_decode_oct(const REAL* e, uint32_t n, REAL* out3)
{
	for (uint32_t i = 0; i < n; ++i)
		va_decode_oct(e[2 * (size_t)i], e[2 * (size_t)i + 1], out3 + 3 * (size_t)i);
}
void va_x_encode_oct(const REAL* v, uint32_t n, REAL* out2)
{
	for (uint32_t i = 0; i < n; ++i)
		va_encode_oct(v + 3 * (size_t)i, out2 + 2 * (size_t)i);
}
void va_x_tosrgb(const REAL* c, uint32_t n, REAL* out)
{
	for (uint32_t i = 0; i < n; ++i)
		out[i] = va_tosrgb(c[i]);
}

/* src/shaders/meshlet.mesh.glsl:129-140: one vertex (unpackTBN: src/shaders/math.h:104-109) */
static void va_vertex(const Globals* g, const Draw* d, const Vertex* v, Corner* o)
{
	REAL normal[3], tangent[4], position[3] = { f16(v->vx), f16(v->vy), f16(v->vz) }, rot[3], v4[4];
	va_unpack_tbn(v->np, v->tp, normal, tangent);
	o->t[3] = tangent[3];
	va_rotate(normal, d->orientation, o->n);
	va_rotate(tangent, d->orientation, o->t);
	o->uv[0] = f16(v->tu), o->uv[1] = f16(v->tv);
	va_rotate(position, d->orientation, rot);
	for (int k = 0; k < 3; ++k)
		o->w[k] = rot[k] * (REAL)d->scale + (REAL)d->position[k];
	/* :140, with the association of DESIGN.md §2 (raster_ref.c vertex_stage) */
	for (int r = 0; r < 4; ++r)
		v4[r] = (((REAL)g->view[r] * o->w[0] + (REAL)g->view[4 + r] * o->w[1]) + (REAL)g->view[8 + r] * o->w[2]) + (REAL)g->view[12 + r];
	for (int r = 0; r < 4; ++r)
		o->clip[r] = (((REAL)g->projection[r] * v4[0] + (REAL)g->projection[4 + r] * v4[1]) + (REAL)g->projection[8 + r] * v4[2]) +
		             (REAL)g->projection[12 + r] * v4[3];
}

static REAL va_mix(const REAL l[3], REAL a0, REAL a1, REAL a2) { return (l[0] * a0 + l[1] * a1) + l[2] * a2; }
static REAL va_fract(REAL x) { return x - floor(x); }

/* UNORM: clamp to [0, 1] with NaN -> 0, scale, round half to even */
static uint32_t va_unorm(REAL x, REAL scale)
{
	REAL v = x > K(0.0f) ? x : K(0.0f);
	v = v < K(1.0f) ? v : K(1.0f);
	return (uint32_t)rint(v * scale);
}

/* The triangle a record names, validated (include/niagara_vis.h: the invalid classes); 0 when the record is invalid. */
static int va_triangle(const VisRecord* r, const Draw* draws, uint32_t drawCount, const Meshlet* meshlets, uint32_t meshletCount, const uint32_t* data,
                       uint32_t dataWords, uint32_t vertexCount, const Material* materials, uint32_t materialCount, uint64_t vi[3])
{
	if (r->drawId >= drawCount || r->meshletIndex >= meshletCount)
		return 0;
	const Meshlet* m = &meshlets[r->meshletIndex];
	uint32_t ve = m->vertexCount < MAXVTX ? m->vertexCount : MAXVTX, te = m->triangleCount < MAXTRI ? m->triangleCount : MAXTRI;
	if (r->triangle >= te)
		return 0;
	/* src/shaders/meshlet.mesh.glsl:116,170 */
	uint64_t indexOffset = (uint64_t)m->dataOffset + (m->shortRefs == 1 ? (m->vertexCount + 1u) / 2u : m->vertexCount);
	uint64_t o = indexOffset * 4 + r->triangle * 3u, bytes = (uint64_t)dataWords * 4;
	const uint8_t* d8 = (const uint8_t*)data;
	const uint16_t* d16 = (const uint16_t*)data;
	for (int k = 0; k < 3; ++k)
	{
		if (o + k >= bytes)
			return 0;
		uint32_t i = d8[o + k];
		if (i >= ve)
			return 0;
		/* :127 */
		uint64_t ref;
		if (m->shortRefs == 1)
		{
			uint64_t at = (uint64_t)m->dataOffset * 2 + i;
			if (at * 2 + 2 > bytes)
				return 0;
			ref = d16[at];
		}
		else
		{
			uint64_t at = (uint64_t)m->dataOffset + i;
			if (at >= dataWords)
				return 0;
			ref = data[at];
		}
		vi[k] = ref + m->baseVertex;
		if (vi[k] >= vertexCount)
			return 0;
	}
	if (materials && draws[r->drawId].materialIndex >= materialCount)
		return 0;
	return 1;
}

/* nv_visibility_attributes.  vals: 14 REAL per pixel (uv, bary, normal, tangent, wpos: NvPixelAttributes without its two integer words), ids:
 * {drawId, materialIndex} per pixel; gb0 / gb1; totals4 (accumulated).  Extras for the tests, each optional: flags per pixel (1 shaded,
 * 2 invalid, 4 degenerate, 8 a corner of the triangle fails clip.w > 0 && clip.z <= clip.w, 16 the material names a texture) and chan, the
 * 8 G-buffer channels before the UNORM pack. */
void va_attributes(const Globals* g, const VisRecord* records, uint32_t W, uint32_t H, const Draw* draws, uint32_t drawCount, const Meshlet* meshlets,
                   uint32_t meshletCount, const uint32_t* data, uint32_t dataWords, const Vertex* vertices, uint32_t vertexCount,
                   const Material* materials, uint32_t materialCount, REAL* vals, uint32_t* ids, uint32_t* gb0, uint32_t* gb1, uint64_t* totals4,
                   uint8_t* flags, REAL* chan)
{
	for (uint32_t i = 0; i < W * H; ++i)
	{
		const VisRecord* r = &records[i];
		REAL out[14] = { 0 }, ch[8] = { 0 };
		uint32_t id[2] = { 0xffffffffu, 0 }, g0 = 0, g1 = 0;
		uint8_t fl = 0;
		uint64_t vi[3];
		int named = r->drawId != 0xffffffffu;
		int ok = named && va_triangle(r, draws, drawCount, meshlets, meshletCount, data, dataWords, vertexCount, materials, materialCount, vi);
		if (named && !ok)
			fl |= 2;
		if (ok)
		{
			const Draw* d = &draws[r->drawId];
			Corner c[3];
			for (int k = 0; k < 3; ++k)
			{
				va_vertex(g, d, &vertices[vi[k]], &c[k]);
				if (!(c[k].clip[3] > K(0.0f) && c[k].clip[2] <= c[k].clip[3]))
					fl |= 8;
			}
			fl |= 1;
			/* homogeneous barycentrics at the pixel centre, row 0 at the top */
			uint32_t py = i / W, px = i - py * W;
			REAL fx = (REAL)px + K(0.5f), fy = (REAL)py + K(0.5f);
			REAL nx = (fx / (REAL)W) * K(2.0f) - K(1.0f), ny = K(1.0f) - (fy / (REAL)H) * K(2.0f);
			REAL dx[3], dy[3], b[3], l[3];
			for (int k = 0; k < 3; ++k)
			{
				dx[k] = c[k].clip[0] - nx * c[k].clip[3];
				dy[k] = c[k].clip[1] - ny * c[k].clip[3];
			}
			b[0] = dx[1] * dy[2] - dy[1] * dx[2];
			b[1] = dx[2] * dy[0] - dy[2] * dx[0];
			b[2] = dx[0] * dy[1] - dy[0] * dx[1];
			REAL s = (b[0] + b[1]) + b[2];
			for (int k = 0; k < 3; ++k)
				l[k] = b[k] / s;
			if (s == K(0.0f) || !isfinite(l[0]) || !isfinite(l[1]) || !isfinite(l[2]))
			{
				l[0] = K(1.0f), l[1] = K(0.0f), l[2] = K(0.0f);
				fl |= 4;
			}
			REAL uv[2], n[3], t[4], w[3];
			for (int k = 0; k < 2; ++k)
				uv[k] = va_mix(l, c[0].uv[k], c[1].uv[k], c[2].uv[k]);
			for (int k = 0; k < 3; ++k)
				n[k] = va_mix(l, c[0].n[k], c[1].n[k], c[2].n[k]);
			for (int k = 0; k < 4; ++k)
				t[k] = va_mix(l, c[0].t[k], c[1].t[k], c[2].t[k]);
			for (int k = 0; k < 3; ++k)
				w[k] = va_mix(l, c[0].w[k], c[1].w[k], c[2].w[k]);
			out[0] = uv[0], out[1] = uv[1], out[2] = l[1], out[3] = l[2];
			out[4] = n[0], out[5] = n[1], out[6] = n[2];
			out[7] = t[0], out[8] = t[1], out[9] = t[2], out[10] = t[3];
			out[11] = w[0], out[12] = w[1], out[13] = w[2];
			id[0] = r->drawId, id[1] = d->materialIndex;
			if (materials)
			{
				/* src/shaders/mesh.frag.glsl:57-89 without the texture terms */
				const Material* m = &materials[d->materialIndex];
				if (m->albedoTexture > 0 || m->normalTexture > 0 || m->specularTexture > 0 || m->emissiveTexture > 0)
					fl |= 16;
				/* :60, src/shaders/math.h:99-102 gradientNoise(gl_FragCoord.xy) */
				REAL noise = va_fract(K(52.9829189f) * va_fract(fx * K(0.06711056f) + fy * K(0.00583715f)));
				REAL deband = noise * K(2.0f) - K(1.0f);
				/* :66, :78-80: nmap = (0, 0, 1), multiplications by zero included */
				REAL bt[3] = { n[1] * t[2] - t[1] * n[2], n[2] * t[0] - t[2] * n[0], n[0] * t[1] - t[0] * n[1] }, nrm[3];
				for (int k = 0; k < 3; ++k)
				{
					REAL bitangent = bt[k] * t[3];
					nrm[k] = (K(0.0f) * t[k] + K(0.0f) * bitangent) + K(1.0f) * n[k];
				}
				va_normalize(nrm);
				/* :82 */
				REAL emissivef = (((REAL)m->emissiveFactor[0] * K(0.3f) + (REAL)m->emissiveFactor[1] * K(0.6f)) + (REAL)m->emissiveFactor[2] * K(0.1f)) /
				                 ((((REAL)m->diffuseFactor[0] * K(0.3f) + (REAL)m->diffuseFactor[1] * K(0.6f)) + (REAL)m->diffuseFactor[2] * K(0.1f)) + K(1e-3f));
				/* :85, src/shaders/math.h:74-77 tosrgb */
				for (int k = 0; k < 3; ++k)
					ch[k] = va_tosrgb((REAL)m->diffuseFactor[k]);
				ch[3] = log2(K(1.0f) + emissivef) / K(5.0f);
				g0 = va_unorm(ch[0], K(255.0f)) | va_unorm(ch[1], K(255.0f)) << 8 | va_unorm(ch[2], K(255.0f)) << 16 | va_unorm(ch[3], K(255.0f)) << 24;
				/* :86, src/shaders/math.h:52-58 encodeOct */
				REAL oct[2];
				va_encode_oct(nrm, oct);
				REAL ex = oct[0], ey = oct[1];
				REAL band = deband * (K(0.5f) / K(1023.0f));
				ch[4] = (ex * K(0.5f) + K(0.5f)) + band;
				ch[5] = (ey * K(0.5f) + K(0.5f)) + band;
				ch[6] = (REAL)m->specularFactor[3];
				ch[7] = K(0.0f);
				g1 = va_unorm(ch[4], K(1023.0f)) | va_unorm(ch[5], K(1023.0f)) << 10 | va_unorm(ch[6], K(1023.0f)) << 20 | va_unorm(ch[7], K(3.0f)) << 30;
			}
		}
		if (totals4)
		{
			totals4[0] += fl & 1 ? 1 : 0;
			totals4[1] += fl & 2 ? 1 : 0;
			totals4[2] += fl & 4 ? 1 : 0;
			totals4[3] += fl & 16 ? 1 : 0;
		}
		if (vals)
			memcpy(vals + (size_t)i * 14, out, sizeof(out));
		if (ids)
			ids[2 * (size_t)i] = id[0], ids[2 * (size_t)i + 1] = id[1];
		if (gb0)
			gb0[i] = g0;
		if (gb1)
			gb1[i] = g1;
		if (flags)
			flags[i] = fl;
		if (chan)
			memcpy(chan + (size_t)i * 8, ch, sizeof(ch));
	}
}

unsigned va_real_bytes(void) { return (unsigned)sizeof(REAL); }
