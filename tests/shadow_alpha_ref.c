/* shadow_alpha_ref.c — CPU restatement of nv_shadow_trace_textured (include/niagara_vis.h): BRUTE FORCE.  There is no BVH
 * here: every casting triangle of every casting instance is tested for every ray, one after the other, and NOTHING ends the loops early, so
 * that besides the mask the restatement can say per ray how many accepted candidates the alpha test rejected.
 *
 * Test infrastructure: compiled by tests/shadow_alpha_ref.py with raster_ref.py's flags (fp32, -ffp-contract=off).  The ray, the casting rule,
 * the object-space ray and T are shadow_ref.c's (included below); T is written out once more here because the alpha test needs its U, V, W and
 * det.  The level-0 sampler is restated here from the rule set (REPEAT, bilinear, UNORM alpha = code / 255): it shares no text with
 * niagara_amd/csrc/texmath.h.
 *
 * Layouts are the C ABI's: Material 64 bytes, TextureDesc 16. */
#include "shadow_ref.c"

typedef struct
{
	uint32_t albedoTexture, normalTexture, specularTexture, emissiveTexture;
	float diffuseFactor[4], specularFactor[4], emissiveFactor[3];
	uint32_t padding;
} Material;
typedef struct
{
	uint32_t offset, width, height, levels;
} TextureDesc;

int sar_sizes_ok(void) { return shr_sizes_ok() && sizeof(Material) == 64 && sizeof(TextureDesc) == 16; }

/* T of shadow_ref.c's triangle_test, handing back U, V, W (after the fp64 fallback) and det of an accepted triangle */
static int triangle_test_uvw(const RaySetup* r, vec3 v0, vec3 v1, vec3 v2, float tmin, float tmax, float* uvwd)
{
	vec3 A = { v0.x - r->o.x, v0.y - r->o.y, v0.z - r->o.z };
	vec3 B = { v1.x - r->o.x, v1.y - r->o.y, v1.z - r->o.z };
	vec3 C = { v2.x - r->o.x, v2.y - r->o.y, v2.z - r->o.z };
	float Ax = comp(A, r->kx) - r->Sx * comp(A, r->kz), Ay = comp(A, r->ky) - r->Sy * comp(A, r->kz);
	float Bx = comp(B, r->kx) - r->Sx * comp(B, r->kz), By = comp(B, r->ky) - r->Sy * comp(B, r->kz);
	float Cx = comp(C, r->kx) - r->Sx * comp(C, r->kz), Cy = comp(C, r->ky) - r->Sy * comp(C, r->kz);
	float U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
	float det, T, t;
	if (U == 0.0f || V == 0.0f || W == 0.0f)
	{
		U = (float)((double)Cx * (double)By - (double)Cy * (double)Bx);
		V = (float)((double)Ax * (double)Cy - (double)Ay * (double)Cx);
		W = (float)((double)Bx * (double)Ay - (double)By * (double)Ax);
	}
	if ((U < 0.0f || V < 0.0f || W < 0.0f) && (U > 0.0f || V > 0.0f || W > 0.0f))
		return 0;
	det = (U + V) + W;
	if (det == 0.0f)
		return 0;
	T = (U * (r->Sz * comp(A, r->kz)) + V * (r->Sz * comp(B, r->kz))) + W * (r->Sz * comp(C, r->kz));
	t = T / det;
	uvwd[0] = U, uvwd[1] = V, uvwd[2] = W, uvwd[3] = det;
	return t > tmin && t < tmax;
}

/* the chain of `levels` levels from word `offset` lies inside texelWords, and the shape is one the library takes */
static int desc_ok(const TextureDesc* d, uint64_t texelWords)
{
	uint64_t words = 0;
	uint32_t l;
	if (d->width == 0 || d->height == 0 || d->width > 16384u || d->height > 16384u || d->levels == 0 || d->levels > 15u)
		return 0;
	for (l = 0; l < d->levels; ++l)
	{
		uint64_t w = d->width >> l, h = d->height >> l;
		words += (w ? w : 1u) * (h ? h : 1u);
	}
	return (uint64_t)d->offset + words <= texelWords;
}

/* REPEAT + LINEAR on one axis: the two texel indices and the weight of the second.  A non-finite coordinate gives a NaN weight (and index 0) */
static void wrap_axis(float x, uint32_t size, uint32_t* i0, uint32_t* i1, float* weight)
{
	float s = x - floorf(x);           /* REPEAT: the fractional part */
	float u = s * (float)size - 0.5f;  /* unnormalised, shifted to texel centres */
	float fl = floorf(u);
	int64_t i = isfinite(fl) ? (int64_t)fl : 0;
	*weight = u - fl;
	*i0 = (uint32_t)(((i % (int64_t)size) + (int64_t)size) % (int64_t)size);
	*i1 = (uint32_t)((((i + 1) % (int64_t)size) + (int64_t)size) % (int64_t)size);
}

static float mix1(float a, float b, float w) { return a * (1.0f - w) + b * w; }

/* textureLod(tex, (u, v), 0).w: level 0 only, x first, then y */
static float alpha_lod0(const uint32_t* texels, const TextureDesc* d, float u, float v)
{
	uint32_t x0, x1, y0, y1;
	float ax, ay, a00, a01, a10, a11;
	const uint32_t* level0 = texels + d->offset;
	wrap_axis(u, d->width, &x0, &x1, &ax);
	wrap_axis(v, d->height, &y0, &y1, &ay);
	a00 = (float)(level0[(size_t)y0 * d->width + x0] >> 24) / 255.0f;
	a01 = (float)(level0[(size_t)y0 * d->width + x1] >> 24) / 255.0f;
	a10 = (float)(level0[(size_t)y1 * d->width + x0] >> 24) / 255.0f;
	a11 = (float)(level0[(size_t)y1 * d->width + x1] >> 24) / 255.0f;
	return mix1(mix1(a00, a01, ax), mix1(a10, a11, ax), ay);
}

/* shadow.comp.glsl:113: uv = uva (1 - bary.x - bary.y) + uvb bary.x + uvc bary.y, the operators left to right */
static void interpolate_uv(float b1, float b2, const float* tu, const float* tv, float* u, float* v)
{
	float w0 = (1.0f - b1) - b2;
	*u = (tu[0] * w0 + tu[1] * b1) + tu[2] * b2;
	*v = (tv[0] * w0 + tv[1] * b1) + tv[2] * b2;
}

/* the same for n hits (test infrastructure: tests/test_shadow_vs_ref.py holds the reference's uv against it).  bary: n x 2, tu / tv: n x 3 */
void sar_interpolate_uv(const float* bary, const float* tu, const float* tv, uint64_t n, float* uv)
{
	uint64_t i;
	for (i = 0; i < n; ++i)
		interpolate_uv(bary[2 * i], bary[2 * i + 1], tu + 3 * i, tv + 3 * i, &uv[2 * i], &uv[2 * i + 1]);
}

typedef struct
{
	const Material* materials;
	uint32_t materialCount;
	const TextureDesc* textures;
	uint32_t textureCount;
	const uint32_t* texels;
	uint64_t texelWords;
} AlphaInputs;

/* 1 when some accepted triangle is confirmed.  *rejected = the accepted triangles (of all casting instances) the alpha test did not confirm */
static int occluded_alpha(const Mesh* meshes, uint32_t meshCount, const uint32_t* indices, uint32_t indexCapacity, const Vertex* vertices,
                          uint32_t vertexCapacity, const MeshDraw* draws, uint32_t drawCount, const AlphaInputs* in, vec3 o, vec3 d, float tmin, float tmax,
                          int quality, uint32_t* rejected)
{
	uint32_t i, t, k;
	int hit = 0;
	*rejected = 0;
	if (!(finite1(o.x) && finite1(o.y) && finite1(o.z) && finite1(d.x) && finite1(d.y) && finite1(d.z)))
		return 0;
	for (i = 0; i < drawCount; ++i)
	{
		const MeshDraw* dr = &draws[i];
		const Mesh* mesh;
		const MeshLod* lod;
		const TextureDesc* tex = NULL; /* NULL: every accepted triangle of this instance is confirmed */
		vec3 c, rel, ro, rd, o2, d2;
		RaySetup rs;
		if (!draw_casts(dr, meshCount, quality))
			continue;
		mesh = &meshes[dr->meshIndex];
		if (mesh->lodRT >= 8u || mesh->lodRT >= mesh->lodCount)
			continue;
		lod = &mesh->lods[mesh->lodRT];
		if (quality == 1 && dr->postPass == 1u && dr->materialIndex < in->materialCount)
		{
			uint32_t id = in->materials[dr->materialIndex].albedoTexture;
			if (id != 0 && id < in->textureCount && desc_ok(&in->textures[id], in->texelWords))
				tex = &in->textures[id];
		}
		c.x = -dr->orientation[0], c.y = -dr->orientation[1], c.z = -dr->orientation[2];
		rel.x = o.x - dr->position[0], rel.y = o.y - dr->position[1], rel.z = o.z - dr->position[2];
		ro = rotate_quat(rel, c, dr->orientation[3]);
		rd = rotate_quat(d, c, dr->orientation[3]);
		o2.x = ro.x / dr->scale, o2.y = ro.y / dr->scale, o2.z = ro.z / dr->scale;
		d2.x = rd.x / dr->scale, d2.y = rd.y / dr->scale, d2.z = rd.z / dr->scale;
		rs = ray_setup(o2, d2);
		for (t = 0; t < lod->indexCount / 3u; ++t)
		{
			vec3 v[3];
			float tu[3], tv[3], uvwd[4];
			int keep = 1;
			for (k = 0; k < 3u; ++k)
			{
				uint64_t at = (uint64_t)lod->indexOffset + 3ull * t + k, corner;
				if (at >= indexCapacity)
				{
					keep = 0;
					break;
				}
				corner = (uint64_t)mesh->vertexOffset + indices[at];
				if (corner >= vertexCapacity)
				{
					keep = 0;
					break;
				}
				v[k].x = half_to_float(vertices[corner].vx), v[k].y = half_to_float(vertices[corner].vy), v[k].z = half_to_float(vertices[corner].vz);
				tu[k] = half_to_float(vertices[corner].tu), tv[k] = half_to_float(vertices[corner].tv);
			}
			if (!keep || !triangle_test_uvw(&rs, v[0], v[1], v[2], tmin, tmax, uvwd))
				continue;
			if (tex)
			{
				float b1 = uvwd[1] / uvwd[3], b2 = uvwd[2] / uvwd[3];
				float u, w, alpha;
				interpolate_uv(b1, b2, tu, tv, &u, &w);
				alpha = alpha_lod0(in->texels, tex, u, w);
				if (!(alpha >= 0.5f)) /* a NaN does not confirm */
				{
					++*rejected;
					continue;
				}
			}
			hit = 1;
		}
	}
	return hit;
}

/* out[i] = 0 (occluded) or 255, rejected[i] = the candidates of ray i the alpha test rejected, for n given rays */
void sar_trace(const Mesh* meshes, uint32_t meshCount, const uint32_t* indices, uint32_t indexCapacity, const Vertex* vertices, uint32_t vertexCapacity,
               const MeshDraw* draws, uint32_t drawCount, const Material* materials, uint32_t materialCount, const TextureDesc* textures, uint32_t textureCount,
               const uint32_t* texels, uint64_t texelWords, const float* origins, const float* dirs, uint64_t n, float tmin, float tmax, int quality,
               uint8_t* out, uint32_t* rejected)
{
	AlphaInputs in = { materials, materialCount, textures, textureCount, texels, texelWords };
	uint64_t i;
	for (i = 0; i < n; ++i)
	{
		vec3 o = { origins[3 * i], origins[3 * i + 1], origins[3 * i + 2] }, d = { dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2] };
		out[i] = occluded_alpha(meshes, meshCount, indices, indexCapacity, vertices, vertexCapacity, draws, drawCount, &in, o, d, tmin, tmax, quality, &rejected[i]) ? 0
		                                                                                                                                                            : 255;
	}
}

/* the pass over W' x h invocations, in place in `shadow` (texels no invocation owns keep their bytes) and `rejected` (w * h, the same rule) */
void sar_shadow_trace(const ShadowData* sd, const Mesh* meshes, uint32_t meshCount, const uint32_t* indices, uint32_t indexCapacity, const Vertex* vertices,
                      uint32_t vertexCapacity, const MeshDraw* draws, uint32_t drawCount, const Material* materials, uint32_t materialCount,
                      const TextureDesc* textures, uint32_t textureCount, const uint32_t* texels, uint64_t texelWords, const float* depth, uint8_t* shadow,
                      uint32_t* rejected, uint32_t w, uint32_t h, int quality)
{
	AlphaInputs in = { materials, materialCount, textures, textureCount, texels, texelWords };
	uint32_t gx, gy, wi = sd->checkerboard > 0 ? (w + 1u) / 2u : w;
	for (gy = 0; gy < h; ++gy)
		for (gx = 0; gx < wi; ++gx)
		{
			int64_t px = gx;
			vec3 o, d;
			size_t at;
			if (sd->checkerboard > 0)
				px = px * 2 + (((int32_t)gy ^ sd->checkerboard) & 1);
			if (px >= (int64_t)w) /* a store outside the image is dropped */
				continue;
			at = (size_t)gy * w + (size_t)px;
			pixel_ray(sd, (uint32_t)px, gy, depth[at], &o, &d);
			shadow[at] = occluded_alpha(meshes, meshCount, indices, indexCapacity, vertices, vertexCapacity, draws, drawCount, &in, o, d, 1e-2f, 1e3f, quality,
			                            &rejected[at])
			                 ? 0
			                 : 255;
		}
}
