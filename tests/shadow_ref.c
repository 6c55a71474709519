/* shadow_ref.c — CPU restatement of nv_shadow_trace (include/niagara_vis.h): BRUTE FORCE.  There is no BVH here: the mask
 * is the OR of the triangle test T over every casting triangle of every casting instance, one ray at a time.  The library's BVH is an
 * acceleration that must never change a bit of this.
 *
 * Test infrastructure: compiled by tests/shadow_ref.py with raster_ref.py's flags (fp32, -ffp-contract=off).  Written from the rule set of
 * §4.16; every fp32 operation is one IEEE operation in the stated order, mat4 * vec4 and dot associate left to right.
 *
 * Layouts are the C ABI's (src/scene.h): Mesh 208 bytes, MeshDraw 48, Vertex 16, ShadowData 96. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct
{
	uint32_t indexOffset, indexCount, meshletOffset, meshletCount;
	float error;
} MeshLod;
typedef struct
{
	float center[3], radius;
	uint32_t vertexOffset, vertexCount, ommIndexData, ommIndexBase, lodCount, lodRT, padding[2];
	MeshLod lods[8];
} Mesh;
typedef struct
{
	float position[3], scale, orientation[4];
	uint32_t meshIndex, meshletVisibilityOffset, postPass, materialIndex;
} MeshDraw;
typedef struct
{
	uint16_t vx, vy, vz, tp;
	uint32_t np;
	uint16_t tu, tv;
} Vertex;
typedef struct /* shadow.comp.glsl:26-35 */
{
	float sunDirection[3], sunJitter, inverseViewProjection[16], imageSize[2];
	int32_t checkerboard;
	uint32_t pad;
} ShadowData;

typedef struct
{
	float x, y, z;
} vec3;

int shr_sizes_ok(void) { return sizeof(Mesh) == 208 && sizeof(MeshDraw) == 48 && sizeof(Vertex) == 16 && sizeof(ShadowData) == 96; }

static float half_to_float(uint16_t h) /* exact */
{
	uint32_t s = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 1023u, bits;
	float v;
	if (e == 0)
	{
		v = (float)m * 5.9604644775390625e-8f;
		return s ? -v : v;
	}
	bits = s | (e == 31u ? 0x7f800000u | m << 13 : (e + 112u) << 23 | m << 13);
	memcpy(&v, &bits, 4);
	return v;
}

static int finite1(float f) { return isfinite(f) != 0; }

/* math.h:99-102 */
static float gradient_noise(float x, float y)
{
	float inner = x * 0.06711056f + y * 0.00583715f;
	float f0 = inner - floorf(inner);
	float n1 = 52.9829189f * f0;
	return n1 - floorf(n1);
}

/* shadow.comp.glsl:136-151 for the pixel (px, py) with the depth texel `depth` */
static void pixel_ray(const ShadowData* sd, uint32_t px, uint32_t py, float depth, vec3* o, vec3* d)
{
	const float* m = sd->inverseViewProjection;
	float uvx = ((float)px + 0.5f) / sd->imageSize[0], uvy = ((float)py + 0.5f) / sd->imageSize[1];
	float cx = uvx * 2.0f - 1.0f, cy = 1.0f - uvy * 2.0f;
	float hx = ((m[0] * cx + m[4] * cy) + m[8] * depth) + m[12] * 1.0f;
	float hy = ((m[1] * cx + m[5] * cy) + m[9] * depth) + m[13] * 1.0f;
	float hz = ((m[2] * cx + m[6] * cy) + m[10] * depth) + m[14] * 1.0f;
	float hw = ((m[3] * cx + m[7] * cy) + m[11] * depth) + m[15] * 1.0f;
	float dx, dy, dz, l;
	o->x = hx / hw, o->y = hy / hw, o->z = hz / hw;
	dx = sd->sunDirection[0], dy = sd->sunDirection[1], dz = sd->sunDirection[2];
	dx = dx + (gradient_noise((float)px, (float)py) * 2.0f - 1.0f) * sd->sunJitter;
	dz = dz + (gradient_noise((float)py, (float)px) * 2.0f - 1.0f) * sd->sunJitter;
	l = sqrtf((dx * dx + dy * dy) + dz * dz);
	d->x = dx / l, d->y = dy / l, d->z = dz / l;
}

static vec3 cross3(vec3 a, vec3 b)
{
	vec3 o = { a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y };
	return o;
}

/* math.h:46-49: v + 2.0 * cross(q.xyz, cross(q.xyz, v) + q.w * v) */
static vec3 rotate_quat(vec3 v, vec3 q, float qw)
{
	vec3 t = cross3(q, v), u, o;
	t.x = t.x + qw * v.x, t.y = t.y + qw * v.y, t.z = t.z + qw * v.z;
	u = cross3(q, t);
	o.x = v.x + 2.0f * u.x, o.y = v.y + 2.0f * u.y, o.z = v.z + 2.0f * u.z;
	return o;
}

static float comp(vec3 v, int k) { return k == 0 ? v.x : k == 1 ? v.y : v.z; }

/* the triangle test T for the object-space ray (o, d) */
typedef struct
{
	int kx, ky, kz;
	float Sx, Sy, Sz;
	vec3 o;
} RaySetup;

static RaySetup ray_setup(vec3 o, vec3 d)
{
	RaySetup r;
	float best = fabsf(d.x);
	int kz = 0, kx, ky;
	if (fabsf(d.y) > best)
		kz = 1, best = fabsf(d.y);
	if (fabsf(d.z) > best)
		kz = 2;
	kx = (kz + 1) % 3, ky = (kx + 1) % 3;
	if (comp(d, kz) < 0.0f)
	{
		int s = kx;
		kx = ky, ky = s;
	}
	r.kx = kx, r.ky = ky, r.kz = kz;
	r.Sx = comp(d, kx) / comp(d, kz);
	r.Sy = comp(d, ky) / comp(d, kz);
	r.Sz = 1.0f / comp(d, kz);
	r.o = o;
	return r;
}

/* test infrastructure only: the rays for which T took its fp64 branch against a casting triangle before the ray was decided (an input
 * condition of the degenerate-ray tests; no result depends on it), and those among them for which the branch turned an fp32 zero of U, V or W
 * into a number with a sign: the rays its extra precision can decide */
static _Thread_local int fp64_flag, fp64_decided_flag;
static uint64_t fp64_rays, fp64_decided_rays;

static int triangle_test(const RaySetup* r, vec3 v0, vec3 v1, vec3 v2, float tmin, float tmax)
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
		const float U32 = U, V32 = V, W32 = W;
		fp64_flag = 1;
		U = (float)((double)Cx * (double)By - (double)Cy * (double)Bx);
		V = (float)((double)Ax * (double)Cy - (double)Ay * (double)Cx);
		W = (float)((double)Bx * (double)Ay - (double)By * (double)Ax);
		if ((U32 == 0.0f && U != 0.0f) || (V32 == 0.0f && V != 0.0f) || (W32 == 0.0f && W != 0.0f))
			fp64_decided_flag = 1;
	}
	if ((U < 0.0f || V < 0.0f || W < 0.0f) && (U > 0.0f || V > 0.0f || W > 0.0f))
		return 0;
	det = (U + V) + W;
	if (det == 0.0f)
		return 0;
	T = (U * (r->Sz * comp(A, r->kz)) + V * (r->Sz * comp(B, r->kz))) + W * (r->Sz * comp(C, r->kz));
	t = T / det;
	return t > tmin && t < tmax;
}

static int draw_casts(const MeshDraw* d, uint32_t meshCount, int quality)
{
	int k, finite = finite1(d->scale);
	for (k = 0; k < 3; ++k)
		finite = finite && finite1(d->position[k]);
	for (k = 0; k < 4; ++k)
		finite = finite && finite1(d->orientation[k]);
	return d->meshIndex < meshCount && finite && d->scale > 0.0f && (quality == 0 ? d->postPass == 0u : d->postPass <= 1u);
}

/* 1 when any casting triangle passes T for the world-space ray (o, d) */
static int occluded(const Mesh* meshes, uint32_t meshCount, const uint32_t* indices, uint32_t indexCapacity, const Vertex* vertices, uint32_t vertexCapacity,
                    const MeshDraw* draws, uint32_t drawCount, vec3 o, vec3 d, float tmin, float tmax, int quality)
{
	uint32_t i, t, k;
	if (!(finite1(o.x) && finite1(o.y) && finite1(o.z) && finite1(d.x) && finite1(d.y) && finite1(d.z)))
		return 0;
	for (i = 0; i < drawCount; ++i)
	{
		const MeshDraw* dr = &draws[i];
		const Mesh* mesh;
		const MeshLod* lod;
		vec3 c, rel, ro, rd, o2, d2;
		RaySetup rs;
		if (!draw_casts(dr, meshCount, quality))
			continue;
		mesh = &meshes[dr->meshIndex];
		if (mesh->lodRT >= 8u || mesh->lodRT >= mesh->lodCount)
			continue;
		lod = &mesh->lods[mesh->lodRT];
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
			}
			if (keep && triangle_test(&rs, v[0], v[1], v[2], tmin, tmax))
				return 1;
		}
	}
	return 0;
}

static int occluded_counted(const Mesh* meshes, uint32_t meshCount, const uint32_t* indices, uint32_t indexCapacity, const Vertex* vertices,
                            uint32_t vertexCapacity, const MeshDraw* draws, uint32_t drawCount, vec3 o, vec3 d, float tmin, float tmax, int quality)
{
	int hit;
	fp64_flag = fp64_decided_flag = 0;
	hit = occluded(meshes, meshCount, indices, indexCapacity, vertices, vertexCapacity, draws, drawCount, o, d, tmin, tmax, quality);
	if (fp64_flag)
		__atomic_fetch_add(&fp64_rays, 1, __ATOMIC_RELAXED);
	if (fp64_decided_flag)
		__atomic_fetch_add(&fp64_decided_rays, 1, __ATOMIC_RELAXED);
	return hit;
}

/* the counts since the last call */
uint64_t shr_fp64_rays(void) { return __atomic_exchange_n(&fp64_rays, 0, __ATOMIC_RELAXED); }
uint64_t shr_fp64_decided_rays(void) { return __atomic_exchange_n(&fp64_decided_rays, 0, __ATOMIC_RELAXED); }

/* the rays of the full-resolution image (no checkerboard): origins / dirs are w * h * 3 floats */
void shr_rays(const ShadowData* sd, const float* depth, uint32_t w, uint32_t h, float* origins, float* dirs)
{
	uint32_t x, y;
	for (y = 0; y < h; ++y)
		for (x = 0; x < w; ++x)
		{
			vec3 o, d;
			size_t at = (size_t)y * w + x;
			pixel_ray(sd, x, y, depth[at], &o, &d);
			origins[3 * at] = o.x, origins[3 * at + 1] = o.y, origins[3 * at + 2] = o.z;
			dirs[3 * at] = d.x, dirs[3 * at + 1] = d.y, dirs[3 * at + 2] = d.z;
		}
}

/* out[i] = 0 (occluded) or 255 for n given rays */
void shr_trace(const Mesh* meshes, uint32_t meshCount, const uint32_t* indices, uint32_t indexCapacity, const Vertex* vertices, uint32_t vertexCapacity,
               const MeshDraw* draws, uint32_t drawCount, const float* origins, const float* dirs, uint64_t n, float tmin, float tmax, int quality, uint8_t* out)
{
	uint64_t i;
	for (i = 0; i < n; ++i)
	{
		vec3 o = { origins[3 * i], origins[3 * i + 1], origins[3 * i + 2] }, d = { dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2] };
		out[i] = occluded_counted(meshes, meshCount, indices, indexCapacity, vertices, vertexCapacity, draws, drawCount, o, d, tmin, tmax, quality) ? 0 : 255;
	}
}

/* the pass: shadow.comp.glsl:125-161 over W' x h invocations, in place in `shadow` (w * h bytes; texels no invocation owns keep their bytes) */
void shr_shadow_trace(const ShadowData* sd, const Mesh* meshes, uint32_t meshCount, const uint32_t* indices, uint32_t indexCapacity, const Vertex* vertices,
                      uint32_t vertexCapacity, const MeshDraw* draws, uint32_t drawCount, const float* depth, uint8_t* shadow, uint32_t w, uint32_t h, int quality)
{
	uint32_t gx, gy, wi = sd->checkerboard > 0 ? (w + 1u) / 2u : w;
	for (gy = 0; gy < h; ++gy)
		for (gx = 0; gx < wi; ++gx)
		{
			int64_t px = gx;
			vec3 o, d;
			float z;
			if (sd->checkerboard > 0)
				px = px * 2 + (((int32_t)gy ^ sd->checkerboard) & 1);
			z = px < (int64_t)w ? depth[(size_t)gy * w + (size_t)px] : 0.0f; /* a fetch outside the image returns 0 */
			pixel_ray(sd, (uint32_t)px, gy, z, &o, &d);
			if (px < (int64_t)w) /* a store outside the image is dropped */
				shadow[(size_t)gy * w + (size_t)px] =
				    occluded_counted(meshes, meshCount, indices, indexCapacity, vertices, vertexCapacity, draws, drawCount, o, d, 1e-2f, 1e3f, quality) ? 0 : 255;
		}
}
