// rtbuild.cpp — the host side of the ray-traced shadow pass: nv_rt_scene_build writes the scene blob rtmath.h's traversal
// walks (one BLAS per mesh with triangles, one TLAS over the casting draws, both binary BVHs in depth-first preorder with skip links),
// nv_rt_scene_validate makes a blob safe to walk, nv_rt_scene_trace_host walks it on the CPU.  No device work, no context: niagara builds its
// BLAS / TLAS at load time too (src/scenert.cpp).  Plain C++, -ffp-contract=off: the host traversal computes the kernel's bits.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "../../include/niagara_vis.h"
#include "rtmath.h"

namespace
{

using namespace nv;

static_assert(sizeof(RtHeader) == 64 && sizeof(RtBlas) == 32 && sizeof(RtNode) == 32 && sizeof(RtInstance) == 64 && sizeof(RtF4) == 16, "blob records");

float half_to_float(uint32_t h) // exact
{
	const uint32_t s = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 1023u;
	if (e == 0)
	{
		const float v = (float)m * 5.9604644775390625e-8f;
		return s ? -v : v;
	}
	const uint32_t bits = s | (e == 31u ? 0x7f800000u | m << 13 : (e + 112u) << 23 | m << 13);
	float v;
	memcpy(&v, &bits, 4);
	return v;
}

struct Box
{
	float lo[3], hi[3];
};

Box box_empty()
{
	return Box{ { INFINITY, INFINITY, INFINITY }, { -INFINITY, -INFINITY, -INFINITY } };
}

void box_add(Box& b, const Box& o)
{
	for (int k = 0; k < 3; ++k)
	{
		b.lo[k] = o.lo[k] < b.lo[k] ? o.lo[k] : b.lo[k];
		b.hi[k] = o.hi[k] > b.hi[k] ? o.hi[k] : b.hi[k];
	}
}

// the sort key of a primitive along an axis: the middle of its box (0 for a box that is not finite: it is never rejected, where it sorts is free)
float box_mid(const Box& b, int k)
{
	const float m = b.lo[k] * 0.5f + b.hi[k] * 0.5f;
	return rt_finite(m) ? m : 0.0f;
}

// Median split of the primitives order[begin, end) on the longest axis of their middles, emitted in depth-first preorder; a node's skip is the
// index behind its subtree.  The order is total (key, then primitive index): the same inputs give the same bytes.
void build_nodes(std::vector<RtNode>& nodes, std::vector<uint32_t>& order, const std::vector<Box>& boxes, uint32_t begin, uint32_t end, uint32_t leafMax,
                 uint32_t base)
{
	const uint32_t self = (uint32_t)nodes.size();
	nodes.push_back(RtNode());
	Box b = box_empty();
	float mlo[3] = { INFINITY, INFINITY, INFINITY }, mhi[3] = { -INFINITY, -INFINITY, -INFINITY };
	for (uint32_t i = begin; i < end; ++i)
	{
		box_add(b, boxes[order[i]]);
		for (int k = 0; k < 3; ++k)
		{
			const float m = box_mid(boxes[order[i]], k);
			mlo[k] = m < mlo[k] ? m : mlo[k];
			mhi[k] = m > mhi[k] ? m : mhi[k];
		}
	}
	uint32_t leaf = 0;
	if (end - begin <= leafMax)
		leaf = (end - begin) << RT_LEAF_SHIFT | begin;
	else
	{
		int axis = 0;
		if (mhi[1] - mlo[1] > mhi[axis] - mlo[axis])
			axis = 1;
		if (mhi[2] - mlo[2] > mhi[axis] - mlo[axis])
			axis = 2;
		const uint32_t mid = begin + (end - begin) / 2u;
		std::sort(order.begin() + begin, order.begin() + end, [&](uint32_t l, uint32_t r) {
			const float a = box_mid(boxes[l], axis), c = box_mid(boxes[r], axis);
			return a < c || (a == c && l < r);
		});
		build_nodes(nodes, order, boxes, begin, mid, leafMax, base);
		build_nodes(nodes, order, boxes, mid, end, leafMax, base);
	}
	RtNode& n = nodes[self];
	for (int k = 0; k < 3; ++k)
		n.lo[k] = b.lo[k], n.hi[k] = b.hi[k];
	n.skip = (uint32_t)nodes.size() - base;
	n.leaf = leaf;
}

struct Tri
{
	float v[3][3];
};

// the kept triangles of meshes[mi].lods[lodRT] (the rule of include/niagara_vis.h)
void mesh_triangles(const NvMesh& mesh, const uint32_t* indices, uint32_t indexCapacity, const NvVertex* vertices, uint32_t vertexCapacity, std::vector<Tri>& out)
{
	out.clear();
	if (mesh.lodRT >= NV_MAX_LODS || mesh.lodRT >= mesh.lodCount)
		return;
	const NvMeshLod& lod = mesh.lods[mesh.lodRT];
	for (uint32_t t = 0; t < lod.indexCount / 3u; ++t)
	{
		Tri tri;
		bool keep = true;
		for (uint32_t k = 0; k < 3u && keep; ++k)
		{
			const uint64_t at = (uint64_t)lod.indexOffset + 3ull * t + k;
			if (at >= indexCapacity)
			{
				keep = false;
				break;
			}
			const uint64_t corner = (uint64_t)mesh.vertexOffset + indices[at];
			if (corner >= vertexCapacity)
			{
				keep = false;
				break;
			}
			const NvVertex& v = vertices[corner];
			tri.v[k][0] = half_to_float(v.vx), tri.v[k][1] = half_to_float(v.vy), tri.v[k][2] = half_to_float(v.vz);
		}
		if (keep)
			out.push_back(tri);
	}
}

bool draw_casts(const NvMeshDraw& d, uint32_t meshCount)
{
	bool finite = rt_finite(d.scale);
	for (int k = 0; k < 3; ++k)
		finite = finite && rt_finite(d.position[k]);
	for (int k = 0; k < 4; ++k)
		finite = finite && rt_finite(d.orientation[k]);
	return d.meshIndex < meshCount && finite && d.scale > 0.0f && d.postPass <= 1u;
}

float round_down(double v)
{
	float f = (float)v;
	return (double)f > v ? nextafterf(f, -INFINITY) : f;
}
float round_up(double v)
{
	float f = (float)v;
	return (double)f < v ? nextafterf(f, INFINITY) : f;
}

// The padded world box of an instance whose BLAS root box is `root` (DESIGN.md §4.16 "the TLAS box").  The object-space ray is
// L (x - p), L = M / s with M the matrix of rotateQuat(., conj(q)) (any finite q, unit or not), so the instance occupies p + s M^-1 (box).
// Static padding cB + cO max|p| is added here, the traversal adds padOrigin max|o| with padOrigin >= cO.  An instance whose map is singular
// or so ill-conditioned that cO would exceed 2^-10 gets the infinite box: it is never rejected.  All of it in fp64, rounded outward.
Box instance_box(const NvMeshDraw& d, const Box& root, float maxAbs, double* cO_)
{
	const Box everything = { { -INFINITY, -INFINITY, -INFINITY }, { INFINITY, INFINITY, INFINITY } };
	*cO_ = 0.0;
	const double x = -(double)d.orientation[0], y = -(double)d.orientation[1], z = -(double)d.orientation[2], w = d.orientation[3], s = d.scale;
	// v + 2 c x (c x v + w v) = (I + 2 (C C + w C)) v, C = [c]x
	const double C[3][3] = { { 0, -z, y }, { z, 0, -x }, { -y, x, 0 } };
	double M[3][3];
	for (int r = 0; r < 3; ++r)
		for (int c = 0; c < 3; ++c)
		{
			double cc = 0;
			for (int k = 0; k < 3; ++k)
				cc += C[r][k] * C[k][c];
			M[r][c] = (r == c ? 1.0 : 0.0) + 2.0 * (cc + w * C[r][c]);
		}
	const double det = M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
	                   M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
	if (!(fabs(det) > 0.0) || !(fabs(det) < INFINITY))
		return everything;
	double I[3][3];
	for (int r = 0; r < 3; ++r)
		for (int c = 0; c < 3; ++c)
		{
			const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3; // cofactor of (c, r)
			I[r][c] = (M[r1][c1] * M[r2][c2] - M[r1][c2] * M[r2][c1]) / det;
		}
	double nM = 0, nI = 0; // infinity norms
	for (int r = 0; r < 3; ++r)
	{
		nM = std::max(nM, fabs(M[r][0]) + fabs(M[r][1]) + fabs(M[r][2]));
		nI = std::max(nI, fabs(I[r][0]) + fabs(I[r][1]) + fabs(I[r][2]));
	}
	const double Qa = fabs(x) + fabs(y) + fabs(z), rotAbs = 1.0 + 2.0 * Qa * (Qa + fabs(w)), kappa = nM * nI, u = (double)RT_U, K = (double)RT_PAD_K;
	const double cO = u * (K * kappa + 16.0 * rotAbs * nI * (1.0 + kappa));
	const double cB = u * s * (double)maxAbs * nI * (K + 16.0 * rotAbs * nI);
	if (!(cO <= 0.0009765625) || !(cB < INFINITY))
		return everything;
	const double pmax = std::max(std::max(fabs((double)d.position[0]), fabs((double)d.position[1])), fabs((double)d.position[2]));
	const double pad = (cB + cO * pmax) * 1.0000001;
	double lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
	for (int corner = 0; corner < 8; ++corner)
	{
		const double c[3] = { corner & 1 ? root.hi[0] : root.lo[0], corner & 2 ? root.hi[1] : root.lo[1], corner & 4 ? root.hi[2] : root.lo[2] };
		for (int r = 0; r < 3; ++r)
		{
			const double v = (double)d.position[r] + s * ((I[r][0] * c[0] + I[r][1] * c[1]) + I[r][2] * c[2]);
			lo[r] = std::min(lo[r], v);
			hi[r] = std::max(hi[r], v);
		}
	}
	Box b;
	for (int r = 0; r < 3; ++r)
	{
		// the fp64 evaluation above errs by a few 2^-53 of its terms: far inside the padding's slack (RT_PAD_K is > 2 x what the analysis needs)
		b.lo[r] = round_down(lo[r] - pad), b.hi[r] = round_up(hi[r] + pad);
		if (!(b.lo[r] <= b.hi[r])) // NaN
			return everything;
	}
	*cO_ = cO;
	return b;
}

uint64_t align16(uint64_t v) { return (v + 15u) & ~(uint64_t)15u; }

const RtHeader* checked_header(const void* blob, uint64_t bytes)
{
	if (!blob || bytes < sizeof(RtHeader) || (reinterpret_cast<uintptr_t>(blob) & 15u))
		return nullptr;
	const RtHeader* h = static_cast<const RtHeader*>(blob);
	if (h->magic != RT_MAGIC || h->version != RT_VERSION || h->bytes != bytes)
		return nullptr;
	// the sections lie in this order, aligned, inside the blob
	const uint64_t sizes[5] = { (uint64_t)h->meshCount * sizeof(RtBlas), (uint64_t)h->tlasNodes * sizeof(RtNode), (uint64_t)h->instances * sizeof(RtInstance),
		                        (uint64_t)h->blasNodes * sizeof(RtNode), (uint64_t)h->triangles * 48u };
	const uint32_t offs[5] = { h->tableOff, h->tlasOff, h->instOff, h->blasOff, h->triOff };
	uint64_t at = sizeof(RtHeader);
	for (int i = 0; i < 5; ++i)
	{
		if ((offs[i] & 15u) || offs[i] < at || (uint64_t)offs[i] + sizes[i] > bytes)
			return nullptr;
		at = (uint64_t)offs[i] + sizes[i];
	}
	return h;
}

} // namespace

extern "C" {

int nv_rt_scene_build(const NvMesh* meshes, uint32_t meshCount, const uint32_t* indices, uint32_t indexCapacity, const NvVertex* vertices,
                      uint32_t vertexCapacity, const NvMeshDraw* draws, uint32_t drawCount, void* out, uint64_t* bytes)
{
	if (!bytes || (meshCount && !meshes) || (indexCapacity && !indices) || (vertexCapacity && !vertices) || (drawCount && !draws) ||
	    (reinterpret_cast<uintptr_t>(out) & 15u))
		return NV_EINVAL;
	try
	{
		std::vector<RtBlas> table(meshCount);
		std::vector<RtNode> blasNodes, tlasNodes;
		std::vector<RtF4> tris;
		std::vector<Box> roots(meshCount);
		std::vector<Tri> meshTris;
		std::vector<Box> boxes;
		std::vector<uint32_t> order;
		for (uint32_t mi = 0; mi < meshCount; ++mi)
		{
			RtBlas& e = table[mi];
			memset(&e, 0, sizeof(e));
			mesh_triangles(meshes[mi], indices, indexCapacity, vertices, vertexCapacity, meshTris);
			if (meshTris.empty())
				continue;
			if (meshTris.size() > RT_LEAF_FIRST || tris.size() / 3u + meshTris.size() > RT_LEAF_FIRST)
				return NV_EINVAL;
			boxes.resize(meshTris.size());
			order.resize(meshTris.size());
			float maxAbs = 0.0f, maxExtent = 0.0f;
			for (size_t t = 0; t < meshTris.size(); ++t)
			{
				Box b = box_empty();
				for (int c = 0; c < 3; ++c)
					for (int k = 0; k < 3; ++k)
					{
						const float v = meshTris[t].v[c][k]; // (a NaN coordinate fails every comparison: it widens nothing, and T misses such a triangle)
						b.lo[k] = v < b.lo[k] ? v : b.lo[k];
						b.hi[k] = v > b.hi[k] ? v : b.hi[k];
						maxAbs = fabsf(v) > maxAbs ? fabsf(v) : maxAbs;
					}
				for (int k = 0; k < 3; ++k)
					maxExtent = b.hi[k] - b.lo[k] > maxExtent ? b.hi[k] - b.lo[k] : maxExtent;
				boxes[t] = b;
				order[t] = (uint32_t)t;
			}
			e.nodeFirst = (uint32_t)blasNodes.size();
			e.triFirst = (uint32_t)(tris.size() / 3u);
			e.triCount = (uint32_t)meshTris.size();
			e.maxAbs = maxAbs;
			e.maxExtent = maxExtent;
			build_nodes(blasNodes, order, boxes, 0, e.triCount, RT_LEAF_MAX, e.nodeFirst);
			e.nodeCount = (uint32_t)blasNodes.size() - e.nodeFirst;
			roots[mi] = Box{ { blasNodes[e.nodeFirst].lo[0], blasNodes[e.nodeFirst].lo[1], blasNodes[e.nodeFirst].lo[2] },
				             { blasNodes[e.nodeFirst].hi[0], blasNodes[e.nodeFirst].hi[1], blasNodes[e.nodeFirst].hi[2] } };
			for (uint32_t t = 0; t < e.triCount; ++t) // leaf order
				for (int c = 0; c < 3; ++c)
					tris.push_back(RtF4{ meshTris[order[t]].v[c][0], meshTris[order[t]].v[c][1], meshTris[order[t]].v[c][2], 0.0f });
		}
		std::vector<RtInstance> instances;
		boxes.clear();
		double cOmax = (double)RT_PAD_K * (double)RT_U;
		for (uint32_t i = 0; i < drawCount; ++i)
		{
			const NvMeshDraw& d = draws[i];
			if (!draw_casts(d, meshCount) || table[d.meshIndex].nodeCount == 0)
				continue;
			RtInstance in;
			memset(&in, 0, sizeof(in));
			memcpy(in.position, d.position, 12);
			in.scale = d.scale;
			memcpy(in.orientation, d.orientation, 16);
			in.drawId = i, in.postPass = d.postPass, in.blas = d.meshIndex;
			double cO;
			boxes.push_back(instance_box(d, roots[d.meshIndex], table[d.meshIndex].maxAbs, &cO));
			cOmax = cO > cOmax ? cO : cOmax;
			instances.push_back(in);
		}
		if (instances.size() > RT_LEAF_FIRST || blasNodes.size() > 0x7fffffffu)
			return NV_EINVAL;
		order.resize(instances.size());
		for (size_t i = 0; i < order.size(); ++i)
			order[i] = (uint32_t)i;
		if (!instances.empty())
			build_nodes(tlasNodes, order, boxes, 0, (uint32_t)instances.size(), 1u, 0u);

		RtHeader h;
		memset(&h, 0, sizeof(h));
		h.magic = RT_MAGIC, h.version = RT_VERSION;
		h.meshCount = meshCount, h.tlasNodes = (uint32_t)tlasNodes.size(), h.instances = (uint32_t)instances.size();
		h.blasNodes = (uint32_t)blasNodes.size(), h.triangles = (uint32_t)(tris.size() / 3u), h.drawCount = drawCount;
		h.padOrigin = round_up(cOmax * 1.0000001);
		uint64_t at = sizeof(RtHeader);
		const uint64_t tableOff = at;
		at = align16(at + table.size() * sizeof(RtBlas));
		const uint64_t tlasOff = at;
		at = align16(at + tlasNodes.size() * sizeof(RtNode));
		const uint64_t instOff = at;
		at = align16(at + instances.size() * sizeof(RtInstance));
		const uint64_t blasOff = at;
		at = align16(at + blasNodes.size() * sizeof(RtNode));
		const uint64_t triOff = at;
		at = align16(at + tris.size() * sizeof(RtF4));
		if (at > 0xffffffffull)
			return NV_EINVAL;
		h.tableOff = (uint32_t)tableOff, h.tlasOff = (uint32_t)tlasOff, h.instOff = (uint32_t)instOff, h.blasOff = (uint32_t)blasOff, h.triOff = (uint32_t)triOff;
		h.bytes = (uint32_t)at;
		if (!out)
		{
			*bytes = at;
			return NV_OK;
		}
		if (*bytes < at)
			return NV_EINVAL;
		unsigned char* p = static_cast<unsigned char*>(out);
		memset(p, 0, (size_t)at);
		memcpy(p, &h, sizeof(h));
		if (!table.empty())
			memcpy(p + tableOff, table.data(), table.size() * sizeof(RtBlas));
		if (!tlasNodes.empty())
			memcpy(p + tlasOff, tlasNodes.data(), tlasNodes.size() * sizeof(RtNode));
		for (size_t i = 0; i < instances.size(); ++i) // leaf order: TLAS leaf k holds instance order[k]
			memcpy(p + instOff + i * sizeof(RtInstance), &instances[order[i]], sizeof(RtInstance));
		if (!blasNodes.empty())
			memcpy(p + blasOff, blasNodes.data(), blasNodes.size() * sizeof(RtNode));
		if (!tris.empty())
			memcpy(p + triOff, tris.data(), tris.size() * sizeof(RtF4));
		*bytes = at;
		return NV_OK;
	}
	catch (const std::bad_alloc&)
	{
		return NV_ENOMEM;
	}
}

int nv_rt_scene_validate(const void* blob, uint64_t bytes)
{
	const RtHeader* h = checked_header(blob, bytes);
	if (!h)
		return NV_EINVAL;
	const unsigned char* p = static_cast<const unsigned char*>(blob);
	const RtBlas* table = reinterpret_cast<const RtBlas*>(p + h->tableOff);
	const RtNode* tlas = reinterpret_cast<const RtNode*>(p + h->tlasOff);
	const RtInstance* inst = reinterpret_cast<const RtInstance*>(p + h->instOff);
	const RtNode* blas = reinterpret_cast<const RtNode*>(p + h->blasOff);
	for (uint32_t i = 0; i < h->tlasNodes; ++i)
	{
		const uint32_t count = tlas[i].leaf >> RT_LEAF_SHIFT, first = tlas[i].leaf & RT_LEAF_FIRST;
		if (tlas[i].skip <= i || tlas[i].skip > h->tlasNodes || (tlas[i].leaf != 0u && (count != 1u || first >= h->instances)))
			return NV_EINVAL;
	}
	for (uint32_t i = 0; i < h->instances; ++i)
		if (inst[i].blas >= h->meshCount)
			return NV_EINVAL;
	for (uint32_t m = 0; m < h->meshCount; ++m)
	{
		const RtBlas& e = table[m];
		if ((uint64_t)e.nodeFirst + e.nodeCount > h->blasNodes || (uint64_t)e.triFirst + e.triCount > h->triangles)
			return NV_EINVAL;
		for (uint32_t j = 0; j < e.nodeCount; ++j)
		{
			const RtNode& n = blas[e.nodeFirst + j];
			const uint32_t count = n.leaf >> RT_LEAF_SHIFT, first = n.leaf & RT_LEAF_FIRST;
			if (n.skip <= j || n.skip > e.nodeCount || (n.leaf != 0u && (count > RT_LEAF_MAX || (uint64_t)first + count > e.triCount)))
				return NV_EINVAL;
		}
	}
	return NV_OK;
}

int nv_rt_scene_stats(const void* blob, uint64_t bytes, NvRtSceneStats* out)
{
	if (!out || nv_rt_scene_validate(blob, bytes) != NV_OK)
		return NV_EINVAL;
	const RtHeader* h = static_cast<const RtHeader*>(blob);
	const unsigned char* p = static_cast<const unsigned char*>(blob);
	const RtBlas* table = reinterpret_cast<const RtBlas*>(p + h->tableOff);
	const RtNode* tlas = reinterpret_cast<const RtNode*>(p + h->tlasOff);
	const RtNode* blas = reinterpret_cast<const RtNode*>(p + h->blasOff);
	memset(out, 0, sizeof(*out));
	out->bytes = h->bytes, out->instances = h->instances, out->tlasNodes = h->tlasNodes, out->blasNodes = h->blasNodes, out->triangles = h->triangles;
	for (uint32_t i = 0; i < h->tlasNodes; ++i)
		if (tlas[i].leaf)
		{
			++out->tlasLeaves;
			out->tlasMaxLeaf = std::max(out->tlasMaxLeaf, tlas[i].leaf >> RT_LEAF_SHIFT);
		}
	for (uint32_t m = 0; m < h->meshCount; ++m)
		out->blasCount += table[m].nodeCount ? 1u : 0u;
	for (uint32_t i = 0; i < h->blasNodes; ++i)
		if (blas[i].leaf)
		{
			++out->blasLeaves;
			out->blasMaxLeaf = std::max(out->blasMaxLeaf, blas[i].leaf >> RT_LEAF_SHIFT);
		}
	return NV_OK;
}

int nv_rt_scene_trace_host(const void* blob, const float origin[3], const float dir[3], float tmin, float tmax, int quality)
{
	if (!blob || !origin || !dir || quality < 0 || quality > 1)
		return NV_EINVAL;
	return rt_occluded(static_cast<const unsigned char*>(blob), rt3{ origin[0], origin[1], origin[2] }, rt3{ dir[0], dir[1], dir[2] }, tmin, tmax, (uint32_t)quality)
	           ? 1
	           : 0;
}

int nv_rt_scene_trace_host_rays(const void* blob, const float* origins, const float* dirs, uint64_t count, float tmin, float tmax, int quality, uint8_t* out)
{
	if (!blob || (count && (!origins || !dirs || !out)) || quality < 0 || quality > 1)
		return NV_EINVAL;
	for (uint64_t i = 0; i < count; ++i)
		out[i] = rt_occluded(static_cast<const unsigned char*>(blob), rt3{ origins[3 * i], origins[3 * i + 1], origins[3 * i + 2] },
		                     rt3{ dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2] }, tmin, tmax, (uint32_t)quality)
		             ? 0
		             : 255;
	return NV_OK;
}

} // extern "C"
