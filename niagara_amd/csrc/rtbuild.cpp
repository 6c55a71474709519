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
#include "rtalpha.h"
#include "rtmath.h"
#include "rttlas.h"
#include "launch.h"

namespace
{

using namespace nv;

static_assert(sizeof(TxDesc) == sizeof(NvTextureDesc) && sizeof(NvMeshDraw) == 48 && sizeof(NvMaterial) == 64, "the alpha test's records");
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

using Box = TlBox; // rttlas.h

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
	uint32_t tc[3]; // tu | tv << 16 of each corner
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
			tri.tc[k] = (uint32_t)v.tu | (uint32_t)v.tv << 16;
		}
		if (keep)
			out.push_back(tri);
	}
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

namespace nv
{

// The canonical blob — nv_rt_scene_build's section order and packing — from its parts: the BLAS side as `src` describes it, a TLAS and its
// instances.  The size protocol of nv_rt_scene_build.  nv_rt_tlas_build_host and nv_rt_scene_download (context.hip) end here, so that a host
// and a device rebuild compare with == on bytes.
int rt_pack_blob(const RtHeader& src, const RtBlas* table, const RtNode* tlas, uint32_t tlasNodes, const RtInstance* inst, uint32_t instances,
                 const RtNode* blas, const RtF4* tris, float padOrigin, uint32_t drawCount, void* out, uint64_t* bytes)
{
	RtHeader h;
	memset(&h, 0, sizeof(h));
	h.magic = RT_MAGIC, h.version = RT_VERSION;
	h.meshCount = src.meshCount, h.tlasNodes = tlasNodes, h.instances = instances;
	h.blasNodes = src.blasNodes, h.triangles = src.triangles, h.drawCount = drawCount;
	h.padOrigin = padOrigin;
	h.flags = src.flags; // the triangles are src's: what their w words mean goes with them
	const uint64_t sizes[5] = { (uint64_t)h.meshCount * sizeof(RtBlas), (uint64_t)tlasNodes * sizeof(RtNode), (uint64_t)instances * sizeof(RtInstance),
		                        (uint64_t)h.blasNodes * sizeof(RtNode), (uint64_t)h.triangles * 48u };
	const void* parts[5] = { table, tlas, inst, blas, tris };
	uint64_t offs[5], at = sizeof(RtHeader);
	for (int i = 0; i < 5; ++i)
	{
		offs[i] = at;
		at = align16(at + sizes[i]);
	}
	if (at > 0xffffffffull)
		return NV_EINVAL;
	h.tableOff = (uint32_t)offs[0], h.tlasOff = (uint32_t)offs[1], h.instOff = (uint32_t)offs[2], h.blasOff = (uint32_t)offs[3], h.triOff = (uint32_t)offs[4];
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
	for (int i = 0; i < 5; ++i)
		if (sizes[i])
			memcpy(p + offs[i], parts[i], (size_t)sizes[i]);
	*bytes = at;
	return NV_OK;
}

} // namespace nv

namespace
{

// The tree of rttlas.h by plain recursion: the sorted range [l, r] splits in front of the first string whose highest differing bit is set.
// (The device finds every inner node's range on its own from the neighbouring strings: a different algorithm for the same, unique tree.)
void tlas_emit(std::vector<RtNode>& nodes, const std::vector<uint64_t>& strings, const std::vector<Box>& leaves, uint32_t l, uint32_t r, uint32_t lefts)
{
	const uint32_t pos = tl_pos(l, lefts);
	RtNode& n = nodes[pos];
	n.skip = tl_skip(pos, l, r);
	if (l == r)
	{
		for (int k = 0; k < 3; ++k)
			n.lo[k] = leaves[l].lo[k], n.hi[k] = leaves[l].hi[k];
		n.leaf = 1u << RT_LEAF_SHIFT | l;
		return;
	}
	const uint64_t bit = 1ull << (63 - __builtin_clzll(strings[l] ^ strings[r]));
	uint32_t a = l, b = r; // strings[a] has the bit clear, strings[b] has it set
	while (b - a > 1u)
	{
		const uint32_t m = a + (b - a) / 2u;
		if (strings[m] & bit)
			b = m;
		else
			a = m;
	}
	tlas_emit(nodes, strings, leaves, l, b - 1u, lefts + 1u);
	tlas_emit(nodes, strings, leaves, b, r, lefts);
	const RtNode &cl = nodes[pos + 1u], &cr = nodes[tl_pos(b, lefts)];
	for (int k = 0; k < 3; ++k)
		n.lo[k] = tl_fmin(cl.lo[k], cr.lo[k]), n.hi[k] = tl_fmax(cl.hi[k], cr.hi[k]);
	n.leaf = 0u;
}

} // namespace

namespace
{

// a float with the bits `u`: a triangle's w word is carried, never computed with
float bits_as_float(uint32_t u)
{
	float f;
	memcpy(&f, &u, 4);
	return f;
}

// nv_rt_scene_build (texcoords false: w = 0, flags = 0) and nv_rt_scene_build_textured (the corners' packed texcoords in w, RT_FLAG_TEXCOORDS)
int scene_build(const NvMesh* meshes, uint32_t meshCount, const uint32_t* indices, uint32_t indexCapacity, const NvVertex* vertices, uint32_t vertexCapacity,
                const NvMeshDraw* draws, uint32_t drawCount, void* out, uint64_t* bytes, bool texcoords)
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
					tris.push_back(RtF4{ meshTris[order[t]].v[c][0], meshTris[order[t]].v[c][1], meshTris[order[t]].v[c][2],
						                 texcoords ? bits_as_float(meshTris[order[t]].tc[c]) : 0.0f });
		}
		std::vector<RtInstance> instances;
		boxes.clear();
		double cOmax = (double)RT_PAD_K * (double)RT_U;
		for (uint32_t i = 0; i < drawCount; ++i)
		{
			const NvMeshDraw& d = draws[i];
			if (!tl_draw_casts(d, meshCount) || table[d.meshIndex].nodeCount == 0)
				continue;
			const RtInstance in = tl_instance(d, i);
			double cO;
			boxes.push_back(tl_instance_box(d, roots[d.meshIndex], table[d.meshIndex].maxAbs, &cO));
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
		h.padOrigin = tl_pad_origin(cOmax);
		h.flags = texcoords ? RT_FLAG_TEXCOORDS : 0u;
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

} // namespace

extern "C" {

int nv_rt_scene_build(const NvMesh* meshes, uint32_t meshCount, const uint32_t* indices, uint32_t indexCapacity, const NvVertex* vertices,
                      uint32_t vertexCapacity, const NvMeshDraw* draws, uint32_t drawCount, void* out, uint64_t* bytes)
{
	return scene_build(meshes, meshCount, indices, indexCapacity, vertices, vertexCapacity, draws, drawCount, out, bytes, false);
}

int nv_rt_scene_build_textured(const NvMesh* meshes, uint32_t meshCount, const uint32_t* indices, uint32_t indexCapacity, const NvVertex* vertices,
                               uint32_t vertexCapacity, const NvMeshDraw* draws, uint32_t drawCount, void* out, uint64_t* bytes)
{
	return scene_build(meshes, meshCount, indices, indexCapacity, vertices, vertexCapacity, draws, drawCount, out, bytes, true);
}

int nv_rt_scene_validate(const void* blob, uint64_t bytes)
{
	const RtHeader* h = checked_header(blob, bytes);
	if (!h || (h->flags & ~RT_FLAGS_KNOWN)) // a flag this library does not know changes what the bytes mean: refused
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

int nv_rt_tlas_build_host(const void* blob, uint64_t blobBytes, const NvMeshDraw* draws, uint32_t drawCount, void* out, uint64_t* bytes)
{
	if (!bytes || (drawCount && !draws) || (reinterpret_cast<uintptr_t>(out) & 15u) || drawCount > RT_LEAF_FIRST ||
	    nv_rt_scene_validate(blob, blobBytes) != NV_OK)
		return NV_EINVAL;
	try
	{
		const RtHeader* h = static_cast<const RtHeader*>(blob);
		const unsigned char* p = static_cast<const unsigned char*>(blob);
		const RtBlas* table = reinterpret_cast<const RtBlas*>(p + h->tableOff);
		const RtNode* blas = reinterpret_cast<const RtNode*>(p + h->blasOff);
		struct Caster
		{
			uint32_t key, draw;
			Box box;
		};
		std::vector<Caster> casters;
		double cOmax = 0.0;
		float midLo[3] = { INFINITY, INFINITY, INFINITY }, midHi[3] = { -INFINITY, -INFINITY, -INFINITY };
		for (uint32_t i = 0; i < drawCount; ++i)
		{
			const NvMeshDraw& d = draws[i];
			if (!tl_draw_casts(d, h->meshCount) || table[d.meshIndex].nodeCount == 0)
				continue;
			const RtNode& rn = blas[table[d.meshIndex].nodeFirst];
			const Box root = { { rn.lo[0], rn.lo[1], rn.lo[2] }, { rn.hi[0], rn.hi[1], rn.hi[2] } };
			double cO;
			Caster c;
			c.key = 0u, c.draw = i;
			c.box = tl_instance_box(d, root, table[d.meshIndex].maxAbs, &cO);
			cOmax = cO > cOmax ? cO : cOmax;
			for (int k = 0; k < 3; ++k)
			{
				const float m = tl_mid(c.box.lo[k], c.box.hi[k]);
				midLo[k] = tl_fmin(midLo[k], m), midHi[k] = tl_fmax(midHi[k], m);
			}
			casters.push_back(c);
		}
		for (Caster& c : casters)
			c.key = tl_key(c.box, midLo, midHi);
		std::stable_sort(casters.begin(), casters.end(), [](const Caster& a, const Caster& b) { return a.key < b.key; }); // (key, drawId)
		const uint32_t n = (uint32_t)casters.size();
		std::vector<RtNode> nodes(n ? 2u * (size_t)n - 1u : 0u);
		std::vector<RtInstance> instances(n);
		std::vector<uint64_t> strings(n);
		std::vector<Box> leaves(n);
		for (uint32_t k = 0; k < n; ++k)
		{
			strings[k] = tl_string(casters[k].key, k);
			leaves[k] = casters[k].box;
			instances[k] = tl_instance(draws[casters[k].draw], casters[k].draw);
		}
		if (n)
			tlas_emit(nodes, strings, leaves, 0u, n - 1u, 0u);
		return rt_pack_blob(*h, table, nodes.data(), (uint32_t)nodes.size(), instances.data(), n, blas, reinterpret_cast<const RtF4*>(p + h->triOff),
		                    tl_pad_origin(cOmax), drawCount, out, bytes);
	}
	catch (const std::bad_alloc&)
	{
		return NV_ENOMEM;
	}
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

int nv_rt_scene_trace_host_textured_rays(const void* blob, const float* origins, const float* dirs, uint64_t count, float tmin, float tmax, int quality,
                                         const NvMeshDraw* draws, uint32_t drawCount, const NvMaterial* materials, uint32_t materialCount,
                                         const NvTextureDesc* textures, uint32_t textureCount, const uint32_t* texels, uint64_t texelWords, uint8_t* out)
{
	if (!blob || (count && (!origins || !dirs || !out)) || quality < 0 || quality > 1 || (drawCount && !draws) || (materialCount && !materials) ||
	    (textureCount && !textures) || (texelWords && !texels) || !(static_cast<const RtHeader*>(blob)->flags & RT_FLAG_TEXCOORDS))
		return NV_EINVAL;
	if (quality == 0)
		return nv_rt_scene_trace_host_rays(blob, origins, dirs, count, tmin, tmax, 0, out);
	RtAlphaInputs<TxDecoded> in;
	in.draws = draws, in.materials = materials, in.textures = reinterpret_cast<const TxDesc*>(textures), in.data = texels;
	in.extent = texelWords, in.drawCount = drawCount, in.materialCount = materialCount, in.textureCount = textureCount;
	for (uint64_t i = 0; i < count; ++i)
		out[i] = rt_occluded_alpha(static_cast<const unsigned char*>(blob), in, rt3{ origins[3 * i], origins[3 * i + 1], origins[3 * i + 2] },
		                           rt3{ dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2] }, tmin, tmax)
		             ? 0
		             : 255;
	return NV_OK;
}

int nv_rt_alpha_sample_host(const NvTextureDesc* desc, const uint32_t* texels, uint64_t texelWords, const float* uv, uint64_t count, float* fourTap,
                            float* sampler)
{
	if (!desc || !texels || (count && (!uv || !fourTap || !sampler)))
		return NV_EINVAL;
	TxDesc t;
	memcpy(&t, desc, sizeof(t));
	if (!tx_desc_ok(t, texelWords))
		return NV_EINVAL;
	for (uint64_t i = 0; i < count; ++i)
	{
		fourTap[i] = TxDecoded::alpha_lod0(texels, t, uv[2 * i], uv[2 * i + 1]);
		sampler[i] = tx_sample_lod0(texels, t, uv[2 * i], uv[2 * i + 1]).w;
	}
	return NV_OK;
}

} // extern "C"
