"""ctypes loader of tests/visindexed_ref.c, the CPU reference of the visibility buffer of the indexed draws (test infrastructure,
DESIGN.md §4.23): nv_rasterdepth_indexed_visibility, nv_visibility_resolve_indexed, the word's encode / decode, and small scenes of
commands whose sizes the tests choose.

`load(directory)` compiles it there with gcc and raster_ref.c's flags and returns a VisIndexedRef."""
import ctypes as C
import os
import subprocess

import numpy as np

import raster_ref as RR
from niagara_amd import layouts as L

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "visindexed_ref.c")
SHIFT = 34
ID_MASK = (1 << SHIFT) - 1
TRI34_END = (1 << SHIFT) - 1
NO_SAMPLE = (0xFFFFFFFF, 0, 0, 0)
UNRESOLVED = (0xFFFFFFFF,) * 4


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def encode(depth_bits, tri34):
    """the word of a sample: bits(z) << 34 | (tri34 + 1)"""
    assert 0 <= depth_bits <= 0x3F800000 and 0 <= tri34 < TRI34_END
    return int(depth_bits) << SHIFT | (int(tri34) + 1)


def decode(word):
    """(depth bits, tri34) of a non-zero word"""
    word = int(word)
    return word >> SHIFT, (word & ID_MASK) - 1


class VisIndexedRef:
    def __init__(self, so):
        self.lib = C.CDLL(so)
        self.lib.vi_rasterdepth_indexed.restype = None
        self.lib.vi_resolve.restype = None

    def raster(self, g, commands, count, draws, indices, vertices, width, height, offsets, depth=None, vis=None, draw_count=None,
               index_capacity=None, vertex_capacity=None, near_clip=0):
        """(depth fp32 (height, width), visibility u64 (height, width), totals4): RI.IndexedRef.raster's arguments, `offsets` (draw_count + 1
        u64: on a shard the slice at its first draw) and `vis`, the target to load instead of a cleared one"""
        d = np.zeros((height, width), np.float32) if depth is None else np.ascontiguousarray(depth, np.float32).copy()
        v = np.zeros((height, width), np.uint64) if vis is None else np.ascontiguousarray(vis, np.uint64).copy()
        tot = np.zeros(4, np.uint64)
        cnt = np.array([int(count)], np.uint32)
        commands = np.ascontiguousarray(commands, L.DRAWCMD)
        ind = np.ascontiguousarray(indices, np.uint32)
        off = np.ascontiguousarray(offsets, np.uint64)
        n = len(draws) if draw_count is None else draw_count
        assert len(off) >= n + 1
        self.lib.vi_rasterdepth_indexed(_p(g), _p(commands), _p(cnt), _p(draws), C.c_uint32(n), _p(ind if len(ind) else np.zeros(1, np.uint32)),
                                        C.c_uint32(len(ind) if index_capacity is None else index_capacity),
                                        _p(vertices if len(vertices) else np.zeros(1, L.VERTEX)),
                                        C.c_uint32(len(vertices) if vertex_capacity is None else vertex_capacity), _p(d), C.c_uint32(width),
                                        C.c_uint32(height), _p(tot), C.c_int(int(near_clip)), _p(off), _p(v))
        return d, v, tot

    def resolve(self, cull, vis, draws, meshes, offsets, draw_count=None, mesh_count=None):
        """nv_visibility_resolve_indexed: dict(records (h * w VISINDEXEDRECORD), draw_pixels (len(draws) u32), totals (4 u64))"""
        vis = np.ascontiguousarray(vis, np.uint64).reshape(-1)
        off = np.ascontiguousarray(offsets, np.uint64)
        rec = np.zeros(len(vis), dtype=L.VISINDEXEDRECORD)
        dp = np.zeros(max(1, len(draws)), np.uint32)
        tot = np.zeros(4, np.uint64)
        self.lib.vi_resolve(_p(cull), _p(vis), C.c_uint32(len(vis)), _p(draws if len(draws) else np.zeros(1, L.MESHDRAW)),
                            C.c_uint32(len(draws) if draw_count is None else draw_count), _p(meshes if len(meshes) else np.zeros(1, L.MESH)),
                            C.c_uint32(len(meshes) if mesh_count is None else mesh_count), _p(off), _p(rec), _p(dp), _p(tot))
        return dict(records=rec, draw_pixels=dp[:len(draws)], totals=tot)


def load(directory):
    so = os.path.join(str(directory), "libvisindexed_ref.so")
    if not os.path.exists(so):
        subprocess.check_call(["gcc"] + RR.FLAGS + ["-Wall", "-shared", "-fPIC", "-I", HERE, "-o", so, SRC, "-lm"])
    return VisIndexedRef(so)


def vertices_of(positions):
    v = np.zeros(len(positions), dtype=L.VERTEX)
    hp = np.asarray(positions, np.float32).astype(np.float16)
    v["vx"], v["vy"], v["vz"] = (hp[:, k].view(np.uint16) for k in range(3))
    return v


def triangle_soup(sizes, seed, spread=(4.0, 3.0), z=(-14.0, -4.0), edge=0.6, big_every=7):
    """One draw, one single-LOD mesh and one command per entry of `sizes` (its triangle count): random counter-clockwise triangles around
    the draw's position, every `big_every`-th one several times larger (so that both the lane path and the wave path draw some of every
    command at the default small limit).  Returns dict(meshes, draws, commands, count, indices, vertices, offsets) with the offsets the
    helper's rule gives (the prefix of the sizes)."""
    rng = np.random.default_rng(seed)
    n, total = len(sizes), int(sum(sizes))
    tri = rng.normal(0, edge * 0.3, (total, 3, 3)).astype(np.float32)
    tri[:, 1, 0] += edge
    tri[:, 2, 1] += edge  # counter-clockwise seen from +z
    tri[::big_every] *= 6.0
    flip = rng.uniform(size=total) < 0.2  # some back faces: drawn by the post pass only
    tri[flip] = tri[flip][:, ::-1]
    draws = np.zeros(n, dtype=L.MESHDRAW)
    draws["position"] = np.stack([rng.uniform(-spread[0], spread[0], n), rng.uniform(-spread[1], spread[1], n), rng.uniform(z[0], z[1], n)], 1)
    draws["scale"], draws["orientation"] = 1.0, (0, 0, 0, 1)
    meshes = np.zeros(n, dtype=L.MESH)
    commands = np.zeros(n, dtype=L.DRAWCMD)
    at = 0
    for i, k in enumerate(sizes):
        draws[i]["meshIndex"] = i
        meshes[i]["radius"], meshes[i]["lodCount"], meshes[i]["vertexCount"] = 4.0, 1, 3 * k
        meshes[i]["lods"]["indexOffset"][0], meshes[i]["lods"]["indexCount"][0] = 3 * at, 3 * k
        commands[i]["drawId"], commands[i]["firstIndex"], commands[i]["indexCount"], commands[i]["instanceCount"] = i, 3 * at, 3 * k, 1
        at += k
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    return dict(meshes=meshes, draws=draws, commands=commands, count=n, indices=np.arange(3 * total, dtype=np.uint32),
                vertices=vertices_of(tri.reshape(-1, 3)), offsets=offsets)
