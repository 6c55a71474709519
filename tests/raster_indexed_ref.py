"""ctypes loader of tests/raster_indexed_ref.c, the CPU reference of nv_rasterdepth_indexed, and the indexed scenes of its tests (test
infrastructure).

`load(directory)` compiles it there with gcc and raster_ref.c's flags and returns an IndexedRef."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle
import raster_ref as RR
from niagara_amd import layouts as L

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "raster_indexed_ref.c")


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class IndexedRef:
    def __init__(self, so):
        self.lib = C.CDLL(so)
        self.lib.rr_rasterdepth_indexed.restype = None

    def raster(self, g, commands, count, draws, indices, vertices, width, height, depth=None, draw_count=None, index_capacity=None,
               vertex_capacity=None):
        """(depth fp32 (height, width), totals4).  count: dccb word 0; draw_count (maxDrawCount), index_capacity and vertex_capacity default to
        len(draws), len(indices) and len(vertices); `depth` (optional) is the target to load instead of a cleared one"""
        d = np.zeros((height, width), np.float32) if depth is None else np.ascontiguousarray(depth, np.float32).copy()
        tot = np.zeros(4, np.uint64)
        cnt = np.array([int(count)], np.uint32)
        commands = np.ascontiguousarray(commands, L.DRAWCMD)
        ind = np.ascontiguousarray(indices, np.uint32)
        self.lib.rr_rasterdepth_indexed(_p(g), _p(commands), _p(cnt), _p(draws), C.c_uint32(len(draws) if draw_count is None else draw_count),
                                        _p(ind if len(ind) else np.zeros(1, np.uint32)),
                                        C.c_uint32(len(ind) if index_capacity is None else index_capacity),
                                        _p(vertices if len(vertices) else np.zeros(1, L.VERTEX)),
                                        C.c_uint32(len(vertices) if vertex_capacity is None else vertex_capacity), _p(d), C.c_uint32(width),
                                        C.c_uint32(height), _p(tot))
        return d, tot


def load(directory):
    so = os.path.join(str(directory), "libraster_indexed_ref.so")
    if not os.path.exists(so):
        subprocess.check_call(["gcc"] + RR.FLAGS + ["-Wall", "-shared", "-fPIC", "-I", HERE, "-o", so, SRC, "-lm"])
    return IndexedRef(so)


def commands_for(index_ranges, draw_ids=None):
    """one MeshDrawCommand per (firstIndex, indexCount): instanceCount 1, vertexOffset 0, drawId = draw_ids[i] (default i)"""
    c = np.zeros(len(index_ranges), dtype=L.DRAWCMD)
    for i, (first, count) in enumerate(index_ranges):
        c[i]["drawId"] = i if draw_ids is None else draw_ids[i]
        c[i]["firstIndex"], c[i]["indexCount"], c[i]["instanceCount"] = first, count, 1
    return c


def from_mesh_scene(s, tris):
    """RR.mesh_scene's inputs as indexed draws: the triangle list as one index buffer, one command per draw over all of it"""
    ind = np.asarray(tris, np.uint32).reshape(-1)
    n = len(s["draws"])
    return dict(g=s["g"], commands=commands_for([(0, len(ind))] * n), count=n, draws=s["draws"], indices=ind, vertices=s["vertices"],
                viewport=s["viewport"])


def meshlet_triangles(meshlets, data, k):
    """global vertex ids (t, 3) of meshlet k's triangles as the mesh shader reads them; triangles naming a vertex past min(vertexCount, 64) are
    left out (the cluster path skips them too)"""
    m = meshlets[k]
    vc, tc, off = int(m["vertexCount"]), min(int(m["triangleCount"]), 96), int(m["dataOffset"])
    short = m["shortRefs"] == 1
    refs = (data.view(np.uint16)[off * 2:off * 2 + vc] if short else data[off:off + vc]).astype(np.int64) + int(m["baseVertex"])
    io = (off + ((vc + 1) // 2 if short else vc)) * 4
    idx = data.view(np.uint8)[io:io + 3 * tc].reshape(-1, 3).astype(np.int64)
    idx = idx[(idx < min(vc, 64)).all(axis=1)]
    return refs[idx]


def from_cluster_scene(s):
    """scenes.make_triangle_scene as indexed draws: per draw, every meshlet of its task commands decoded into one index range (global vertex
    ids, vertexOffset 0); also the cluster list of every one of those meshlets, for nv_rasterdepth over the same triangles"""
    draws, commands, meshlets, data = s["draws"], s["commands"], s["meshlets"], s["data"]
    per_draw = [[] for _ in range(len(draws))]
    ids = []
    for ci, c in enumerate(commands[:s["n"]]):
        for j in range(int(c["taskCount"])):
            per_draw[int(c["drawId"])].append(meshlet_triangles(meshlets, data, int(c["taskOffset"]) + j))
            ids.append(ci | j << 24)
    ranges, chunks, at = [], [], 0
    for tl in per_draw:
        t = np.concatenate(tl).reshape(-1) if tl else np.zeros(0, np.int64)
        ranges.append((at, len(t)))
        chunks.append(t)
        at += len(t)
    ind = np.concatenate(chunks).astype(np.uint32) if chunks else np.zeros(0, np.uint32)
    cc4 = np.array([len(ids), 0, 0, 0], np.uint32)
    cib = np.concatenate([np.array(ids, np.uint32), np.zeros(512, np.uint32)])
    oracle.clustersubmit(cc4, cib)
    return dict(commands=commands_for(ranges), count=len(draws), draws=draws, indices=ind, vertices=s["vertices"], cib=cib, cc4=cc4)


def kitten_geometry():
    """tests/golden/mesh/kitten.npz as an indexed mesh: fp16 vertices of its positions, its face corners' position indices"""
    k = np.load(os.path.join(HERE, "golden", "mesh", "kitten.npz"))
    pos, corners = k["positions"], k["corners"]
    v = np.zeros(len(pos), dtype=L.VERTEX)
    h = pos.astype(np.float16)
    v["vx"], v["vy"], v["vz"] = (h[:, i].view(np.uint16) for i in range(3))
    return v, corners[:, 0].astype(np.uint32), pos


def oracle_frames_classic(scene, frames, post_pass=False, iref=None):
    """VisibilityPipeline.frame(task=False) on the CPU: the oracle's drawcull(task = 0) with clusterOcclusionEnabled 0 and the reference
    indexed raster in place of the graphics passes, depthreduce between the phases.  One record per frame: per phase count4, the commands,
    dvb and depth; the pyramid."""
    meshes, draws, ind, verts = scene["meshes"], scene["draws"].copy(), scene["indices"], scene["vertices"]
    cd = scene["cull"].copy()
    cd["clusterOcclusionEnabled"] = 0
    w, h = scene["viewport"]
    oracle.assign_visibility_offsets(draws, meshes)
    dvb = np.zeros(max(1, len(draws)), np.uint32)
    pyr = oracle.Pyramid(w, h)
    depth = np.zeros((h, w), np.float32)
    out = []
    for _ in range(frames):
        rec = {}
        for name, late, pp in [("early", 0, 0), ("late", 1, 0)] + ([("post", 1, 1)] if post_pass else []):
            if name == "late":
                oracle.depthreduce(depth, pyr)
            pd = cd.copy()
            pd["clusterBackfaceEnabled"] = 1 if pp == 0 else 0
            pd["postPass"] = pp
            co, c4 = np.zeros(len(draws) + 1, dtype=L.DRAWCMD), np.zeros(4, np.uint32)
            oracle.drawcull(pd, late, 0, draws, meshes, co, c4, dvb, pyr)
            g = RR.globals_for(cd, (w, h), pp)
            depth, _ = iref.raster(g, co[:len(draws)], c4[0], draws, ind, verts, w, h, depth=None if name == "early" else depth)
            rec[name] = dict(count4=c4.copy(), commands=co[:int(c4[0])].copy(), dvb=dvb.copy(), depth=depth.copy())
        rec["pyramid"] = pyr.data.copy()
        out.append(rec)
    return out
