"""ctypes loader of tests/raster_clip_ref.c, the CPU reference of both depth rasterisers with NV_OPT_RASTER_NEAR_CLIP (test infrastructure).

`load(directory)` compiles it there with gcc and raster_ref.c's flags and returns a ClipLib; `ClipLib.cluster(near_clip)` offers
RasterRef.raster's signature (so raster_ref.oracle_frames(..., rref=) runs the closed loop with it), `ClipLib.indexed(near_clip)`
IndexedRef.raster's (raster_indexed_ref.oracle_frames_classic(..., iref=))."""
import ctypes as C
import os
import subprocess

import numpy as np

import raster_ref as RR
from niagara_amd import layouts as L

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "raster_clip_ref.c")

# stats4: per triangle with inside and outside vertices
CROSSING, CLIPPED, REFUSED_RULE, REFUSED_VERTEX = range(4)


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class ClusterClipRef:
    def __init__(self, lib, near_clip):
        self.lib, self.near_clip = lib, int(near_clip)
        self.stats = np.zeros(4, np.uint64)  # accumulated over the calls

    def raster(self, g, commands, draws, meshlets, data, vertices, cib, cc4, width, height, depth=None, visibility=False):
        """RasterRef.raster with the near-plane rule: (depth fp32 (height, width), visibility u64 or None, totals4)"""
        d = np.zeros((height, width), np.float32) if depth is None else np.ascontiguousarray(depth, np.float32).copy()
        vis = np.zeros((height, width), np.uint64) if visibility else None
        tot = np.zeros(4, np.uint64)
        self.lib.rc_rasterdepth(_p(g), _p(commands), _p(draws), _p(meshlets), _p(data), _p(vertices), _p(cib), _p(cc4), _p(d), C.c_uint32(width),
                                C.c_uint32(height), _p(vis), _p(tot), C.c_int(self.near_clip), _p(self.stats))
        return d, vis, tot


class IndexedClipRef:
    def __init__(self, lib, near_clip):
        self.lib, self.near_clip = lib, int(near_clip)
        self.stats = np.zeros(4, np.uint64)

    def raster(self, g, commands, count, draws, indices, vertices, width, height, depth=None, draw_count=None, index_capacity=None,
               vertex_capacity=None):
        """IndexedRef.raster with the near-plane rule: (depth fp32 (height, width), totals4)"""
        d = np.zeros((height, width), np.float32) if depth is None else np.ascontiguousarray(depth, np.float32).copy()
        tot = np.zeros(4, np.uint64)
        cnt = np.array([int(count)], np.uint32)
        commands = np.ascontiguousarray(commands, L.DRAWCMD)
        ind = np.ascontiguousarray(indices, np.uint32)
        self.lib.rc_rasterdepth_indexed(_p(g), _p(commands), _p(cnt), _p(draws), C.c_uint32(len(draws) if draw_count is None else draw_count),
                                        _p(ind if len(ind) else np.zeros(1, np.uint32)),
                                        C.c_uint32(len(ind) if index_capacity is None else index_capacity),
                                        _p(vertices if len(vertices) else np.zeros(1, L.VERTEX)),
                                        C.c_uint32(len(vertices) if vertex_capacity is None else vertex_capacity), _p(d), C.c_uint32(width),
                                        C.c_uint32(height), _p(tot), C.c_int(self.near_clip), _p(self.stats))
        return d, tot


class ClipLib:
    def __init__(self, so):
        self.lib = C.CDLL(so)
        self.lib.rc_rasterdepth.restype = None
        self.lib.rc_rasterdepth_indexed.restype = None

    def cluster(self, near_clip=1):
        return ClusterClipRef(self.lib, near_clip)

    def indexed(self, near_clip=1):
        return IndexedClipRef(self.lib, near_clip)


def load(directory):
    so = os.path.join(str(directory), "libraster_clip_ref.so")
    if not os.path.exists(so):
        subprocess.check_call(["gcc"] + RR.FLAGS + ["-Wall", "-shared", "-fPIC", "-I", HERE, "-o", so, SRC, "-lm"])
    return ClipLib(so)


def crossing_triangles(rref, s):
    """from RasterRef.vertices: how many triangles of the cluster scene `s` (RR.mesh_scene's dict) have both an inside vertex
    (clip w > 0 and z <= 1, i.e. clip.z <= clip.w) and an outside one"""
    vx = rref.vertices(*RR.raster_args(s))
    d8 = s["data"].view(np.uint8)
    n = 0
    for k in range(int(s["cc4"][2]) * 256):
        ci = int(s["cib"][k])
        if ci == 0xffffffff:
            continue
        cmd = s["commands"][ci & 0xffffff]
        m = s["meshlets"][int(cmd["taskOffset"]) + (ci >> 24)]
        vc, tc = int(m["vertexCount"]), min(int(m["triangleCount"]), 96)
        io = (int(m["dataOffset"]) + ((vc + 1) // 2 if m["shortRefs"] == 1 else vc)) * 4
        idx = d8[io:io + 3 * tc].reshape(-1, 3).astype(np.int64)
        idx = idx[(idx < min(vc, 64)).all(axis=1)]
        with np.errstate(invalid="ignore"):
            inside = (vx[k][:, 2] > 0) & (vx[k][:, 3] <= 1)
        t = inside[idx]
        n += int((t.any(axis=1) & ~t.all(axis=1)).sum())
    return n
