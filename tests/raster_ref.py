"""ctypes loader of tests/raster_ref.c, the CPU reference of nv_rasterdepth (test infrastructure).

`load(directory)` compiles it there with gcc and the oracle's floating-point flags and returns a RasterRef; each test module's
session fixture passes pytest's tmp dir."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle
from niagara_amd import layouts as L

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "raster_ref.c")
FLAGS = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-msse2", "-mfpmath=sse"]  # oracle/Makefile FPFLAGS


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class RasterRef:
    def __init__(self, so):
        self.lib = C.CDLL(so)
        self.lib.rr_vertices.restype = None
        self.lib.rr_rasterdepth.restype = None

    def vertices(self, g, commands, draws, meshlets, data, vertices, cib, cc4):
        """per slot of the grid: 64 x {sx, sy, clip w, z}"""
        slots = max(int(cc4[2]) * 256, 1)
        out = np.zeros((slots, 64, 4), np.float32)
        self.lib.rr_vertices(_p(g), _p(commands), _p(draws), _p(meshlets), _p(data), _p(vertices), _p(cib), _p(cc4), _p(out), C.c_uint32(slots))
        return out

    def raster(self, g, commands, draws, meshlets, data, vertices, cib, cc4, width, height, depth=None, visibility=False):
        """(depth fp32 (height, width), visibility u64 or None, totals4); `depth` (optional) is the target to load instead of a cleared one"""
        d = np.zeros((height, width), np.float32) if depth is None else np.ascontiguousarray(depth, np.float32).copy()
        vis = np.zeros((height, width), np.uint64) if visibility else None
        tot = np.zeros(4, np.uint64)
        self.lib.rr_rasterdepth(_p(g), _p(commands), _p(draws), _p(meshlets), _p(data), _p(vertices), _p(cib), _p(cc4), _p(d), C.c_uint32(width),
                                C.c_uint32(height), _p(vis), _p(tot))
        return d, vis, tot


def load(directory):
    so = os.path.join(str(directory), "libraster_ref.so")
    if not os.path.exists(so):
        subprocess.check_call(["gcc"] + FLAGS + ["-Wall", "-shared", "-fPIC", "-o", so, SRC, "-lm"])
    return RasterRef(so)


def globals_for(cd, viewport, post_pass=0):
    from niagara_amd import synth
    pd = cd.copy()
    pd["postPass"] = post_pass
    return synth.make_globals(pd, viewport)


def oracle_frames(scene, frames, post_pass=False, rref=None):
    """VisibilityPipeline.frame on the CPU: the oracle chain (drawcull TASK -> tasksubmit -> clustercull -> clustersubmit, depthreduce)
    with the reference raster in place of the graphics passes.  Returns one record per frame: per phase the buffers the GPU leaves
    (count4, commands, cc4, cib, dvb, mvb, depth) and the pyramid."""
    meshes, meshlets, draws, cd = scene["meshes"], scene["meshlets"], scene["draws"].copy(), scene["cull"]
    w, h = scene["viewport"]
    slots, _ = oracle.assign_visibility_offsets(draws, meshes)
    dvb, mvb = np.zeros(max(1, len(draws)), np.uint32), np.zeros(max(1, (slots + 31) // 32 + 2), np.uint32)
    pyr = oracle.Pyramid(w, h)
    depth = np.zeros((h, w), np.float32)
    cap = 4096 + 64
    out = []
    for _ in range(frames):
        rec = {}
        for name, late, pp in [("early", 0, 0), ("late", 1, 0)] + ([("post", 1, 1)] if post_pass else []):
            if name == "late":
                oracle.depthreduce(depth, pyr)
            pd = cd.copy()
            pd["clusterBackfaceEnabled"] = 1 if pp == 0 else 0
            pd["postPass"] = pp
            co, c4 = np.zeros(cap, dtype=L.TASKCMD), np.zeros(4, np.uint32)
            oracle.drawcull(pd, late, 1, draws, meshes, co, c4, dvb, pyr)
            oracle.tasksubmit(c4, co)
            ncmd = int(c4[1]) * 64
            cc = cd.copy()
            cc["postPass"] = pp
            cib, cc4 = np.zeros(ncmd * 64 + 256, np.uint32), np.zeros(4, np.uint32)
            oracle.clustercull(cc, late, co, c4, draws, meshlets, mvb, pyr, cib, cc4)
            oracle.clustersubmit(cc4, cib)
            g = globals_for(cd, (w, h), pp)
            depth, _, _ = rref.raster(g, co, draws, meshlets, scene["data"], scene["vertices"], cib, cc4, w, h, depth=None if name == "early" else depth)
            nv = int(cc4[2]) * 256
            rec[name] = dict(count4=c4.copy(), commands=co[:ncmd].copy(), cc4=cc4.copy(), cib=cib[:nv].copy(), dvb=dvb.copy(), mvb=mvb.copy(),
                             depth=depth.copy())
        rec["pyramid"] = pyr.data.copy()
        rec["draws"] = draws
        out.append(rec)
    return out


def mesh_scene(pos, tris, viewport, draws=None, cam=None, flags=None):
    """Raster inputs from one triangle list: `pos` (n, 3) mesh-local positions (stored as fp16), `tris` (t, 3) vertex ids, cut into
    meshlets in order (<= 64 vertices, <= 96 triangles); one draw per row of `draws` (default: identity at the origin); every meshlet of
    every draw in the cluster list.  Returns the arguments of RasterRef.raster / nv_rasterdepth as a dict."""
    from niagara_amd import host, synth
    pos = np.asarray(pos, np.float32)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    groups, cur, used = [], [], {}
    for t in tris:
        new = [v for v in dict.fromkeys(t.tolist()) if v not in used]
        if cur and (len(used) + len(new) > 64 or len(cur) == 96):
            groups.append((cur, used))
            cur, used = [], {}
        for v in t.tolist():
            used.setdefault(v, len(used))
        cur.append(t.tolist())
    if cur:
        groups.append((cur, used))
    vertices = np.zeros(len(pos), dtype=L.VERTEX)
    h = pos.astype(np.float16)
    vertices["vx"], vertices["vy"], vertices["vz"] = (h[:, k].view(np.uint16) for k in range(3))
    meshlets = np.zeros(len(groups), dtype=L.MESHLET)
    words = []
    off = 0
    for i, (ts, used) in enumerate(groups):
        refs = np.array(list(used), np.uint32)
        idx = np.array([[used[v] for v in t] for t in ts], np.uint8).reshape(-1)
        idx = np.append(idx, np.zeros((-len(idx)) % 4, np.uint8))
        w = np.concatenate([refs, idx.view(np.uint32)])
        meshlets[i]["dataOffset"], meshlets[i]["vertexCount"], meshlets[i]["triangleCount"] = off, len(refs), len(ts)
        words.append(w)
        off += len(w)
    data = np.concatenate(words + [np.zeros(4, np.uint32)]).astype(np.uint32)
    if draws is None:
        draws = np.zeros(1, dtype=L.MESHDRAW)
        draws["scale"], draws["orientation"] = 1.0, (0, 0, 0, 1)
    n_cmd = (len(meshlets) + 63) // 64
    commands = np.zeros(len(draws) * n_cmd, dtype=L.TASKCMD)
    ids = []
    for d in range(len(draws)):
        for c in range(n_cmd):
            k = d * n_cmd + c
            commands[k]["drawId"], commands[k]["taskOffset"] = d, c * 64
            commands[k]["taskCount"] = min(64, len(meshlets) - c * 64)
            ids += [k | j << 24 for j in range(int(commands[k]["taskCount"]))]
    cc4 = np.array([len(ids), 0, 0, 0], np.uint32)
    cib = np.concatenate([np.array(ids, np.uint32), np.zeros(512, np.uint32)])
    oracle.clustersubmit(cc4, cib)
    cd = host.build_cull_data(viewport=viewport, **(cam or {}))
    for k, v in (flags or {}).items():
        cd[k] = v
    return dict(g=synth.make_globals(cd, viewport), commands=commands, draws=draws, meshlets=meshlets, data=data, vertices=vertices, cib=cib, cc4=cc4,
                viewport=viewport, cull=cd)


def raster_args(s):
    return (s["g"], s["commands"], s["draws"], s["meshlets"], s["data"], s["vertices"], s["cib"], s["cc4"])
