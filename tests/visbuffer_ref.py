"""ctypes loader of tests/visbuffer_ref.c, the CPU reference of the frame-stable visibility buffer (test infrastructure): nv_rasterdepth
with NV_OPT_RASTER_VISIBILITY_ID 1, nv_visibility_resolve, and the word's encode / decode.

`load(directory)` compiles it there with gcc and raster_ref.c's flags and returns a VisRef.  `VisRef.frame_raster(near_clip)` offers
RasterRef.raster's signature and keeps the frame's visibility target between the calls, so raster_ref.oracle_frames(..., rref=) and
sharded_ref.OracleRank(..., rref) run the closed loop with it."""
import ctypes as C
import os
import subprocess

import numpy as np

import raster_ref as RR
from niagara_amd import layouts as L

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "visbuffer_ref.c")
SHIFT = 34
ID_MASK = (1 << SHIFT) - 1
MVI_END = (1 << 27) - 1
NO_SAMPLE = (0xFFFFFFFF, 0, 0, 0)
UNRESOLVED = (0xFFFFFFFF,) * 4


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def encode(depth_bits, mvi, triangle):
    """the stable word of a sample: bits(z) << 34 | ((mvi << 7 | triangle) + 1)"""
    assert 0 <= depth_bits <= 0x3F800000 and 0 <= mvi < MVI_END and 0 <= triangle < 128
    return int(depth_bits) << SHIFT | (((int(mvi) << 7) | int(triangle)) + 1)


def decode(word):
    """(depth bits, mvi, triangle) of a non-zero stable word"""
    word = int(word)
    id34 = word & ID_MASK
    return word >> SHIFT, (id34 - 1) >> 7, (id34 - 1) & 127


class FrameRaster:
    """RasterRef.raster with the stable-form visibility target of a frame kept inside: a call without `depth` (the early pass) clears it,
    the others load it.  history[k] = the target after the k-th call"""

    def __init__(self, ref, near_clip):
        self.ref, self.near_clip = ref, int(near_clip)
        self.vis, self.history = None, []

    def raster(self, g, commands, draws, meshlets, data, vertices, cib, cc4, width, height, depth=None, visibility=False):
        if depth is None or self.vis is None:
            self.vis = np.zeros((height, width), np.uint64)
        d, self.vis, tot = self.ref.raster(g, commands, draws, meshlets, data, vertices, cib, cc4, width, height, depth=depth, vis=self.vis,
                                           near_clip=self.near_clip)
        self.history.append(self.vis.copy())
        return d, self.vis.copy(), tot


class VisRef:
    def __init__(self, so):
        self.lib = C.CDLL(so)
        for f in ("vb_rasterdepth", "vb_resolve", "vb_single_triangle"):
            getattr(self.lib, f).restype = None

    def raster(self, g, commands, draws, meshlets, data, vertices, cib, cc4, width, height, depth=None, vis=None, near_clip=0):
        """(depth fp32 (height, width), stable-form visibility u64, totals4); depth / vis: the targets to load instead of cleared ones"""
        d = np.zeros((height, width), np.float32) if depth is None else np.ascontiguousarray(depth, np.float32).copy()
        v = np.zeros((height, width), np.uint64) if vis is None else np.ascontiguousarray(vis, np.uint64).copy()
        tot = np.zeros(4, np.uint64)
        self.lib.vb_rasterdepth(_p(g), _p(commands), _p(draws), _p(meshlets), _p(data), _p(vertices), _p(cib), _p(cc4), _p(d), C.c_uint32(width),
                                C.c_uint32(height), _p(v), _p(tot), C.c_int(int(near_clip)))
        return d, v, tot

    def frame_raster(self, near_clip=0):
        return FrameRaster(self, near_clip)

    def resolve(self, cull, vis, draws, meshes, mvb_words):
        """nv_visibility_resolve: dict(records (h * w VISRECORD), seen (mvb_words u32), draw_pixels (len(draws) u32), totals (4 u64))"""
        vis = np.ascontiguousarray(vis, np.uint64).reshape(-1)
        draws = np.ascontiguousarray(draws, L.MESHDRAW)
        meshes = np.ascontiguousarray(meshes, L.MESH)
        rec = np.zeros(len(vis), L.VISRECORD)
        seen = np.zeros(mvb_words, np.uint32)
        dp = np.zeros(max(1, len(draws)), np.uint32)
        tot = np.zeros(4, np.uint64)
        self.lib.vb_resolve(_p(np.ascontiguousarray(cull)), _p(vis), C.c_uint32(len(vis)), _p(draws if len(draws) else np.zeros(1, L.MESHDRAW)),
                            C.c_uint32(len(draws)), _p(meshes if len(meshes) else np.zeros(1, L.MESH)), C.c_uint32(len(meshes)), _p(rec), _p(seen),
                            _p(dp), _p(tot))
        return dict(records=rec, seen=seen, draw_pixels=dp, totals=tot)

    def single_triangle(self, g, draw, meshlet, data, vertices, triangle, width, height, near_clip=0):
        """depth bits (height, width) u32 of ONE triangle of one meshlet under one draw rasterised alone (both faces); 0 where not covered"""
        z = np.zeros((height, width), np.uint32)
        d = np.ascontiguousarray(np.atleast_1d(draw), L.MESHDRAW)
        m = np.ascontiguousarray(np.atleast_1d(meshlet), L.MESHLET)
        self.lib.vb_single_triangle(_p(g), _p(d), _p(m), _p(data), _p(vertices), C.c_uint32(int(triangle)), C.c_int(int(near_clip)), C.c_uint32(width),
                                    C.c_uint32(height), _p(z))
        return z


def load(directory):
    so = os.path.join(str(directory), "libvisbuffer_ref.so")
    if not os.path.exists(so):
        subprocess.check_call(["gcc"] + RR.FLAGS + ["-Wall", "-shared", "-fPIC", "-I", HERE, "-o", so, SRC, "-lm"])
    return VisRef(so)


def oracle_frames(scene, frames, post_pass, vref, near_clip=0):
    """raster_ref.oracle_frames with the stable-form visibility target: every frame's record also carries "visibility", the target after
    its last raster"""
    fr = vref.frame_raster(near_clip)
    out = RR.oracle_frames(scene, frames, post_pass=post_pass, rref=fr)
    per = 3 if post_pass else 2
    for f, rec in enumerate(out):
        rec["visibility"] = fr.history[(f + 1) * per - 1]
    return out


def frame_commands(rec, post_pass):
    """the task commands of a frame's rasterised lists (early, late, post), padding dropped"""
    names = ["early", "late"] + (["post"] if post_pass else [])
    return np.concatenate([rec[n]["commands"][:int(rec[n]["count4"][0])] for n in names])


def rasterised_clusters(rec, post_pass):
    """the set of meshlet-visibility indices of every cluster in one of the frame's rasterised lists"""
    out = set()
    for n in ["early", "late"] + (["post"] if post_pass else []):
        r = rec[n]
        ids = r["cib"][:int(r["cc4"][0])]
        ids = ids[ids != 0xffffffff]
        out |= set((r["commands"]["meshletVisibilityOffset"][ids & 0xffffff].astype(np.int64) + (ids >> 24)).tolist())
    return out


def decode_by_commands(vis, commands):
    """The independent decode of a stable-form target: per non-zero word the command whose [meshletVisibilityOffset, + taskCount) holds mvi
    gives drawId and meshletIndex = taskOffset + (mvi - offset).  No LOD is evaluated.  Returns VISRECORD records (unresolved where no
    command holds mvi, or triangle >= 96)."""
    vis = np.asarray(vis, np.uint64).reshape(-1)
    rec = np.zeros(len(vis), L.VISRECORD)
    rec["drawId"] = 0xFFFFFFFF
    has = vis != 0
    id34 = (vis & np.uint64(ID_MASK)).astype(np.int64)
    mvi, tri = (id34 - 1) >> 7, (id34 - 1) & 127
    cm = np.unique(commands[commands["taskCount"] > 0])  # early / late / post repeat commands
    order = np.argsort(cm["meshletVisibilityOffset"], kind="stable")
    cm = cm[order]
    off = cm["meshletVisibilityOffset"].astype(np.int64)
    # commands of one draw and LOD tile its range; two commands with the same offset would be two LODs of one draw in one frame
    assert len(np.unique(off)) == len(off)
    k = np.searchsorted(off, mvi, side="right") - 1
    kc = np.clip(k, 0, max(0, len(cm) - 1))
    ok = has & (id34 != 0) & (k >= 0) & (len(cm) > 0)
    if len(cm):
        ok &= (mvi - off[kc]) < cm["taskCount"][kc].astype(np.int64)
    ok &= tri < 96
    bad = has & ~ok
    if len(cm):
        rec["drawId"][ok] = cm["drawId"][kc][ok]
        rec["meshletIndex"][ok] = (cm["taskOffset"][kc].astype(np.int64) + mvi - off[kc])[ok]
    rec["triangle"][ok] = tri[ok]
    rec["depthBits"][ok] = (vis >> np.uint64(SHIFT)).astype(np.uint32)[ok]
    for f in L.VISRECORD.names:
        rec[f][bad] = 0xFFFFFFFF
    return rec
