"""ctypes loader of tests/raster_alpha_ref.c, the CPU restatement of nv_rasterdepth_textured (test infrastructure), and the
inputs its two test files share: post-pass cluster lists of the synthetic scenes and their decoded texture sets.

`load(directory)` compiles the file there twice with raster_ref.c's flags: with -DRA_FRAGMENT (texture_ref.c's statements: the fragment's alpha)
and without (raster_clip_ref.c's walk, which calls the first through a function pointer)."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle
import raster_ref as RR
from niagara_amd import layouts as L
from niagara_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "raster_alpha_ref.c")
COUNTERS = ("slots_tested", "slots_constant", "slots_absent", "slots_opaque", "tested_samples", "undecided", "tested_small", "tested_large",
            "tested_cut_stamps", "tested_clipped", "nan_alpha")
SAMPLE = np.dtype([(n, "<u4") for n in ("px", "py", "index", "drawId", "meshlet", "triangle", "keep", "status")] + [("alpha", "<f4")])
NO_TEXTURE, SAMPLED, NOT_SAMPLED, NO_MATERIAL, NOT_TESTED = range(5)  # SAMPLE["status"]


class _Params(C.Structure):
    _fields_ = [("materials", C.c_void_p), ("materialCount", C.c_uint32), ("descs", C.c_void_p), ("textureCount", C.c_uint32), ("texels", C.c_void_p),
                ("texelWords", C.c_uint64), ("fragment", C.c_void_p), ("nearClip", C.c_int32), ("stable", C.c_int32), ("band", C.c_int32),
                ("policy", C.c_int32), ("smallLimit", C.c_uint32), ("alphaTotals2", C.c_void_p), ("counters", C.c_void_p), ("undecidedMask", C.c_void_p),
                ("log", C.c_void_p), ("logCapacity", C.c_uint64), ("logCount", C.c_uint64)]


def _p(a):
    return None if a is None else a.ctypes.data


class AlphaRef:
    def __init__(self, so_raster, so_fragment):
        self.frag = C.CDLL(so_fragment)
        self.lib = C.CDLL(so_raster)
        self.lib.ra_rasterdepth.restype = None
        self.frag.tr_hits.restype = None
        self.lib.ra_rasterdepth.argtypes = [C.c_void_p] * 9 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(_Params)]
        assert self.lib.ra_sample_bytes() == SAMPLE.itemsize and self.lib.ra_params_bytes() == C.sizeof(_Params)

    def hits(self, reset=True):
        """texture_ref.TexRef.hits of the fragment library: samples per level d (15 entries) and, last, samples with f != 0, since the last reset"""
        out = np.zeros(16, np.uint64)
        self.frag.tr_hits(C.c_void_p(out.ctypes.data), C.c_int(1 if reset else 0))
        return out

    def raster(self, g, commands, draws, meshlets, data, vertices, cib, cc4, width, height, materials=None, descs=None, texels=None, depth=None,
               visibility=True, near_clip=0, stable=0, band=False, policy=0, small_limit=16, log=0, material_count=None, texture_count=None,
               texel_words=None):
        """dict: depth fp32 (height, width), visibility u64 or None, totals (4) u64 with [3] = samples kept, alpha (2) u64 = dropped, unevaluated,
        counters (dict of COUNTERS), undecided (height, width) bool, and with log = a capacity: samples (SAMPLE records, every covered sample in
        the walk's order).  band: a sampled alpha within B of 0.5 is undecided; policy 1 drops every undecided sample, 2 keeps it"""
        d = np.zeros((height, width), np.float32) if depth is None else np.ascontiguousarray(depth, np.float32).copy()
        vis = np.zeros((height, width), np.uint64) if visibility else None
        tot, alpha, counters = np.zeros(4, np.uint64), np.zeros(2, np.uint64), np.zeros(len(COUNTERS), np.uint64)
        mask = np.zeros((height, width), np.uint8)
        keep = [np.ascontiguousarray(a) for a in (g, commands, draws, meshlets, data, vertices, cib, cc4)]
        mats = None if materials is None else np.ascontiguousarray(materials, L.MATERIAL)
        ds = np.ascontiguousarray(descs if descs is not None else np.zeros(1, L.TEXTUREDESC), L.TEXTUREDESC)
        tx = np.ascontiguousarray(texels if texels is not None and len(texels) else np.zeros(1, np.uint32), np.uint32)
        samples = np.zeros(max(1, log), SAMPLE)
        p = _Params(_p(mats), (0 if mats is None else len(mats)) if material_count is None else material_count, _p(ds),
                    (len(ds) if descs is not None else 0) if texture_count is None else texture_count, _p(tx),
                    (len(texels) if texels is not None else 0) if texel_words is None else texel_words,
                    C.cast(self.frag.ra_fragment_alpha, C.c_void_p).value, int(near_clip), int(stable), int(band), int(policy), int(small_limit), _p(alpha),
                    _p(counters), _p(mask), _p(samples) if log else None, log, 0)
        self.lib.ra_rasterdepth(*[_p(a) for a in keep], _p(d), width, height, _p(vis), _p(tot), C.byref(p))
        out = dict(depth=d, visibility=vis, totals=tot, alpha=alpha, counters=dict(zip(COUNTERS, (int(c) for c in counters))), undecided=mask.astype(bool))
        if log:
            assert p.logCount <= log, "the sample log is too small: %d samples" % p.logCount
            out["samples"] = samples[:p.logCount]
        return out


def load(directory):
    so, frag = (os.path.join(str(directory), "libraster_alpha_%s.so" % k) for k in ("ref", "fragment"))
    for path, extra in ((so, []), (frag, ["-DRA_FRAGMENT"])):
        if not os.path.exists(path):
            subprocess.check_call(["gcc"] + RR.FLAGS + extra + ["-Wall", "-Wno-unused-function", "-shared", "-fPIC", "-I", HERE, "-o", path, SRC, "-lm"])
    return AlphaRef(so, frag)


# ---- inputs

def draw_list(scene, draw_ids):
    """(commands, cib, cc4): every meshlet of LOD 0 of the draws `draw_ids`, in that order, as the cluster list of one raster launch"""
    cmds, ids = [], []
    for d in draw_ids:
        mesh = scene["meshes"][int(scene["draws"][d]["meshIndex"])]
        first, count = int(mesh["lods"][0]["meshletOffset"]), int(mesh["lods"][0]["meshletCount"])
        for c in range(0, count, 64):
            k = len(cmds)
            cmd = np.zeros(1, L.TASKCMD)[0]
            cmd["drawId"], cmd["taskOffset"], cmd["taskCount"] = d, first + c, min(64, count - c)
            cmd["meshletVisibilityOffset"] = int(scene["draws"][d]["meshletVisibilityOffset"]) + c
            cmds.append(cmd)
            ids += [k | j << 24 for j in range(min(64, count - c))]
    return (np.array(cmds, L.TASKCMD),) + slot_list(ids)


def slot_list(ids):
    """(cib, cc4) of the slots `ids` (cluster indices: command | meshlet << 24), laid out by the oracle's clustersubmit"""
    cc4 = np.array([len(ids), 0, 0, 0], np.uint32)
    cib = np.concatenate([np.array(ids, np.uint32), np.zeros(512, np.uint32)])
    oracle.clustersubmit(cc4, cib)
    return cib, cc4


def textured(scene, tref, mips, cutout=True, size=64):
    """synth.with_textures of `scene` with its set decoded by the texture restatement: the scene dict plus "descs" and "texels" """
    s = synth.with_textures(scene, size=size, mips=mips, cutout=cutout)
    s["descs"], s["texels"] = tref.decode_set(s["textures"])
    return s


# Both scenes are symmetric about the camera's axis: unmoved, whole rows and columns of pixel centres fall exactly on a boundary of the checker's
# cells, where the bilinear alpha is exactly 0.5 (61 of the wall's 961 samples at 67 x 37, 82 of the floor's 57836 at 320 x 192, counted on the
# restatement).  Such a sample is undecided under a mip chain (§4.20), so the surfaces are moved off the axis by these world-space offsets.
WALL_SHIFT = (0.11, 0.07, 0.0)
FLOOR_SHIFT = (0.13, 0.0, 0.0)


def occluder(tref, viewport, mips, box_scale=3.0, size=64):
    """the cut-out occluder scene with the wall's draw in the post pass, and the post launch's list: the wall alone.  size: the textures'
    side (64: the wall is minified at 67 x 37 and magnified at 320 x 192; 256: minified at 320 x 192 too)"""
    s = textured(synth.occluder_scene(viewport=viewport, box_scale=box_scale, meshlet_bounds=oracle.meshlet_bounds), tref, mips, size=size)
    s["draws"] = s["draws"].copy()
    s["draws"]["postPass"][s["wall"]] = 1
    s["draws"]["position"][s["wall"]] += np.array(WALL_SHIFT, np.float32)
    s["commands"], s["cib"], s["cc4"] = draw_list(s, s["wall"])
    s["g"] = RR.globals_for(s["cull"], viewport, 1)
    return s


def floor(tref, viewport, mips):
    """synth.interior_scene with a cut-out floor under the camera (and the wall beside it) in the post pass: every near triangle crosses the
    near plane"""
    s = textured(synth.interior_scene(viewport=viewport, meshlet_bounds=oracle.meshlet_bounds), tref, mips)
    s["draws"] = s["draws"].copy()
    s["draws"]["postPass"][s["surfaces"]] = 1
    s["draws"]["position"][s["surfaces"]] += np.array(FLOOR_SHIFT, np.float32)
    s["commands"], s["cib"], s["cc4"] = draw_list(s, s["surfaces"])
    s["g"] = RR.globals_for(s["cull"], viewport, 1)
    return s


def sequence(tref, mips, slots):
    """`slots` slots in the repeating order alpha-tested (material 0: the cut-out albedo), opaque (material 1: no albedo texture), alpha-tested
    of another material (material 2: the cut-out albedo under diffuseFactor.a = 0.7): whichever three or more consecutive slots a wave takes,
    it goes from an alpha-tested slot to an opaque one and back, and from one material's record to another's.  Each draw is one quad of two
    triangles some 11 x 5 pixels large at 64 x 48: more than 16 centres in the box (the wave path), cut by the box at the stamp's right and
    bottom edge"""
    pos = [(-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0)]
    draws = np.zeros(3, L.MESHDRAW)
    draws["orientation"], draws["scale"], draws["postPass"] = (0, 0, 0, 1), (0.9, 0.5, 0.7), 1
    draws["position"] = [(-1.13, 0.21, -8.0), (0.17, -0.33, -7.0), (0.71, 0.52, -9.0)]
    draws["materialIndex"] = (0, 1, 2)
    s = RR.mesh_scene(pos, [(0, 1, 2), (0, 2, 3)], (64, 48), draws=draws)
    s = textured(s, tref, mips)
    m = s["materials"][:3].copy()
    m["albedoTexture"][1] = 0
    m["diffuseFactor"][2, 3] = 0.7
    s["materials"] = m
    s["cib"], s["cc4"] = slot_list([k % 3 for k in range(slots)])
    s["g"]["cullData"]["postPass"] = 1
    return s


def args(s):
    return (s["g"], s["commands"], s["draws"], s["meshlets"], s["data"], s["vertices"], s["cib"], s["cc4"])
