"""ctypes loader of tests/raster_indexed_alpha_ref.c, the CPU restatement of nv_rasterdepth_indexed_textured (test
infrastructure), the restatement of nv_visibility_attributes_indexed_textured, and the inputs their two test files share.

`load(directory)` compiles the raster restatement there with raster_ref.c's flags, and raster_alpha_ref.c with -DRA_FRAGMENT (texture_ref.c's
statements: the fragment's alpha), which the raster calls through a function pointer.

The textured indexed attribute pass has no C file of its own: `attributes` hands every distinct valid triangle of the indexed records to
texture_ref.c's tr_attributes as a one-triangle meshlet with 32-bit references (what visattr_indexed_ref.c does for the untextured pass), so
the fragment statements that run are texture_ref.c's own; which records are invalid is visattr_indexed_ref.c's decision, asked of it."""
import ctypes as C
import os
import subprocess

import numpy as np

import raster_alpha_ref as RA
import raster_ref as RR
import visattr_ref as VA
from niagara_amd import host, synth
from niagara_amd import layouts as L

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "raster_indexed_alpha_ref.c")
SAMPLE = np.dtype([(n, "<u4") for n in ("px", "py", "command", "triangle", "keep", "status")] + [("alpha", "<f4")])
NO_TEXTURE, SAMPLED, NOT_SAMPLED, NO_MATERIAL, NOT_TESTED = range(5)  # SAMPLE["status"]


class _Params(C.Structure):
    _fields_ = [("materials", C.c_void_p), ("materialCount", C.c_uint32), ("descs", C.c_void_p), ("textureCount", C.c_uint32), ("texels", C.c_void_p),
                ("texelWords", C.c_uint64), ("fragment", C.c_void_p), ("nearClip", C.c_int32), ("alphaTotals2", C.c_void_p), ("log", C.c_void_p),
                ("logCapacity", C.c_uint64), ("logCount", C.c_uint64)]


def _p(a):
    return None if a is None else a.ctypes.data


class IndexedAlphaRef:
    def __init__(self, so_raster, so_fragment):
        self.frag = C.CDLL(so_fragment)
        self.lib = C.CDLL(so_raster)
        self.lib.ria_rasterdepth_indexed.restype = None
        self.lib.ria_rasterdepth_indexed.argtypes = ([C.c_void_p] * 4 + [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                                                         C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_Params)])
        assert self.lib.ria_sample_bytes() == SAMPLE.itemsize and self.lib.ria_params_bytes() == C.sizeof(_Params)

    def raster(self, g, commands, count, draws, indices, vertices, width, height, offsets=None, materials=None, descs=None, texels=None, depth=None,
               vis=None, near_clip=0, log=0, material_count=None, texture_count=None, texel_words=None):
        """dict: depth fp32 (height, width), visibility u64 (None without `offsets`), totals (4) u64 with [3] = samples kept, alpha (2) u64 =
        dropped, unevaluated, and with log = a capacity: samples (SAMPLE records, every covered sample)"""
        d = np.zeros((height, width), np.float32) if depth is None else np.ascontiguousarray(depth, np.float32).copy()
        v = None if offsets is None else (np.zeros((height, width), np.uint64) if vis is None else np.ascontiguousarray(vis, np.uint64).copy())
        tot, alpha = np.zeros(4, np.uint64), np.zeros(2, np.uint64)
        cnt = np.array([int(count)], np.uint32)
        commands, draws = np.ascontiguousarray(commands, L.DRAWCMD), np.ascontiguousarray(draws, L.MESHDRAW)
        ind, vertices = np.ascontiguousarray(indices, np.uint32), np.ascontiguousarray(vertices, L.VERTEX)
        off = None if offsets is None else np.ascontiguousarray(offsets, np.uint64)
        assert off is None or len(off) >= len(draws) + 1
        mats = None if materials is None else np.ascontiguousarray(materials, L.MATERIAL)
        ds = np.ascontiguousarray(descs if descs is not None else np.zeros(1, L.TEXTUREDESC), L.TEXTUREDESC)
        tx = np.ascontiguousarray(texels if texels is not None and len(texels) else np.zeros(1, np.uint32), np.uint32)
        samples = np.zeros(max(1, log), SAMPLE)
        p = _Params(_p(mats), (0 if mats is None else len(mats)) if material_count is None else material_count, _p(ds),
                    (len(ds) if descs is not None else 0) if texture_count is None else texture_count, _p(tx),
                    (len(texels) if texels is not None else 0) if texel_words is None else texel_words,
                    C.cast(self.frag.ra_fragment_alpha, C.c_void_p).value, int(near_clip), _p(alpha), _p(samples) if log else None, log, 0)
        self.lib.ria_rasterdepth_indexed(_p(np.ascontiguousarray(g)), _p(commands), _p(cnt), _p(draws), len(draws), _p(ind), len(ind), _p(vertices),
                                         len(vertices), _p(d), width, height, _p(tot), _p(off), _p(v), C.byref(p))
        out = dict(depth=d, visibility=v, totals=tot, alpha=alpha)
        if log:
            assert p.logCount <= log, "the sample log is too small: %d samples" % p.logCount
            out["samples"] = samples[:p.logCount]
        return out


def load(directory):
    so, frag = (os.path.join(str(directory), "libraster_indexed_alpha_%s.so" % k) for k in ("ref", "fragment"))
    for path, src, extra in ((so, SRC, []), (frag, RA.SRC, ["-DRA_FRAGMENT"])):
        if not os.path.exists(path):
            subprocess.check_call(["gcc"] + RR.FLAGS + extra + ["-Wall", "-Wno-unused-function", "-shared", "-fPIC", "-I", HERE, "-o", path, src, "-lm"])
    return IndexedAlphaRef(so, frag)


# ---- the textured indexed attribute pass

def attributes(tref, iaref, g, records, width, height, draws, indices, vertices, materials, descs, texels, counts=None, **kw):
    """texture_ref.TexRef.attributes' dict for layouts.VISINDEXEDRECORD records.  counts: visattr_indexed_ref's capacity overrides ("draws" /
    "indices" / "vertices" / "materials"); kw: TexRef.attributes' (texel_words, texture_count, taps, real)"""
    records = np.ascontiguousarray(records, L.VISINDEXEDRECORD).reshape(-1)
    draws, indices = np.ascontiguousarray(draws, L.MESHDRAW), np.ascontiguousarray(indices, np.uint32)
    vertices, materials = np.ascontiguousarray(vertices, L.VERTEX), np.ascontiguousarray(materials, L.MATERIAL)
    cnt = dict(draws=len(draws), indices=len(indices), vertices=len(vertices), materials=len(materials))
    cnt.update(counts or {})
    with np.errstate(all="ignore"):
        plain = iaref.attributes(g, records, width, height, draws, indices, vertices, materials, counts=cnt)
    named = records["drawId"] != 0xffffffff
    valid = named & ((plain["flags"] & VA.INVALID) == 0)
    rec = np.zeros(len(records), L.VISRECORD)
    rec["drawId"], rec["depthBits"], rec["meshletIndex"] = records["drawId"], records["depthBits"], 0xffffffff
    at = records["indexPosition"][valid].astype(np.int64)
    tri = (np.stack([indices[at + k] for k in range(3)], 1).astype(np.uint64) + records["vertexOffset"][valid][:, None]).astype(np.uint32)  # mod 2^32
    uniq, inverse = np.unique(tri, axis=0, return_inverse=True) if len(tri) else (np.zeros((0, 3), np.uint32), np.zeros(0, np.int64))
    rec["meshletIndex"][valid] = inverse.reshape(-1)
    meshlets = np.zeros(max(1, len(uniq)), L.MESHLET)
    meshlets["dataOffset"], meshlets["vertexCount"], meshlets["triangleCount"] = 4 * np.arange(len(meshlets)), 3, 1
    data = np.zeros(4 * len(meshlets), np.uint32)
    data.reshape(-1, 4)[:len(uniq), :3] = uniq
    data.reshape(-1, 4)[:, 3] = 0 | 1 << 8 | 2 << 16
    # the capacities the kernel checks lie below the restated tables' sizes: a record past them is already invalid above
    with np.errstate(all="ignore"):
        out = tref.attributes(g, rec, width, height, draws[:cnt["draws"]], meshlets, data, vertices, materials[:cnt["materials"]], descs, texels, **kw)
    assert ((out["flags"] & VA.INVALID) != 0).tolist() == (named & ~valid).tolist()
    return out


# ---- inputs: the cluster scenes of raster_alpha_ref with the classic path's index buffer and commands

def indexed(s, draw_ids):
    """the scene dict plus "indices", the meshes with their index ranges, "icommands" / "icount" — one MeshDrawCommand per draw of `draw_ids`,
    LOD 0, in that order — and "offsets" (host.assign_triangle_offsets)"""
    indices, meshes = synth.indexed_geometry(s["meshes"], s["meshlets"], s["data"])
    c = np.zeros(len(draw_ids), L.DRAWCMD)
    for k, d in enumerate(draw_ids):
        mesh = meshes[int(s["draws"][d]["meshIndex"])]
        c[k]["drawId"], c[k]["instanceCount"], c[k]["vertexOffset"] = d, 1, mesh["vertexOffset"]
        c[k]["firstIndex"], c[k]["indexCount"] = mesh["lods"][0]["indexOffset"], mesh["lods"][0]["indexCount"]
    return dict(s, meshes=meshes, indices=indices, icommands=c, icount=len(c), offsets=host.assign_triangle_offsets(s["draws"], meshes))


def occluder(tref, viewport, mips, size=64, **kw):
    """raster_alpha_ref.occluder — the cut-out wall in the post pass, moved off the axis — and the post launch of the classic path: the wall alone"""
    s = RA.occluder(tref, viewport, mips, size=size, **kw)
    return indexed(s, [int(d) for d in s["wall"]])


def floor(tref, viewport, mips):
    """raster_alpha_ref.floor: the cut-out floor under the camera and the wall beside it; every near triangle crosses the near plane"""
    s = RA.floor(tref, viewport, mips)
    return indexed(s, [int(d) for d in s["surfaces"]])


def sequence(tref, mips, n):
    """raster_alpha_ref.sequence's three kinds of draw — alpha-tested (the cut-out albedo), opaque (no albedo texture), alpha-tested under
    diffuseFactor.a = 0.7, each one quad some 11 x 5 pixels large at 64 x 48 — as n draws and n commands in that repeating order (a launch
    draws at most drawCount commands, so every command has a draw of its own)"""
    s = RA.sequence(tref, mips, 3)
    meshes = np.zeros(1, L.MESH)
    meshes["lodCount"], meshes["vertexCount"], meshes["radius"] = 1, len(s["vertices"]), 2.0
    meshes["lods"]["meshletCount"][0, 0] = len(s["meshlets"])
    s["meshes"] = meshes
    s["draws"] = np.tile(s["draws"], n // 3 + 1)[:n]
    return indexed(s, list(range(n)))


def args(s):
    return s["g"], s["icommands"], s["icount"], s["draws"], s["indices"], s["vertices"]


def tex(s):
    return dict(materials=s["materials"], descs=s["descs"], texels=s["texels"])


def soup(tref, sizes, seed, mips, viewport=(64, 48), materials=(0,)):
    """visindexed_ref.triangle_soup (one command per entry of `sizes`) with planar texcoords, the cut-out set and a post-pass launch; command i's
    draw has material materials[i % len(materials)] of a table whose entry 1 names no albedo texture (opaque from its factor) and whose entry 2
    is the cut-out albedo under diffuseFactor.a = 0.7"""
    import visindexed_ref as VI
    s = VI.triangle_soup(sizes, seed)
    s = RA.textured(dict(s, viewport=viewport), tref, mips)
    m = s["materials"][:3].copy()
    m["albedoTexture"][1] = 0
    m["diffuseFactor"][2, 3] = 0.7
    s["materials"] = m
    s["draws"] = s["draws"].copy()
    s["draws"]["materialIndex"] = [materials[i % len(materials)] for i in range(len(s["draws"]))]
    s["draws"]["postPass"] = 1
    s["cull"] = host.build_cull_data(viewport=viewport, draw_count=len(sizes))
    s["g"] = RR.globals_for(s["cull"], viewport, 1)
    return dict(s, icommands=s["commands"], icount=s["count"])
