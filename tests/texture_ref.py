"""ctypes loader of tests/texture_ref.c, the CPU restatement of the material textures (test infrastructure): block decode,
the software sampler, and nv_visibility_attributes_textured one pixel at a time.

`load(directory)` compiles it there twice with raster_ref.c's flags: as fp32 (the bits the kernels must write) and with -DREAL=double."""
import ctypes as C
import os
import subprocess

import numpy as np

import raster_ref as RR
import visattr_ref as VA
from niagara_amd import layouts as L

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "texture_ref.c")
NOT_SAMPLED, NORMAL_MAPPED = 16, 32  # flags of attributes() besides visattr_ref's SHADED, INVALID, DEGENERATE
BLOCK_BYTES = {1: 8, 2: 16, 3: 16, 7: 16}


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def image_size_bc(width, height, levels, block_size):
    """getImageSizeBC (src/textures.cpp:129-142), restated: the bytes of a chain and the byte offset of each level"""
    total, offsets = 0, []
    for _ in range(levels):
        offsets.append(total)
        total += ((width + 3) // 4) * ((height + 3) // 4) * block_size
        width, height = (width // 2 if width > 1 else 1), (height // 2 if height > 1 else 1)
    return total, offsets


def chain_words(width, height, levels):
    return sum(max(1, width >> l) * max(1, height >> l) for l in range(levels))


class TexRef:
    def __init__(self, so32, so64):
        self.libs = {"f32": C.CDLL(so32), "f64": C.CDLL(so64)}
        for k, size in (("f32", 4), ("f64", 8)):
            assert self.libs[k].va_real_bytes() == size
            for f in ("tr_decode_block", "tr_decode_chain", "tr_sample_many", "tr_attributes", "tr_attributes_taps", "tr_hits"):
                getattr(self.libs[k], f).restype = None
            self.libs[k].tr_bad_indices.restype = C.c_uint64

    def decode_blocks(self, fmt, blocks):
        """blocks (n, 8 or 16) uint8 -> (n, 64) uint8"""
        blocks = np.ascontiguousarray(blocks, np.uint8)
        out = np.zeros((len(blocks), 16), np.uint32)
        for i in range(len(blocks)):
            self.libs["f32"].tr_decode_block(C.c_uint32(fmt), _p(blocks[i]), _p(out[i]))
        return out.view(np.uint8).reshape(len(blocks), 64)

    def decode_chain(self, fmt, width, height, levels, payload):
        payload = np.ascontiguousarray(np.frombuffer(bytes(payload), np.uint8))
        assert len(payload) == image_size_bc(width, height, levels, BLOCK_BYTES[fmt])[0]
        out = np.zeros(chain_words(width, height, levels), np.uint32)
        self.libs["f32"].tr_decode_chain(C.c_uint32(fmt), C.c_uint32(width), C.c_uint32(height), C.c_uint32(levels), _p(payload), _p(out))
        return out

    def decode_set(self, files):
        """DDS file images (FourCC or DX10 headers of the four decodable formats, parsed here on their own) -> (descs, texels)"""
        descs, chunks, at = np.zeros(len(files) + 1, L.TEXTUREDESC), [], 0
        for i, data in enumerate(files):
            w = np.frombuffer(bytes(data[:148].ljust(148, b"\0")), "<u4")
            fmt = {0x31545844: 1, 0x33545844: 2, 0x35545844: 3}.get(int(w[21])) or {71: 1, 72: 1, 74: 2, 75: 2, 77: 3, 78: 3, 98: 7, 99: 7}[int(w[32])]
            start = 148 if int(w[21]) == 0x30315844 else 128
            height, width, levels = int(w[3]), int(w[4]), int(w[7])
            chunks.append(self.decode_chain(fmt, width, height, levels, data[start:]))
            descs[i + 1] = (at, width, height, levels)
            at += len(chunks[-1])
        return descs, (np.concatenate(chunks) if chunks else np.zeros(0, np.uint32))

    def sample(self, descs, texels, tex_id, uv, dx=None, dy=None, real="f32", texel_words=None):
        """n samples: (out (n, 4) of `real`, ok (n,) bool)"""
        rt = np.float32 if real == "f32" else np.float64
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        n = len(uv)
        dx = np.zeros((n, 2), np.float32) if dx is None else np.ascontiguousarray(dx, np.float32).reshape(-1, 2)
        dy = np.zeros((n, 2), np.float32) if dy is None else np.ascontiguousarray(dy, np.float32).reshape(-1, 2)
        descs, texels = np.ascontiguousarray(descs, L.TEXTUREDESC), np.ascontiguousarray(texels, np.uint32)
        out, ok = np.zeros((n, 4), rt), np.zeros(n, np.uint8)
        self.libs[real].tr_sample_many(_p(descs), C.c_uint32(len(descs)), _p(texels), C.c_uint64(len(texels) if texel_words is None else texel_words),
                                       C.c_uint32(tex_id), C.c_uint32(n), _p(uv), _p(dx), _p(dy), _p(out), _p(ok))
        return out, ok.astype(bool)

    def bad_indices(self, real="f32"):
        """loads the restatement refused because their index lay outside the texel buffer: 0 for a correct rule set"""
        return int(self.libs[real].tr_bad_indices())

    def hits(self, real="f32", reset=True):
        """samples per level d (15 entries) and, last, samples with f != 0, since the last reset"""
        out = np.zeros(16, np.uint64)
        self.libs[real].tr_hits(_p(out), C.c_int(1 if reset else 0))
        return out

    def attributes(self, g, records, width, height, draws, meshlets, data, vertices, materials, descs, texels, real="f32", texel_words=None,
                   texture_count=None, taps=False):
        """visattr_ref.AttrRef.attributes with the complete fragment stage; flags: NOT_SAMPLED, NORMAL_MAPPED besides visattr_ref's.
        taps=True adds "taps" (h * w, 4, 4): the texel the albedo / normal / specular / emissive slot was given (0 where it was not sampled)"""
        rt = np.float32 if real == "f32" else np.float64
        n = width * height
        records = np.ascontiguousarray(records, L.VISRECORD).reshape(-1)
        assert len(records) == n
        draws, meshlets = np.ascontiguousarray(draws, L.MESHDRAW), np.ascontiguousarray(meshlets, L.MESHLET)
        data, vertices = np.ascontiguousarray(data, np.uint32), np.ascontiguousarray(vertices, L.VERTEX)
        mats = np.ascontiguousarray(materials, L.MATERIAL)
        descs = np.ascontiguousarray(descs if descs is not None else np.zeros(1, L.TEXTUREDESC), L.TEXTUREDESC)
        tex = np.ascontiguousarray(texels if texels is not None and len(texels) else np.zeros(1, np.uint32), np.uint32)
        words = (len(texels) if texels is not None else 0) if texel_words is None else texel_words
        count = len(descs) if texture_count is None else texture_count
        out = dict(vals=np.zeros((n, 14), rt), ids=np.zeros((n, 2), np.uint32), gbuffer0=np.zeros(n, np.uint32), gbuffer1=np.zeros(n, np.uint32),
                   totals=np.zeros(4, np.uint64), flags=np.zeros(n, np.uint8), chan=np.zeros((n, 8), rt))
        args = [_p(np.ascontiguousarray(g)), _p(records), C.c_uint32(width), C.c_uint32(height), _p(draws), C.c_uint32(len(draws)),
                _p(meshlets), C.c_uint32(len(meshlets)), _p(data), C.c_uint32(len(data)), _p(vertices), C.c_uint32(len(vertices)),
                _p(mats), C.c_uint32(len(mats)), _p(descs), C.c_uint32(count), _p(tex), C.c_uint64(words), _p(out["vals"]),
                _p(out["ids"]), _p(out["gbuffer0"]), _p(out["gbuffer1"]), _p(out["totals"]), _p(out["flags"]), _p(out["chan"])]
        if taps:
            out["taps"] = np.zeros((n, 4, 4), rt)
            self.libs[real].tr_attributes_taps(*args, _p(out["taps"]))
        else:
            self.libs[real].tr_attributes(*args)
        if real == "f32":
            a = np.zeros(n, L.PIXELATTR)
            for name, sl in VA._SLICES.items():
                a[name] = out["vals"][:, sl]
            a["drawId"], a["materialIndex"] = out["ids"][:, 0], out["ids"][:, 1]
            out["attributes"] = a
        return out


def load(directory):
    so32, so64 = (os.path.join(str(directory), "libtexture_ref_%s.so" % k) for k in ("f32", "f64"))
    for so, extra in ((so32, []), (so64, ["-DREAL=double"])):
        if not os.path.exists(so):
            subprocess.check_call(["gcc"] + RR.FLAGS + extra + ["-Wall", "-Wno-unused-function", "-shared", "-fPIC", "-I", HERE, "-o", so, SRC, "-lm"])
    return TexRef(so32, so64)


def dds_header(fmt, width, height, levels, dx10=False, **over):
    """a DDS header for the parser tests: FourCC spelling, or the DX10 spelling with dxgi format `fmt`; `over` overrides a word by its name"""
    four = {1: b"DXT1", 2: b"DXT3", 3: b"DXT5", 4: b"ATI1", 5: b"ATI2"}
    w = np.zeros(37 if dx10 else 32, np.uint32)
    w[0], w[1], w[3], w[4], w[7], w[19], w[20] = 0x20534444, 124, height, width, levels, 32, 4
    w[21] = 0x30315844 if dx10 else int.from_bytes(four[fmt], "little")
    if dx10:
        w[32], w[33], w[35] = fmt, 3, 1
    names = dict(magic=0, size=1, height=3, width=4, mips=7, pf_size=19, fourcc=21, caps2=28, dxgi=32, dimension=33)
    for k, v in over.items():
        w[names[k]] = v
    return w.tobytes()
