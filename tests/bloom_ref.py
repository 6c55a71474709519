"""ctypes loader of tests/bloom_ref.c, the CPU restatement of the bloom passes and of final.comp.glsl with its bloom term (test
infrastructure), and the fixed-seed input builders of the bloom tests.

`load(directory)` compiles the restatement there twice, as shade_ref.py does: as fp32 (the bits the kernels must write, up to pow and exp2) and
with -DREAL=double.  Every method takes real="f32" / "f64".  A bloom target is handled as a list of per-level (h, w) uint32 arrays; `pack` /
`unpack` go between that and the one linear buffer of the C ABI."""
import ctypes as C
import os
import subprocess

import numpy as np

import raster_ref as RR
from niagara_amd import layouts as L

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "bloom_ref.c")
MAX_LEVELS = 8


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def mip_levels(w, h):
    """src/resources.cpp:280-292"""
    n = 1
    while w > 1 or h > 1:
        n, w, h = n + 1, w // 2, h // 2
    return n


def desc(width, height):
    """src/niagara.cpp:1331-1333 by the issue's formulas: dict(width, height, levels, sizes [(w, h)], offsets [8], total)"""
    bw, bh = (width + 1) // 2, (height + 1) // 2
    levels = min(MAX_LEVELS, mip_levels(bw, bh))
    sizes = [(max(1, bw >> i), max(1, bh >> i)) for i in range(levels)]
    offsets, at = [], 0
    for i in range(MAX_LEVELS):
        offsets.append(at)
        if i < levels:
            at += sizes[i][0] * sizes[i][1]
    return dict(width=bw, height=bh, levels=levels, sizes=sizes, offsets=offsets, total=at)


def pack(levels):
    return np.concatenate([np.ascontiguousarray(l, np.uint32).reshape(-1) for l in levels])


def unpack(words, d):
    words = np.asarray(words).view(np.uint32).reshape(-1)
    return [words[d["offsets"][i]:d["offsets"][i] + w * h].reshape(h, w).copy() for i, (w, h) in enumerate(d["sizes"])]


def codes(words):
    """(..., 3) int64 R, G, B codes of B10G11R11 words"""
    w = np.asarray(words).view(np.uint32)
    return np.stack([w & np.uint32(2047), (w >> np.uint32(11)) & np.uint32(2047), w >> np.uint32(22)], -1).astype(np.int64)


class BloomRef:
    def __init__(self, so32, so64):
        self.libs = {"f32": C.CDLL(so32), "f64": C.CDLL(so64)}
        for k, size in (("f32", 4), ("f64", 8)):
            for f in ("br_decode_array", "br_encode_array", "br_extract", "br_downsample", "br_upsample", "br_shade_final_bloom", "sr_set_perturb"):
                getattr(self.libs[k], f).restype = None
            assert self.libs[k].sr_real_bytes() == size

    @staticmethod
    def _rt(real):
        return np.float32 if real == "f32" else np.float64

    def perturb(self, mode, ulps=2):
        """move every pow / exp2 result of the fp32 build by `ulps` fp32 ULPs: mode 0 off, 1 up, 2 down, 3 a fixed mix"""
        self.libs["f32"].sr_set_perturb(C.c_int(mode), C.c_int(ulps))

    def decode(self, code_array, mbits, real="f32"):
        c = np.ascontiguousarray(code_array, np.uint32).reshape(-1)
        out = np.zeros(c.size, self._rt(real))
        self.libs[real].br_decode_array(_p(c), C.c_uint32(c.size), C.c_int(mbits), _p(out))
        return out

    def encode(self, values, mbits, real="f32"):
        v = np.ascontiguousarray(values, self._rt(real)).reshape(-1)
        out = np.zeros(v.size, np.uint32)
        self.libs[real].br_encode_array(_p(v), C.c_uint32(v.size), C.c_int(mbits), _p(out))
        return out

    def extract(self, gbuffer0, real="f32", value=False):
        """pass 0: gbuffer0 (H, W) u32 -> level 0 ((H + 1) // 2, (W + 1) // 2) u32 [, the values handed to the store (h, w, 3)], here and in
        passes 1 and 2"""
        g0 = np.ascontiguousarray(gbuffer0).view(np.uint32)
        H, W = g0.shape
        w, h = (W + 1) // 2, (H + 1) // 2
        out = np.zeros((h, w), np.uint32)
        v = np.zeros((h, w, 3), self._rt(real)) if value else None
        self.libs[real].br_extract(_p(g0), C.c_uint32(W), C.c_uint32(H), _p(out), C.c_uint32(w), C.c_uint32(h), _p(v))
        return (out, v) if value else out

    def downsample(self, src, real="f32", value=False):
        """pass 1: a level (H, W) -> the next one (max(1, H >> 1), max(1, W >> 1))"""
        s = np.ascontiguousarray(src, np.uint32)
        H, W = s.shape
        w, h = max(1, W >> 1), max(1, H >> 1)
        out = np.zeros((h, w), np.uint32)
        v = np.zeros((h, w, 3), self._rt(real)) if value else None
        self.libs[real].br_downsample(_p(s), C.c_uint32(W), C.c_uint32(H), _p(out), C.c_uint32(w), C.c_uint32(h), _p(v))
        return (out, v) if value else out

    def upsample(self, src, dst, radius, real="f32", value=False):
        """pass 2: the accumulated copy of `dst` (h, w) from `src` (H, W)"""
        s, d = np.ascontiguousarray(src, np.uint32), np.ascontiguousarray(dst, np.uint32).copy()
        v = np.zeros(d.shape + (3,), self._rt(real)) if value else None
        self.libs[real].br_upsample(_p(s), C.c_uint32(s.shape[1]), C.c_uint32(s.shape[0]), _p(d), C.c_uint32(d.shape[1]), C.c_uint32(d.shape[0]),
                                    C.c_float(radius), _p(v))
        return (d, v) if value else d

    def chain_from(self, level0, levels, real="f32"):
        """src/niagara.cpp:1873-1901 behind pass 0: downsample 1 .. levels - 1, upsample levels - 2 .. 0 with radius 2"""
        out = [np.ascontiguousarray(level0, np.uint32).copy()]
        for _ in range(1, levels):
            out.append(self.downsample(out[-1], real))
        for i in range(levels - 2, -1, -1):
            out[i] = self.upsample(out[i + 1], out[i], 2.0, real)
        return out

    def chain(self, gbuffer0, real="f32"):
        H, W = np.asarray(gbuffer0).shape
        return self.chain_from(self.extract(gbuffer0, real), desc(W, H)["levels"], real)

    def shade_final_bloom(self, sd, gbuffer0, gbuffer1, depth, shadow, bloom0, real="f32", value=False):
        """final.comp.glsl with bloom0, level 0 of the bloom target ((h + 1) // 2, (w + 1) // 2) u32"""
        h, w = depth.shape
        sd = np.ascontiguousarray(sd, L.SHADEDATA)
        g0 = np.ascontiguousarray(gbuffer0).view(np.uint32).reshape(h, w)
        g1 = np.ascontiguousarray(gbuffer1).view(np.uint32).reshape(h, w)
        d = np.ascontiguousarray(depth, np.float32)
        s = None if shadow is None else np.ascontiguousarray(shadow, np.uint8).reshape(h, w)
        b = np.ascontiguousarray(bloom0, np.uint32)
        assert b.shape == ((h + 1) // 2, (w + 1) // 2)
        assert s is not None or int(sd["shadowsEnabled"][0]) != 1
        out = np.zeros((h, w), np.uint32)
        v = np.zeros((h, w, 4), self._rt(real)) if value else None
        self.libs[real].br_shade_final_bloom(_p(sd), _p(g0), _p(g1), _p(d), _p(s), _p(b), C.c_uint32(b.shape[1]), C.c_uint32(b.shape[0]), _p(out),
                                             C.c_uint32(w), C.c_uint32(h), _p(v))
        return (out, v) if value else out


def load(directory):
    so32, so64 = (os.path.join(str(directory), "libbloom_ref_%s.so" % k) for k in ("f32", "f64"))
    for so, extra in ((so32, []), (so64, ["-DREAL=double"])):
        if not os.path.exists(so):
            subprocess.check_call(["gcc"] + RR.FLAGS + extra + ["-Wall", "-Wno-unused-function", "-shared", "-fPIC", "-I", HERE, "-o", so, SRC, "-lm"])
    return BloomRef(so32, so64)


# ---- inputs

def test_gbuffer0(w, h, seed=0):
    """gbuffer0 of the pass-0 tests for a w x h image: random words (every albedo and emissive code), a block without emission (alpha 0) and,
    where the image has room, the two extreme words"""
    rng = np.random.default_rng(7000 * w + h + seed)
    g0 = rng.integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)
    if w >= 5 and h >= 3:
        g0[h // 2:, : max(1, w // 4)] &= np.uint32(0x00FFFFFF)
    if w * h >= 64:
        g0.reshape(-1)[[5, -6]] = (0, 0xFFFFFFFF)
    return g0


def test_levels(width, height, seed=0, top=30, specials=True):
    """The given words of the pass-1 / pass-2 tests, every level of the bloom target of a width x height image: random mantissas under
    exponents 0 (denormal codes, about one in `top + 1`) to `top` (30: sums of the largest pass the format's maximum), zeros, and in every level
    of 16 texels or more two inf codes and two NaN codes"""
    d = desc(width, height)
    rng = np.random.default_rng(9000 * width + height + seed)
    out = []
    for w, h in d["sizes"]:
        e = rng.integers(0, top + 1, (h, w, 3)).astype(np.uint32)
        m = rng.integers(0, 64, (h, w, 3)).astype(np.uint32)
        r, g, b = (e[..., 0] << 6 | m[..., 0]), (e[..., 1] << 6 | m[..., 1]), (e[..., 2] << 5 | m[..., 2] >> 1)
        words = (r | g << 11 | b << 22).astype(np.uint32)
        flat = words.reshape(-1)
        flat[rng.random(flat.size) < 0.05] = 0
        if specials and flat.size >= 16:
            at = rng.choice(flat.size, size=4, replace=False)
            flat[at] = (31 << 6 | (7 << 11), (31 << 6 | 1) | (3 << 22), (31 << 5) << 22, ((31 << 5 | 16) << 22) | 5)
        out.append(words)
    return out


test_gbuffer0.__test__ = False
test_levels.__test__ = False
