"""ctypes loader of tests/shade_ref.c, the CPU restatement of nv_shadow_fill, nv_shadow_blur and nv_shade_final (test infrastructure).

`load(directory)` compiles the restatement there twice, with raster_ref.py's flags: as fp32 (the bits the kernels must write, up to pow and
exp2) and with -DREAL=double (the same statements in fp64: the yardstick of the accuracy check).  Every method takes real="f32" / "f64"."""
import ctypes as C
import os
import subprocess

import numpy as np

import raster_ref as RR
from niagara_amd import layouts as L

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "shade_ref.c")


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class ShadeRef:
    def __init__(self, so32, so64):
        self.libs = {"f32": C.CDLL(so32), "f64": C.CDLL(so64)}
        for k, size in (("f32", 4), ("f64", 8)):
            for f in ("sr_shadow_fill", "sr_shadow_blur", "sr_shade_final", "sr_gw", "sr_set_perturb"):
                getattr(self.libs[k], f).restype = None
            assert self.libs[k].sr_real_bytes() == size

    @staticmethod
    def _rt(real):
        return np.float32 if real == "f32" else np.float64

    def perturb(self, mode, ulps=2):
        """move every pow / non-integer exp2 result of the fp32 build by `ulps` fp32 ULPs: mode 0 off, 1 up, 2 down, 3 a fixed mix"""
        self.libs["f32"].sr_set_perturb(C.c_int(mode), C.c_int(ulps))

    def gw(self, real="f32"):
        out = np.zeros(10, np.float32)
        self.libs[real].sr_gw(_p(out))
        return out

    def shadow_fill(self, shadow, depth, checkerboard, real="f32", value=False):
        """(the filled copy of `shadow` (h, w) u8 [, the values handed to the store (h, w)])"""
        h, w = shadow.shape
        s = np.ascontiguousarray(shadow, np.uint8).copy()
        d = np.ascontiguousarray(depth, np.float32).reshape(h, w)
        v = np.zeros((h, w), self._rt(real)) if value else None
        self.libs[real].sr_shadow_fill(_p(s), _p(d), C.c_uint32(w), C.c_uint32(h), C.c_int(checkerboard), _p(v))
        return (s, v) if value else s

    def shadow_blur(self, shadow, depth, direction, znear, real="f32", value=False):
        h, w = shadow.shape
        s = np.ascontiguousarray(shadow, np.uint8)
        d = np.ascontiguousarray(depth, np.float32).reshape(h, w)
        out = np.zeros((h, w), np.uint8)
        v = np.zeros((h, w), self._rt(real)) if value else None
        self.libs[real].sr_shadow_blur(_p(out), _p(s), _p(d), C.c_uint32(w), C.c_uint32(h), C.c_int(direction), C.c_float(znear), _p(v))
        return (out, v) if value else out

    def shade_final(self, sd, gbuffer0, gbuffer1, depth, shadow=None, real="f32", value=False):
        """the colour words (h, w) u32 [, (h, w, 4): tonemap(outputColor).rgb and the deband term before they are added and stored]"""
        h, w = depth.shape
        sd = np.ascontiguousarray(sd, L.SHADEDATA)
        g0 = np.ascontiguousarray(gbuffer0).view(np.uint32).reshape(h, w)
        g1 = np.ascontiguousarray(gbuffer1).view(np.uint32).reshape(h, w)
        d = np.ascontiguousarray(depth, np.float32)
        s = None if shadow is None else np.ascontiguousarray(shadow, np.uint8).reshape(h, w)
        assert s is not None or int(sd["shadowsEnabled"][0]) != 1
        out = np.zeros((h, w), np.uint32)
        v = np.zeros((h, w, 4), self._rt(real)) if value else None
        self.libs[real].sr_shade_final(_p(sd), _p(g0), _p(g1), _p(d), _p(s), _p(out), C.c_uint32(w), C.c_uint32(h), _p(v))
        return (out, v) if value else out

    def shade(self, sd, gbuffer0, gbuffer1, depth, shadow=None, blur=True, checkerboard=False, znear=0.1, real="f32"):
        """VisibilityPipeline.shade chained on the CPU: fill (checkerboard 1), blur horizontal then vertical, final"""
        if shadow is not None:
            if checkerboard:
                shadow = self.shadow_fill(shadow, depth, 1, real)
            if blur:
                shadow = self.shadow_blur(self.shadow_blur(shadow, depth, 1, znear, real), depth, 0, znear, real)
        return self.shade_final(sd, gbuffer0, gbuffer1, depth, shadow, real)


def load(directory):
    so32, so64 = (os.path.join(str(directory), "libshade_ref_%s.so" % k) for k in ("f32", "f64"))
    for so, extra in ((so32, []), (so64, ["-DREAL=double"])):
        if not os.path.exists(so):
            subprocess.check_call(["gcc"] + RR.FLAGS + extra + ["-Wall", "-Wno-unused-function", "-shared", "-fPIC", "-I", HERE, "-o", so, SRC, "-lm"])
    return ShadeRef(so32, so64)


def channels(words):
    """(..., 4) int64 R, G, B, A of R8G8B8A8 words"""
    w = np.asarray(words).view(np.uint32)
    return np.stack([(w >> np.uint32(8 * k)) & np.uint32(255) for k in range(4)], -1).astype(np.int64)


def test_inputs(w, h, seed=0):
    """The inputs of the parity tests for a w x h image: a depth plane with one step below and one above shadowblur's dgrad threshold
    of 0.1 in view-space distance, a block of sky (zeros), a few NaN / inf / negative / denormal depths, random shadow bytes and random
    G-buffer words with 0 and all ones among them.  Returns dict(depth (h, w) f32, shadow (h, w) u8, gbuffer0 / gbuffer1 (h, w) u32, znear)."""
    rng = np.random.default_rng(1000 * w + h + seed)
    znear = 0.1
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    # view-space distance: a tilted plane 4 .. 6 away, + 0.05 (below the threshold) right of 1/3, + 0.3 more (above it) right of 2/3
    dist = 4.0 + 1.5 * x / max(w - 1, 1) + 0.5 * y / max(h - 1, 1) + 0.05 * (x >= w // 3) + 0.3 * (x >= (2 * w) // 3)
    depth = (znear / dist).astype(np.float32)
    if w >= 5 and h >= 3:
        depth[h // 2:, : max(1, w // 4)] = 0.0  # sky
    flat = depth.reshape(-1)
    special = np.array([np.nan, np.inf, -np.inf, -0.02, 1e-40, -0.0], np.float32)
    if flat.size >= 16:
        where = rng.choice(flat.size, size=len(special), replace=False)
        flat[where] = special
    shadow = rng.integers(0, 256, (h, w)).astype(np.uint8)
    g0 = rng.integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)
    g1 = rng.integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)
    if flat.size >= 4:
        g0.reshape(-1)[[0, -1]] = (0, 0xFFFFFFFF)
        g1.reshape(-1)[[1, -2]] = (0xFFFFFFFF, 0)
    return dict(depth=depth, shadow=shadow, gbuffer0=g0, gbuffer1=g1, znear=znear)


def test_shade_data(w, h, shadows):
    """ShadeData of niagara's default camera moved off the origin, the sun above and in front"""
    from niagara_amd import host, synth
    cd = host.build_cull_data(cam_pos=(0.5, 1.0, 2.0), viewport=(w, h), pyramid=(host.previous_pow2(w), host.previous_pow2(h)))
    sun = np.array([0.3, 0.8, 0.52], np.float64)
    return host.build_shade_data(synth.make_globals(cd, (w, h)), (0.5, 1.0, 2.0), sun / np.linalg.norm(sun), shadows, w, h)


_FRAME = {}


def reference_frame(vref, aref):
    """The occluder scene at its own viewport through the CPU references (two closed-loop frames with the post pass, resolve, the attribute
    pass), computed once: dict(scene, cull, gbuffer0 / gbuffer1 (h, w) u32, depth (h, w) f32: the raster target the post pass leaves,
    shadow (h, w) u8: a synthetic mask (a disc of shadow over lit ground with a soft rim), camera, sun, sd: ShadeData with shadows on)"""
    if not _FRAME:
        import oracle
        import visattr_ref as VA
        from niagara_amd import host, synth
        s = VA.with_attributes(synth.occluder_scene(meshlet_bounds=oracle.meshlet_bounds))
        rec, out = VA.reference_frame(s, 0, vref, aref, frames=2)
        w, h = s["viewport"]
        x, y = np.meshgrid(np.arange(w), np.arange(h))
        r = np.hypot(x - 0.45 * w, y - 0.5 * h) / (0.3 * h)
        shadow = np.clip(np.rint(255.0 * np.clip((r - 0.8) / 0.4, 0.0, 1.0)), 0, 255).astype(np.uint8)
        camera, sun = (0.0, 0.0, 0.0), np.array([0.35, 0.6, 0.72]) / np.linalg.norm([0.35, 0.6, 0.72])
        sd = host.build_shade_data(synth.make_globals(s["cull"], (w, h)), camera, sun, 1, w, h)
        _FRAME.update(scene=s, cull=s["cull"], gbuffer0=out["gbuffer0"].reshape(h, w).copy(), gbuffer1=out["gbuffer1"].reshape(h, w).copy(),
                      depth=np.ascontiguousarray(rec["post"]["depth"], np.float32).reshape(h, w).copy(), shadow=shadow, camera=camera, sun=sun, sd=sd)
    return _FRAME


reference_frame.__test__ = False
test_inputs.__test__ = False
test_shade_data.__test__ = False
