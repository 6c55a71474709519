"""The shading end of the frame without a GPU: NvShadeData's layout, the exported symbols, and the rule set as
tests/shade_ref.c restates it — the gw table, constant images through both filters, sky pixels, the shadow term of the final pass, the fp32
build against the fp64 build within a derived bound, and nv_build_shade_data's inverse.

The accuracy bound is derived, not fitted: a running error analysis of the statements of final.comp.glsl.  With u = 2^-24, a value x carries a
bound e on |fp32 value - fp64 value|; x + y has e_x + e_y + u |x + y|, x y has |x| e_y + |y| e_x + e_x e_y + u |x y|, x / y has (e_x + |x / y| e_y) /
(|y| - e_y) + u |x / y|, sqrt the width of its image of [x - e, x + e] + u sqrt(x), max(x, 0) keeps e, exp2 has 2^x (2^e - 1) and pow(x, y) with
0 <= x <= 1, y >= 1 has y (x + e_x)^(y - 1) e_x + e_y / (e y) (the largest |x^y ln x| on (0, 1] is 1 / (e y)), both plus one fp32 ULP (2 u
relative) for glibc's powf / exp2f, whose documented error is below one ULP.  The one discontinuity of the pass, decodeOct's sign select, is
excluded where the bound cannot decide it (counted; there must be few)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import niagara_amd as N
import shade_ref as SR
import visattr_ref as VA
import visbuffer_ref as VB
from niagara_amd import host, synth
from niagara_amd import layouts as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (7, 5), (21, 3), (3, 21), (67, 37), (65, 5), (65, 17)]  # (65, 5) / (65, 17): the blur kernels' tiles (64 x 4, 64 x 16) + 1
U = 2.0 ** -24


@pytest.fixture(scope="session")
def sref(tmp_path_factory):
    return SR.load(tmp_path_factory.mktemp("shade_ref_cpu"))


@pytest.fixture(scope="session")
def vref(tmp_path_factory):
    return VB.load(tmp_path_factory.mktemp("visbuffer_ref_shade_cpu"))


@pytest.fixture(scope="session")
def aref(tmp_path_factory):
    return VA.load(tmp_path_factory.mktemp("visattr_ref_shade_cpu"))


def test_shade_data_layout_matches_the_header(tmp_path):
    fields = [n for n in L.SHADEDATA.names]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "niagara_vis.h"\nint main(void){printf("%zu", sizeof(NvShadeData));\n' +
                   "".join('printf(" %%zu", offsetof(NvShadeData, %s));\n' % f for f in fields) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == L.SHADEDATA.itemsize == 112
    assert got[1:] == [L.SHADEDATA.fields[f][1] for f in fields]
    assert [L.SHADEDATA.fields[f][1] for f in ("sunDirection", "shadowsEnabled", "inverseViewProjection", "imageSize")] == [16, 28, 32, 96]


def test_library_exports_the_shading_entry_points():
    """the cross-compiled library, loaded without a GPU as tests/test_layouts_abi.py loads it; argument checks need no device"""
    for name in ("nv_shadow_fill", "nv_shadow_blur", "nv_shade_final", "nv_build_shade_data"):
        assert name in N.EXPORTS and hasattr(N.lib, name), name
    assert N.lib.nv_shadow_fill(None, None, None, None, 4, 4, 0) == -1
    assert N.lib.nv_shadow_blur(None, None, None, None, None, 4, 4, 1, 0.1) == -1
    assert N.lib.nv_shade_final(None, None, None, None, None, None, None, None, 4, 4) == -1
    assert N.lib.nv_build_shade_data(None, None, None, None, 0, 4, 4) == -1
    with pytest.raises(N.NvError):  # a singular product
        host.build_shade_data(np.zeros(1, L.GLOBALS), width=4, height=4)


def test_gw_table_is_the_shaders_integer_arithmetic(sref):
    want = [1.0] * 7 + [0.5, 0.5, 0.25]
    assert sref.gw("f32").tolist() == want and sref.gw("f64").tolist() == want
    assert [2.0 ** int(-i * i / 50) for i in range(1, 11)] == want  # int() truncates toward zero, as GLSL's integer division does


@pytest.mark.parametrize("size", SIZES)
def test_blur_of_a_constant_image_is_that_constant(size, sref):
    w, h = size
    rng = np.random.default_rng(w * 100 + h)
    depth = rng.uniform(1e-3, 1.0, (h, w)).astype(np.float32)  # any finite positive depth
    for code in (0, 1, 127, 254, 255):
        shadow = np.full((h, w), code, np.uint8)
        for direction in (0, 1):
            for real in ("f32", "f64"):
                assert (sref.shadow_blur(shadow, depth, direction, 0.1, real) == code).all(), (code, direction, real)


@pytest.mark.parametrize("size", SIZES)
def test_fill_of_a_constant_image_over_constant_depth_loses_what_the_denominator_says(size, sref):
    """every in-range neighbour has weight exp2(0) = 1, every neighbour outside the image depth 0, weight exp2(-20) and shadow 0:
    shadow' = k s / (k + (4 - k) 2^-20 + 1e-2) with k in-range neighbours — below s, by the + 1e-2 of shadowfill.comp.glsl:43"""
    w, h = size
    depth = np.full((h, w), 0.37, np.float32)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    k = (x > 0).astype(np.int64) + (x < w - 1) + (y > 0) + (y < h - 1)
    for code in (0, 3, 128, 255):
        shadow = np.full((h, w), code, np.uint8)
        want = np.rint(255.0 * (k * (code / 255.0)) / (k + (4 - k) * 2.0 ** -20 + float(np.float32(1e-2)))).astype(np.int64)
        for cb in (0, 1):
            owned = (~(y ^ cb) & 1) == (x & 1)
            for real in ("f32", "f64"):
                got = sref.shadow_fill(shadow, depth, cb, real).astype(np.int64)
                assert (got[~owned] == code).all()  # the other parity keeps its bytes
                assert np.abs(got[owned] - want[owned]).max(initial=0) <= 1, (code, cb, real)
        if code == 255 and w > 2 and h > 2:
            assert want[1, 1] == 254  # 255 * 4 / 4.01 = 254.36: the fill darkens a lit interior by one code


def test_sky_pixels_shade_to_tonemap_of_zero_plus_deband(sref):
    """depth 0: wposh.w == 0, view is NaN, max(dot, 0) keeps the NaN and tonemap's max(0, c - 0.004) ends it: the value handed to the store is
    exactly tonemap(0) = 0 plus the deband term — whatever the G-buffer words hold"""
    w, h = 37, 11
    rng = np.random.default_rng(3)
    depth = np.zeros((h, w), np.float32)
    g0 = rng.integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)
    g1 = rng.integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)
    g0[0, :8], g1[0, :8] = 0, 0
    shadow = rng.integers(0, 256, (h, w)).astype(np.uint8)
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    inner = x * np.float32(0.06711056) + y * np.float32(0.00583715)
    n1 = np.float32(52.9829189) * (inner - np.floor(inner))
    band = ((n1 - np.floor(n1)) * np.float32(2.0) - np.float32(1.0)) * (np.float32(0.5) / np.float32(255.0))
    assert band.dtype == np.float32
    for shadows in (0, 1):
        sd = SR.test_shade_data(w, h, shadows)
        assert sd["inverseViewProjection"][0][[3, 7, 15]].tolist() == [0.0, 0.0, 0.0]  # the w row is (0, 0, 1 / znear, 0)
        for real in ("f32", "f64"):
            color, value = sref.shade_final(sd, g0, g1, depth, shadow if shadows else None, real, value=True)
            assert (value[..., :3] == 0.0).all() and not np.isnan(value).any()
            if real == "f32":
                assert value[..., 3].astype(np.float32).tobytes() == band.tobytes()
            want = np.rint(np.clip(band.astype(np.float64), 0.0, 1.0) * 255.0).astype(np.int64)  # 0 everywhere: |band| <= 0.5 / 255
            ch = SR.channels(color)
            assert (ch[..., :3] == want[..., None]).all() and (ch[..., 3] == 255).all()


def test_a_lit_pixel_and_a_shadowed_one_differ_as_the_formula_says(sref):
    """normal codes (511, 511): n ~ (0, 0, 1); sun = (0, 0, 1); gloss 0 and emissive 0 leave albedo * (ndotl * min(shadow + 0.05, 1) * 2.5 + 0.07)"""
    w, h = 4, 3
    cd = host.build_cull_data(viewport=(w, h), pyramid=(2, 2))
    sd = host.build_shade_data(synth.make_globals(cd, (w, h)), (0, 0, 0), (0, 0, 1), 1, w, h)
    g0 = np.full((h, w), 200 | 150 << 8 | 90 << 16, np.uint32)
    g1 = np.full((h, w), 511 | 511 << 10, np.uint32)
    depth = np.full((h, w), 0.02, np.float32)
    e = 511.0 / 1023.0 * 2.0 - 1.0
    n = np.array([e, e, 1.0 - 2.0 * abs(e)])
    ndotl = (n / np.linalg.norm(n))[2]
    albedo = (np.array([200, 150, 90]) / 255.0) ** float(np.float32(2.2))

    def tonemap(c):
        x = np.maximum(0.0, c - float(np.float32(0.004)))
        return (x * (float(np.float32(6.2)) * x + 0.5)) / (x * (float(np.float32(6.2)) * x + float(np.float32(1.7))) + float(np.float32(0.06)))
    got = {}
    for code in (255, 0):
        s = code / 255.0
        want = tonemap(albedo * (ndotl * min(s + float(np.float32(0.05)), 1.0) * 2.5 + float(np.float32(0.07))))
        for real, tol in (("f32", 2e-6), ("f64", 1e-12)):
            color, value = sref.shade_final(sd, g0, g1, depth, np.full((h, w), code, np.uint8), real, value=True)
            assert np.abs(value[..., :3] - want).max() < tol, (code, real)
            got[code, real] = SR.channels(color)[..., :3]
            assert np.abs(got[code, real] - np.rint((want + value[..., 3:4]) * 255.0)).max() <= 1
    assert (got[255, "f32"] > got[0, "f32"] + 50).all()  # the sun term: 2.5 ndotl against 0.125 ndotl under the tonemap


# ---- the fp32 build against the fp64 build: the running error analysis of the module docstring

class V:
    def __init__(self, v, e=0.0):
        self.v, self.e = np.asarray(v, np.float64), np.broadcast_to(np.asarray(e, np.float64), np.shape(v)).copy()

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(np.float64(np.float32(x)))  # a constant of the shader: its fp32 value, exact in both builds

    def _r(self, v, e0):
        return V(v, e0 + U * (np.abs(v) + e0))

    def __add__(self, o):
        o = V.of(o)
        return self._r(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = V.of(o)
        return self._r(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return V.of(o) - self

    def __neg__(self):
        return V(-self.v, self.e)

    def __mul__(self, o):
        o = V.of(o)
        return self._r(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    def __truediv__(self, o):
        o = V.of(o)
        q = self.v / o.v
        room = np.abs(o.v) - o.e
        return self._r(q, np.where(room > 0, (self.e + np.abs(q) * o.e) / np.where(room > 0, room, 1.0), np.inf))

    def sqrt(self):
        return self._r(np.sqrt(self.v), np.sqrt(self.v + self.e) - np.sqrt(np.maximum(self.v - self.e, 0.0)))

    def abs(self):
        return V(np.abs(self.v), self.e)

    def max0(self):
        return V(np.maximum(self.v, 0.0), self.e)

    def min1(self):
        return V(np.minimum(self.v, 1.0), self.e)

    def exp2(self):
        v = 2.0 ** self.v
        e0 = v * (2.0 ** self.e - 1.0)
        return V(v, e0 + 2 * U * (v + e0))

    def pow(self, y):
        y = V.of(y)
        v = self.v ** y.v
        e0 = (y.v + y.e) * (self.v + self.e) ** (y.v - y.e - 1.0) * self.e + y.e / (np.e * (y.v - y.e))
        return V(v, e0 + 2 * U * (v + e0))


def _normalize(a):
    l = ((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]).sqrt()
    return [a[0] / l, a[1] / l, a[2] / l]


def final_bound(sd, g0, g1, depth, shadow):
    """(tonemap(outputColor) (n, 3) by the analysis' fp64 values, its bound (n, 3), undecided (n): decodeOct's select cannot be bounded)"""
    h, w = depth.shape
    sd = sd[0]
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    x, y, g0, g1 = x.reshape(-1), y.reshape(-1), g0.reshape(-1).astype(np.int64), g1.reshape(-1).astype(np.int64)
    f8 = lambda k: V(((g0 >> (8 * k)) & 255).astype(np.float64)) / 255.0
    f10 = lambda k: V(((g1 >> (10 * k)) & 1023).astype(np.float64)) / 1023.0
    sun = [V(np.full(len(x), np.float64(c))) for c in sd["sunDirection"]]
    cam = [V(np.full(len(x), np.float64(c))) for c in sd["cameraPosition"]]
    m = sd["inverseViewProjection"].astype(np.float64)
    albedo = [f8(k).pow(2.2) for k in range(3)]
    e = (f8(3) * 5.0).exp2() - 1.0
    emissive = [a * e for a in albedo]
    ex, ey = f10(0) * 2.0 - 1.0, f10(1) * 2.0 - 1.0
    vz = (1.0 - ex.abs()) - ey.abs()
    t = (-vz).max0()
    undecided = ((np.abs(ex.v) <= ex.e) | (np.abs(ey.v) <= ey.e)) & (t.v + t.e > 0)
    vx = ex + V(np.where(ex.v >= 0, -t.v, t.v), t.e)
    vy = ey + V(np.where(ey.v >= 0, -t.v, t.v), t.e)
    normal = _normalize([vx, vy, vz])
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    ndotl = dot(normal, sun).max0()
    uvx, uvy = (V(x) + 0.5) / float(sd["imageSize"][0]), (V(y) + 0.5) / float(sd["imageSize"][1])
    clip = [uvx * 2.0 - 1.0, 1.0 - uvy * 2.0, V(depth.reshape(-1).astype(np.float64)), V(np.ones(len(x)))]
    wposh = [((V(np.full(len(x), m[r])) * clip[0] + V(np.full(len(x), m[4 + r])) * clip[1]) + V(np.full(len(x), m[8 + r])) * clip[2]) +
             V(np.full(len(x), m[12 + r])) * clip[3] for r in range(4)]
    view = _normalize([cam[k] - wposh[k] / wposh[3] for k in range(3)])
    halfv = _normalize([view[k] + sun[k] for k in range(3)])
    ndoth = dot(normal, halfv).max0()
    gloss = f10(2)
    ndoth = V(np.minimum(ndoth.v, 1.0), ndoth.e)  # (a unit dot product: the analysis' pow takes x in [0, 1]; x + e may pass 1 by e)
    specular = ndoth.pow(V.of(1.0) * (1.0 - gloss) + V.of(64.0) * gloss) * gloss
    sh = V(shadow.reshape(-1).astype(np.float64)) / 255.0
    lit = (ndotl * (sh + 0.05).min1()) * 2.5 + 0.07
    spec = (specular * sh) * 2.5
    out_v, out_e = [], []
    for k in range(3):
        o = ((albedo[k] * lit + spec) + emissive[k]) + 0.0
        c = (o - 0.004).max0()
        tm = (c * (c * 6.2 + 0.5)) / (c * (c * 6.2 + 1.7) + 0.06)
        out_v.append(tm.v), out_e.append(tm.e)
    return np.stack(out_v, -1), np.stack(out_e, -1), undecided


def test_fp32_build_stays_within_the_derived_bound_of_the_fp64_build(sref, vref, aref):
    """final.comp.glsl on the occluder frame (the end-to-end case of tests/test_shade_gpu.py) with its blurred shadow mask as an input: every
    geometry pixel's tonemap(outputColor) of the fp32 build lies within the running-error bound of the fp64 build's"""
    f = SR.reference_frame(vref, aref)
    znear = float(f["cull"]["znear"][0])
    shadow = sref.shadow_blur(sref.shadow_blur(f["shadow"], f["depth"], 1, znear), f["depth"], 0, znear)
    _, v32 = sref.shade_final(f["sd"], f["gbuffer0"], f["gbuffer1"], f["depth"], shadow, "f32", value=True)
    _, v64 = sref.shade_final(f["sd"], f["gbuffer0"], f["gbuffer1"], f["depth"], shadow, "f64", value=True)
    with np.errstate(all="ignore"):
        val, bound, undecided = final_bound(f["sd"], f["gbuffer0"], f["gbuffer1"], f["depth"], shadow)
    geo = (f["depth"].reshape(-1) > 0) & ~undecided
    assert geo.sum() > 1000 and (f["depth"] == 0).sum() > 1000 and undecided.sum() < 0.01 * undecided.size
    a, b = v32[..., :3].reshape(-1, 3)[geo].astype(np.float64), v64[..., :3].reshape(-1, 3)[geo]
    assert np.abs(val[geo] - b).max() < 1e-9  # the analysis evaluates the statements the fp64 build evaluates
    err, bnd = np.abs(a - b), bound[geo]
    print("final: %d geometry pixels, fp32 - fp64 error / bound <= %.3f (largest error %.3g, median bound %.3g, largest bound %.3g)"
          % (int(geo.sum()), float((err / bnd).max()), float(err.max()), float(np.median(bnd)), float(bnd.max())))
    assert (err <= bnd).all()
    assert np.median(bnd) < 0.05 / 255.0  # the bound says something: a twentieth of a code


def test_perturbed_pow_and_exp2_stay_inside_the_gpu_tests_conditions(sref):
    """the GPU comparison allows one code and asks for 90 % equal channels because the device's and glibc's pow / exp2 differ by a few ULP:
    moving every such result of the restatement by 2 ULP, up, down or mixed, on the GPU tests' own inputs must stay inside both"""
    try:
        for w, h in SIZES:
            i = SR.test_inputs(w, h)
            sd = SR.test_shade_data(w, h, 1)
            base = dict(fill0=sref.shadow_fill(i["shadow"], i["depth"], 0), fill1=sref.shadow_fill(i["shadow"], i["depth"], 1),
                        blur0=sref.shadow_blur(i["shadow"], i["depth"], 0, i["znear"]), blur1=sref.shadow_blur(i["shadow"], i["depth"], 1, i["znear"]),
                        final=SR.channels(sref.shade_final(sd, i["gbuffer0"], i["gbuffer1"], i["depth"], i["shadow"])))
            for mode in (1, 2, 3):
                sref.perturb(mode, 2)
                got = dict(fill0=sref.shadow_fill(i["shadow"], i["depth"], 0), fill1=sref.shadow_fill(i["shadow"], i["depth"], 1),
                           blur0=sref.shadow_blur(i["shadow"], i["depth"], 0, i["znear"]), blur1=sref.shadow_blur(i["shadow"], i["depth"], 1, i["znear"]),
                           final=SR.channels(sref.shade_final(sd, i["gbuffer0"], i["gbuffer1"], i["depth"], i["shadow"])))
                sref.perturb(0)
                for k in base:
                    d = np.abs(got[k].astype(np.int64) - base[k].astype(np.int64))
                    assert d.max() <= 1, (w, h, mode, k)
                    assert (d == 0).mean() >= 0.9, (w, h, mode, k, float((d == 0).mean()))
    finally:
        sref.perturb(0)


@pytest.mark.parametrize("camera", [((0, 0, 0), (0, 0, 0, 1)), ((3.0, -2.0, 11.0), (0.1, 0.7, -0.2, 0.68)), ((-40.0, 5.0, 0.25), (0.5, 0.5, 0.5, 0.5))])
def test_build_shade_data_inverts_projection_times_view(camera):
    """M = fl32(inverse(P V)): every entry is off by at most u |entry| from the fp64 inverse, so |M (P V) - I| <= u (|M| |P V|) entry by entry,
    plus the fp64 inverse's own error, kappa 2^-53 relative with kappa(P V) < 1e6 for these cameras: below 1e-9 (|M| |P V|)"""
    pos, quat = camera
    q = np.array(quat, np.float64) / np.linalg.norm(quat)
    w, h = 320, 192
    cd = host.build_cull_data(cam_pos=pos, cam_quat=q, viewport=(w, h), pyramid=(256, 128))
    g = synth.make_globals(cd, (w, h))
    sd = host.build_shade_data(g, pos, (0, 1, 0), 0)
    assert sd["imageSize"][0].tolist() == [w, h] and sd["shadowsEnabled"][0] == 0 and sd["cameraPosition"][0].tolist() == list(np.float32(pos))
    P = g["projection"][0].astype(np.float64).reshape(4, 4).T  # column-major
    Vw = g["cullData"][0]["view"].astype(np.float64).reshape(4, 4).T
    A = P @ Vw
    assert np.linalg.cond(A) < 1e6
    M = sd["inverseViewProjection"][0].astype(np.float64).reshape(4, 4).T
    bound = (U + 1e-9) * (np.abs(M) @ np.abs(A))
    err = np.abs(M @ A - np.eye(4))
    print("inverse: error / bound <= %.3f" % float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound + 1e-300).all()
