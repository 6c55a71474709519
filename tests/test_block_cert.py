"""The margin of the filter form's block test (filtermath.h block_record / block_planes / block_outside, clustercull.hip BLOCK), checked on
the CPU against the compiled header (tests/block_shim.cpp) in the style of tests/test_cert_margins.py:

    block_outside(draw, block)  =>  certainly_outside<FOLD> holds for every meshlet of the block  =>  the reference rejects every one of them,

in bulk with fp64-emulated FMAs, for a sample in exact rational arithmetic, over test_cert_margins's scene classes (non-unit quaternions,
large positions and scales, tiny scenes) plus pools with fp16 extremes (+-65504, subnormals) and zero radii; and the records themselves:
the centre inside the block's box, every meshlet sphere inside (C, D, rho) in exact arithmetic, non-finite and empty blocks never rejecting."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import oracle
from test_cert_margins import CASES, filters_of, fma64, pool_bounds, rn32, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _build(tmp, name):
    so = str(tmp / (name + ".so"))
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(ROOT, "tests", name + ".cpp"), "-o", so], check=True)
    return C.CDLL(so)


@pytest.fixture(scope="module")
def shims(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("block")
    blk = _build(tmp, "block_shim")
    blk.shim_block_records.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_void_p]
    blk.shim_half_up.restype = C.c_uint32
    blk.shim_half_up.argtypes = [C.c_double]
    blk.shim_block_outside.argtypes = [C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    cert = _build(tmp, "cert_shim")
    cert.shim_filter_k.restype = C.c_float
    cert.shim_filter_k.argtypes = [C.c_void_p, C.c_float, C.c_float]
    cert.shim_make_filters.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_float, C.c_float, C.c_float, C.c_void_p]
    return blk, cert


def records(blk, meshlets):
    words = np.ascontiguousarray(np.stack([meshlets["center"][:, 0].astype(np.uint32) | meshlets["center"][:, 1].astype(np.uint32) << 16,
                                           meshlets["center"][:, 2].astype(np.uint32) | meshlets["radius"].astype(np.uint32) << 16], axis=1))
    nb = (len(meshlets) + 63) // 64 + 1  # the mirror's blocks, the padding block included
    out = np.zeros((nb, 4), np.uint32)
    blk.shim_block_records(words.ctypes.data, len(meshlets), nb, out.ctypes.data)
    return out


def half(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float64)


def test_half_up_is_the_smallest_half_above(shims):
    blk, _ = shims
    rng = np.random.default_rng(1)
    xs = np.concatenate([rng.uniform(0, 1, 2000) * 10.0 ** rng.integers(-9, 5, 2000), half(np.arange(0, 0x7c00, 37)), [0.0, 65504.0, 65504.5, 1e9]])
    for x in xs:
        h = blk.shim_half_up(float(x))
        v = float(half(h)) if h < 0x7c00 else np.inf
        assert v >= x, (x, h)
        if h > 0:
            assert float(half(h - 1)) < x, (x, h)  # the next smaller half is below x


def special_pool(n, seed):
    """meshlets with fp16 extremes: +-65504 centres, subnormals, zero radii, blocks of tight clusters; a few NaN / inf blocks"""
    from niagara_amd import synth
    rng = np.random.default_rng(seed)
    m = synth.make_meshlets(n, seed=seed)
    cen = m["center"]
    for b in range(0, n // 64, 5):
        i = b * 64 + rng.integers(0, 64, 4)
        cen[i, rng.integers(0, 3)] = rng.choice([0x7bff, 0xfbff, 0x0001, 0x8001, 0x03ff], 4)
    m["radius"][rng.integers(0, n, n // 10)] = 0
    tight = rng.uniform(-1, 1, (n // 64, 3))
    for b in range(1, n // 64, 7):
        v = tight[b] + 1e-3 * rng.standard_normal((64, 3))
        cen[b * 64:b * 64 + 64] = v.astype(np.float16).view(np.uint16)
    for b, bits in ((3, 0x7e00), (11, 0x7c00), (19, 0xfc00)):
        cen[b * 64 + 7, 1] = bits
    m["radius"][25 * 64 + 3] = 0x7c00
    return m


@pytest.mark.parametrize("pool", ["synthetic", "extremes"])
def test_records_bound_every_meshlet(shims, pool):
    from niagara_amd import synth
    blk, _ = shims
    m = synth.make_meshlets(64 * 200 + 17, seed=3) if pool == "synthetic" else special_pool(64 * 120, 4)
    tab = records(blk, m)
    cnt = len(m)
    for b, rec in enumerate(tab):
        lo, hi = b * 64, min(cnt, b * 64 + 64)
        dbits, rbits = int(rec[3]) & 0xffff, int(rec[3]) >> 16
        h = np.concatenate([m["center"][lo:hi].ravel(), m["radius"][lo:hi]])
        if hi <= lo or ((h & 0x7c00) == 0x7c00).any():
            assert dbits == 0x7c00 and rbits == 0x7c00, b
            continue
        Cf = rec[:3].view(np.float32).astype(np.float64)
        v = half(m["center"][lo:hi].ravel()).reshape(-1, 3)
        assert ((v.min(axis=0) <= Cf) & (Cf <= v.max(axis=0))).all(), b
        assert float(half(rbits)) >= np.abs(half(m["radius"][lo:hi])).max(), b
        if dbits == 0x7c00:  # a block spanning more than 65504 (fp16 extremes): D rounds up to inf, which bounds anything
            continue
        D = Fraction(float(half(dbits)))
        Cx = [Fraction(float(x)) for x in Cf]
        for i in range(len(v)):  # exact rationals
            assert sum((Fraction(float(v[i, j])) - Cx[j]) ** 2 for j in range(3)) <= D * D, (b, i)
    # the records are tight enough to be useful: D within 2^-10 of the largest exact distance (fp16 rounding upward) on ordinary blocks
    if pool == "synthetic":
        b = 5
        v = half(m["center"][b * 64:b * 64 + 64].ravel()).reshape(-1, 3)
        dmax = np.sqrt(((v - tab[b, :3].view(np.float32).astype(np.float64)) ** 2).sum(axis=1)).max()
        assert float(half(int(tab[b, 3]) & 0xffff)) <= dmax * (1 + 2.0 ** -10)


def fold_rows(F, fr):
    """what the kernel's block test and filter loop read: the side rows folded with the plane coefficients (one fp32 rounding each)"""
    m, b = F[:, 0:9], F[:, 9:12]
    rows = np.zeros((len(F), 14), f32)
    rows[:, 0:3] = (fr[0] * m[:, 0:3]).astype(f32)
    rows[:, 3] = (fr[0] * b[:, 0]).astype(f32)
    rows[:, 4:7] = (fr[2] * m[:, 3:6]).astype(f32)
    rows[:, 7] = (fr[2] * b[:, 1]).astype(f32)
    rows[:, 8:11] = m[:, 6:9]
    rows[:, 11] = b[:, 2]
    rows[:, 12] = F[:, 15]  # scale
    rows[:, 13] = F[:, 18]  # tK
    return rows


SCENES = CASES + [("fp16 extremes in the pool", 300.0, 1.0, 1.0, (0, 0, 0), (0, 0, 0, 1))]


@pytest.mark.parametrize("case", SCENES, ids=[c[0] for c in SCENES])
def test_block_outside_implies_filter_and_reference_reject(shims, case):
    blk, cert = shims
    name, radius, scale_mul, qmul, cam, camq = case
    draws, meshlets, commands, cd = scene(radius, scale_mul, qmul, cam, camq, n_draws=400, cpd=2, seed=11)
    if name.startswith("fp16"):
        sp = special_pool(len(meshlets), 8)
        meshlets["center"], meshlets["radius"] = sp["center"], sp["radius"]
    n = len(commands)
    tab = records(blk, meshlets)
    fr = cd["frustum"][0].astype(f32)
    znear, zfar = f32(cd["znear"][0]), f32(cd["zfar"][0])
    filterK, F = filters_of(cert, cd, draws, *pool_bounds(meshlets))
    assert filterK > 0
    d = commands["drawId"]
    off = commands["taskOffset"].astype(np.int64)
    assert (off % 64 == 0).all()
    rows = np.ascontiguousarray(fold_rows(F, fr)[d])
    recs = np.ascontiguousarray(tab[off // 64])
    plane = np.array([fr[1], fr[3], znear, zfar], f32)
    out = np.zeros(n, np.int32)
    blk.shim_block_outside(n, rows.ctypes.data, plane.ctypes.data, recs.ctypes.data, out.ctypes.data)
    out = out.astype(bool)
    # the filter loop's decision per meshlet (clustercull.hip certainly_outside<true>, FMA = fp64 product-sum rounded to fp32)
    ml = meshlets[off[:, None] + np.arange(64)[None, :]]
    v = half(ml["center"].ravel()).reshape(n, 64, 3).astype(f32)
    rad = half(ml["radius"]).astype(f32)
    R = np.broadcast_to(rows[:, None, :], (n, 64, 14))
    cs = [fma64(R[..., 4 * k], v[..., 0], fma64(R[..., 4 * k + 1], v[..., 1], fma64(R[..., 4 * k + 2], v[..., 2], R[..., 4 * k + 3]))) for k in range(2)]
    cz = fma64(R[..., 8], v[..., 0], fma64(R[..., 9], v[..., 1], fma64(R[..., 10], v[..., 2], R[..., 11])))
    with np.errstate(invalid="ignore", over="ignore"):
        g = np.fmin(np.fmin(fma64(cz, fr[1], -np.abs(cs[0])), fma64(cz, fr[3], -np.abs(cs[1]))), np.fmin(cz - znear, zfar - cz))
        filt = g < -fma64(R[..., 12], rad, R[..., 13])
    assert filt[out].all(), "%s: a block said outside holds a meshlet the filter keeps" % name
    probe = oracle.probe_cluster_scalars(cd, commands, draws, meshlets)
    vis_ref = probe[..., 14] != 0
    assert not vis_ref[out].any(), "%s: a block said outside holds a meshlet the reference keeps" % name
    # and it must finish most of what the filter finishes (the point of it), where the blocks are not degenerate
    filt_cmd = filt.all(axis=1)
    if name.startswith("config 3A") or name.startswith("dense"):
        assert out.sum() >= 0.5 * filt_cmd.sum(), (name, int(out.sum()), int(filt_cmd.sum()))
    # ---- a sample in exact rational arithmetic: every FMA = the exact a b + c rounded once to fp32
    rng = np.random.default_rng(5)
    idx = np.nonzero(out)[0]
    for ci in rng.choice(idx, min(24, len(idx)), replace=False) if len(idx) else []:
        r = [Fraction(float(x)) for x in rows[ci]]
        f1, f3, zn, zf = (Fraction(float(x)) for x in plane)
        for li in rng.integers(0, 64, 4):
            vx, vy, vz, rr = (Fraction(float(x)) for x in (*v[ci, li], rad[ci, li]))
            if not all(np.isfinite([float(vx), float(vy), float(vz), float(rr)])):
                continue
            ch = lambda k: rn32(r[4 * k] * vx + rn32(r[4 * k + 1] * vy + rn32(r[4 * k + 2] * vz + r[4 * k + 3])))  # noqa: E731
            czz = rn32(r[8] * vx + rn32(r[9] * vy + rn32(r[10] * vz + r[11])))
            gs = [rn32(czz * f1 - abs(ch(0))), rn32(czz * f3 - abs(ch(1))), rn32(czz - zn), rn32(zf - czz)]
            thr = rn32(r[12] * rr + r[13])
            assert min(gs) < -thr, (name, ci, li)


def test_non_finite_never_rejects(shims):
    """D = inf records, tK = inf / NaN draws: never outside"""
    blk, _ = shims
    rows = np.zeros((4, 14), f32)
    rows[:, 0] = rows[:, 4] = rows[:, 10] = 1.0
    rows[:, 11] = -1e6  # far behind the near plane
    rows[:, 12] = 1.0
    rows[:, 13] = [1e-3, np.inf, np.nan, 1e-3]
    recs = np.zeros((4, 4), np.uint32)
    recs[:, 3] = [0x7c00 | 0x7c00 << 16, 0, 0, 0x7c00]
    plane = np.array([0.6, 0.6, 0.1, 100.0], f32)
    out = np.zeros(4, np.int32)
    blk.shim_block_outside(4, rows.ctypes.data, plane.ctypes.data, recs.ctypes.data, out.ctypes.data)
    assert list(out) == [0, 0, 0, 0]
    recs[:, 3] = 0  # finite: the first row is outside
    blk.shim_block_outside(4, rows.ctypes.data, plane.ctypes.data, recs.ctypes.data, out.ctypes.data)
    assert list(out) == [1, 0, 0, 1]
