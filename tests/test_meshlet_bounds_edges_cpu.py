"""SURVEY.md §8(f) N2 at its edges, on the CPU: orc_meshlet_bounds against a second restatement (tests/bounds_ref.py, plain
Python over float32 scalars) on the named cases of tests/bounds_cases.py — count clamps, the index mask, reference widths and
alignments, compaction, ties, long growth passes, mindp next to 0.1f, the s8 clamp, fp16 ties / flush / saturation and
non-finite vertices — byte for byte, records and floats; containment of the finite cases in exact rationals; the oracle's
quantiser against IEEE rounding and its three documented deviations; and a stand-alone sanitised program over all cases."""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import oracle
from niagara_amd import layouts as L

import bounds_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    meshlets, data, vertices, names = C.build()
    return meshlets, data, vertices, names


@pytest.fixture(scope="module")
def run(cases):
    """the oracle over all cases, once: (records, floats)"""
    meshlets, data, vertices, _ = cases
    out = meshlets.copy()
    f = oracle.meshlet_bounds(vertices, data, out, want_float=True)
    out.setflags(write=False)
    f.setflags(write=False)
    return out, f


def _show(names, k, got, want):
    return "%s (meshlet %d)\n  oracle   %s\n  restated %s" % (names[k], k, bytes(got).hex(" ", 4), bytes(want).hex(" ", 4))


def test_every_group_reached_its_condition():
    reached = C.conditions()
    for key in sorted(reached):
        print("%s: %s" % (key, reached[key]))
    assert reached["meshlets"] >= 2000 and set(C.groups()) == {"counts", "references", "compaction", "ties", "growth", "cone", "quantiser", "non-finite", "random"}


def test_oracle_equals_the_second_restatement_byte_for_byte(cases, run):
    """records (bytes 0..11) and the eight floats, NaNs compared as bits: both sides store the canonical quiet NaN"""
    names, ref = cases[3], C.reference()
    out, f = run
    rec = out.view(np.uint8).reshape(-1, 24)
    bad = []
    for k, d in enumerate(ref):
        if rec[k, :12].tobytes() != d["rec"].tobytes():
            bad.append(_show(names, k, rec[k, :12], d["rec"]))
        if f[k].tobytes() != d["f8"].tobytes():
            bad.append(_show(names, k, f[k].view(np.uint8), d["f8"].view(np.uint8)))
    assert not bad, "%d differences\n%s" % (len(bad), "\n".join(bad[:20]))


def test_inputs_are_left_alone_and_the_prefill_does_not_matter(cases, run):
    meshlets, data, vertices, _ = cases
    out, f = run
    assert (out.view(np.uint8).reshape(-1, 24)[:, 12:] == meshlets.view(np.uint8).reshape(-1, 24)[:, 12:]).all()
    zeroed = meshlets.copy()
    zeroed.view(np.uint8).reshape(-1, 24)[:, :12] = 0
    f0 = oracle.meshlet_bounds(vertices, data, zeroed, want_float=True)
    assert zeroed.tobytes() == out.tobytes() and f0.tobytes() == f.tobytes()
    again = out.copy()
    oracle.meshlet_bounds(vertices, data, again)
    assert again.tobytes() == out.tobytes()


# ---- exact rationals
def _sqrt_bounds(x, bits=96):
    """rationals (lo, hi) with lo <= sqrt(x) <= hi, hi - lo = 2^-bits / denominator"""
    x = Fraction(x)
    assert x >= 0
    n = math.isqrt(x.numerator * x.denominator << (2 * bits))
    den = x.denominator << bits
    return Fraction(n, den), Fraction(n + 1, den)


def _ge_scaled_root(x, c, n):
    """x >= c * sqrt(n) for rationals x, c and n >= 0"""
    if c >= 0:
        return x >= 0 and x * x >= c * c * n
    return x >= 0 or x * x <= c * c * n


def test_finite_cases_contain_their_geometry_in_exact_rationals(cases, run):
    """the tolerances of test_sphere_and_cone_contain_the_geometry, evaluated without rounding: every kept corner inside the
    float sphere, every kept normal inside the float cone, the s8 cone conservative against the float cone"""
    meshlets, data, vertices, names = cases
    out, f = run
    ref = C.reference()
    rng = np.random.default_rng(8)
    checked = cones = 0
    for k, d in enumerate(ref):
        finite = np.isfinite(f[k]).all() and all(np.isfinite(p).all() for p in d["corners"])
        if not finite or not d["kept"]:
            continue
        checked += 1
        c, r = [Fraction(float(x)) for x in f[k, :3]], Fraction(float(f[k, 3]))
        axis, cutoff = [Fraction(float(x)) for x in f[k, 4:7]], Fraction(float(f[k, 7]))
        bound = r * (1 + Fraction("1e-5")) + Fraction("1e-7")
        corners = [[Fraction(float(x)) for x in p] for p in d["corners"]]
        for p in corners:
            assert sum((p[a] - c[a]) ** 2 for a in range(3)) <= bound * bound, names[k]
        aq = [Fraction(int(x), 127) for x in out[k]["cone_axis"]]
        cutq = Fraction(int(out[k]["cone_cutoff"]), 127)
        if cutoff < 1:
            cones += 1
            mindp_hi = _sqrt_bounds(max(Fraction(0), 1 - cutoff * cutoff))[1]
            for t in range(d["kept"]):
                p0, p1, p2 = corners[3 * t:3 * t + 3]
                u, v = [p1[a] - p0[a] for a in range(3)], [p2[a] - p0[a] for a in range(3)]
                n = [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
                dot, lo_hi = sum(n[a] * axis[a] for a in range(3)), _sqrt_bounds(sum(x * x for x in n))
                cos_lo = dot / (lo_hi[1] if dot >= 0 else lo_hi[0])
                assert cos_lo + Fraction("1e-5") >= mindp_hi, names[k]                      # n . axis >= mindp - 1e-5
            a2 = sum(x * x for x in axis)
            assert (1 - Fraction("1e-5")) ** 2 < a2 < (1 + Fraction("1e-5")) ** 2, names[k]
            assert cutoff <= cutq <= 1, names[k]
            # the 8-bit test culls only what the float cone culls: dot(d, aq) >= cutq |d|  =>  dot(d, axis) >= (cutoff - 1e-6) |d|
            a8 = [int(x) for x in out[k]["cone_axis"]]
            dirs = [[int(x) for x in rng.integers(-60, 61, 3)] for _ in range(24)] + [a8]
            # and directions on both sides of the 8-bit cone's boundary: a8 |p|^2 s + p t with t / s close to tan(acos(cutq)) |a8| |p|
            if 0 < cutq < 1:
                for _ in range(8):
                    w = [int(x) for x in rng.integers(-9, 10, 3)]
                    p = [a8[1] * w[2] - a8[2] * w[1], a8[2] * w[0] - a8[0] * w[2], a8[0] * w[1] - a8[1] * w[0]]  # perpendicular to a8
                    p2 = sum(x * x for x in p)
                    if not p2:
                        continue
                    tan = math.sqrt(1 - float(cutq) ** 2) / float(cutq) * math.sqrt(sum(x * x for x in a8) / p2)
                    for nudge in ("0.98", "0.998", "1", "1.002", "1.02"):
                        t = Fraction(tan).limit_denominator(10 ** 6) * Fraction(nudge)
                        dirs.append([a8[a] + p[a] * t for a in range(3)])
            for dv in dirs:
                n2 = sum(x * x for x in dv)
                if n2 and _ge_scaled_root(sum(dv[a] * aq[a] for a in range(3)), cutq, n2):
                    assert _ge_scaled_root(sum(dv[a] * axis[a] for a in range(3)), cutoff - Fraction("1e-6"), n2), names[k]
        else:
            assert out[k]["cone_cutoff"] == 127 and not out[k]["cone_axis"].any(), names[k]
    assert checked > 1500 and cones > 300


def test_stored_halves_are_ieee_rounding_except_on_the_three_deviations(cases, run):
    """the oracle's own orc_quantize_half, through the records: centre and radius of the quantiser group (and of every other
    case) against numpy.float16 — equal, except that ties go up in magnitude, values below 2^-14 are flushed, and NaN is 0x7e00"""
    names = cases[3]
    out, f = run
    stored = np.concatenate([out["center"], out["radius"][:, None]], axis=1)
    v = f[:, :4]
    with np.errstate(all="ignore"):
        ieee = v.astype(np.float16).view(np.uint16)
    a = np.abs(v.astype(np.float64))
    nan = np.isnan(v)
    flush = (a < 2.0 ** -14) & (a > 0)
    e = np.floor(np.log2(np.where((a > 0) & np.isfinite(a), a, 1.0)))
    q = np.where(np.isfinite(a), a, 0.0) / 2.0 ** (e - 10)
    tie = np.isfinite(a) & (a >= 2.0 ** -14) & (a < 65520) & (q - np.floor(q) == 0.5)
    plain = ~(nan | flush | tie)
    assert (stored[plain] == ieee[plain]).all()                                    # includes saturation, infinities, signed zeros, 65504
    quant = np.zeros(len(out), bool)
    quant[list(C.groups()["quantiser"])] = True
    # ties: up in magnitude; this differs from round-to-even exactly when the neighbour below is even
    assert (tie & quant[:, None]).sum() >= 20
    below = (np.floor(q).astype(np.int64) - 1024) + ((e + 15).astype(np.int64) << 10)
    want = (np.signbit(v).astype(np.int64) << 15) | (below + 1)
    assert (stored[tie] == want[tie]).all()
    even = tie & (np.floor(q) % 2 == 0)
    assert (even & quant[:, None]).sum() >= 10 and (stored[even] == ieee[even] + 1).all() and (stored[tie & ~even] == ieee[tie & ~even]).all()
    # flush: a signed zero where IEEE keeps a subnormal; exactly 2^-14 stays
    assert (flush & quant[:, None]).sum() >= 20 and (stored[flush] == (np.signbit(v[flush]).astype(np.uint16) << 15)).all()
    assert (ieee[flush & (a > 2.0 ** -25)] & 0x7FFF != 0).all() and (flush & (a > 2.0 ** -25) & quant[:, None]).sum() >= 20
    assert ((a == 2.0 ** -14) & quant[:, None]).sum() >= 6 and (stored[a == 2.0 ** -14] & 0x7FFF == 0x0400).all()
    # saturation and the largest finite value
    sat = (a >= 65520) & np.isfinite(a)
    assert (sat & quant[:, None]).sum() >= 5 and (stored[sat] & 0x7FFF == 0x7C00).all()
    assert ((a == 65504) & quant[:, None]).sum() >= 7 and (stored[a == 65504] & 0x7FFF == 0x7BFF).all()
    # NaN: the results hold the canonical quiet NaN (sign clear), so the half is 0x7e00
    assert nan.sum() >= 20 and (stored[nan] == 0x7E00).all() and (v.view(np.uint32)[nan] == 0x7FC00000).all()


def _write_cases(path, meshlets, data, vertices):
    with open(path, "wb") as fh:
        fh.write(np.array([0x4342564E, len(meshlets), len(data), len(vertices)], "<u4").tobytes())
        fh.write(meshlets.tobytes() + data.tobytes() + vertices.tobytes())


def test_the_standalone_program_runs_clean_under_the_host_sanitizers(tmp_path, cases, run):
    """tools/bounds_check.c with oracle/oracle.c, its own main, no Python in the process: AddressSanitizer and UBSan (with
    float-cast-overflow: the conversions of the quantisers and of the s8 cutoff) linked statically, over all groups; what the
    sanitised build computes is what the library computed"""
    meshlets, data, vertices, _ = cases
    exe, raw, res = tmp_path / "bounds_check", tmp_path / "cases.bin", tmp_path / "results.bin"
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-g", "-ffp-contract=off", "-fopenmp", "-fsanitize=address,undefined,float-cast-overflow",
                           "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", os.path.join(ROOT, "oracle"),
                           os.path.join(ROOT, "tools", "bounds_check.c"), os.path.join(ROOT, "oracle", "oracle.c"), "-lm", "-o", str(exe)])
    _write_cases(raw, meshlets, data, vertices)
    out = subprocess.run([str(exe), str(raw), str(res)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    print(out.stdout.decode())
    assert out.returncode == 0 and b"bounds_check: ok" in out.stdout
    blob = open(res, "rb").read()
    assert blob == run[0].tobytes() + run[1].tobytes()
