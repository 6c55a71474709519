"""ctypes loader of tests/animate_ref.c, the independent CPU restatement of the keyframe animation (test infrastructure), the
fuzz inputs of tests/test_animation_cpu.py and tests/test_animation_gpu.py, and the counted bound of the trigonometric branch.

`load(directory)` compiles it there twice with raster_ref.c's flags: as fp32 (the bits nv_animate_draws_host must write) and with -DREAL=double."""
import ctypes as C
import os
import subprocess

import numpy as np

import raster_ref as RR
from niagara_amd import layouts as L

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "animate_ref.c")
TRIG, NEGATED = 1, 2  # ar_eval's flags

# per orientation component of the trigonometric branch, |fp32 - fp64| <= M (2 A + 2 S + 5/2) 2^-23 to first order, with
# A = S = 4 the ulp bounds of acos and sin that cover both libraries (OpenCL's table, which the device library is built to; glibc documents
# 1 and 1), and M = |x_k| W0 + |z_k| W1 <= sqrt(2) max|component| for the weights W of an angle <= pi / 2: 18.5 sqrt(2) = 26.2, stated as 27
# to hold the second-order terms, for quaternions whose components do not exceed 1 in magnitude
TRIG_BOUND = 27.0 * 2.0 ** -23


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class AnimRef:
    def __init__(self, so32, so64):
        self.libs = {"f32": C.CDLL(so32), "f64": C.CDLL(so64)}
        for k, size in (("f32", 4), ("f64", 8)):
            assert self.libs[k].ar_real_bytes() == size
            self.libs[k].ar_eval.restype = None
            self.libs[k].ar_apply.restype = None

    def eval(self, animations, keyframes, which, times, real="f32"):
        """one sample per (animation which[i], time times[i]): dict of skipped (bool), index0, index1, t (float32), out (n, 8) float64 =
        position xyz, scale, orientation xyzw in the build's precision, flags (TRIG, NEGATED); the entries of a skipped sample are zero"""
        a, k = np.ascontiguousarray(animations, L.ANIMATION), np.ascontiguousarray(keyframes, L.KEYFRAME)
        which, times = np.ascontiguousarray(which, np.uint32), np.ascontiguousarray(times, np.float64)
        n = len(which)
        r = dict(skipped=np.zeros(n, np.uint8), index0=np.zeros(n, np.uint32), index1=np.zeros(n, np.uint32), t=np.zeros(n, np.float32),
                 out=np.zeros((n, 8), np.float64), flags=np.zeros(n, np.uint8))
        self.libs[real].ar_eval(_p(a), _p(k), _p(which), _p(times), C.c_uint64(n), _p(r["skipped"]), _p(r["index0"]), _p(r["index1"]), _p(r["t"]),
                                _p(r["out"]), _p(r["flags"]))
        r["skipped"] = r["skipped"].astype(bool)
        return r

    def apply(self, time, animations, keyframes, draws, lights=None, real="f32"):
        """the reference's loop over the table in array order: (draws, lights) rewritten copies"""
        a, k = np.ascontiguousarray(animations, L.ANIMATION), np.ascontiguousarray(keyframes, L.KEYFRAME)
        d = None if draws is None else np.ascontiguousarray(draws, L.MESHDRAW).copy()
        li = None if lights is None else np.ascontiguousarray(lights, L.LIGHT).copy()
        self.libs[real].ar_apply(C.c_double(float(time)), _p(a), C.c_uint32(len(a)), _p(k), _p(d), _p(li))
        return d, li


def load(directory):
    sos = []
    for name, extra in (("libanimate_ref32.so", []), ("libanimate_ref64.so", ["-DREAL=double"])):
        so = os.path.join(str(directory), name)
        if not os.path.exists(so):
            subprocess.check_call(["gcc"] + RR.FLAGS + extra + ["-Wall", "-shared", "-fPIC", "-o", so, SRC, "-lm"])
        sos.append(so)
    return AnimRef(*sos)


def unit_quats(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.clip(q.astype(np.float32), -1.0, 1.0)


def fuzz_table(count, draw_count, seed, light_count=0, max_keys=9):
    """`count` animations over distinct random draws (and, for the first light_count of them, distinct lights), 1 .. max_keys keyframes each:
    start times in [-2, 2], periods in [0.05, 3] (every fourth animation on the 0.25 grid); random unit quaternions, of which a quarter
    repeat their predecessor up to a rotation of ~1e-4 .. 1e-3 rad (both sides of slerp's threshold) and about half of the rest lie in the far hemisphere of their predecessor (the negated path comes with random quaternions)"""
    rng = np.random.default_rng(seed)
    a = np.zeros(count, L.ANIMATION)
    a["drawIndex"] = rng.permutation(draw_count)[:count]
    a["lightIndex"] = -1
    a["lightIndex"][:light_count] = rng.permutation(light_count)
    a["startTime"] = rng.uniform(-2.0, 2.0, count).astype(np.float32)
    a["period"] = rng.uniform(0.05, 3.0, count).astype(np.float32)
    grid = np.arange(count) % 4 == 0  # a quarter on the 0.25 grid: multiples of 0.25 are exact keyframe instants of theirs
    a["startTime"][grid] = (rng.integers(-8, 9, count) * 0.25).astype(np.float32)[grid]
    a["period"][grid] = rng.choice(np.array([0.25, 0.5, 1.0, 2.0], np.float32), count)[grid]
    a["keyframeCount"] = rng.integers(1, max_keys + 1, count)
    a["keyframeOffset"] = np.concatenate([[0], np.cumsum(a["keyframeCount"])[:-1]]) if count else 0
    total = int(a["keyframeCount"].sum())
    k = np.zeros(total, L.KEYFRAME)
    k["translation"] = rng.uniform(-50.0, 50.0, (total, 3)).astype(np.float32)
    k["scale"] = rng.uniform(0.25, 4.0, total).astype(np.float32)
    q = unit_quats(rng, total).astype(np.float64)
    near = np.flatnonzero(rng.random(total) < 0.25)
    near = near[near > 0]
    for i in near:  # q[i] = q[i - 1] turned by a small angle about a random axis (in order: chains of near keyframes are fine)
        ang = 10.0 ** rng.uniform(-4.0, -3.0)
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        bx, by, bz = ax * np.sin(ang / 2)
        bw = np.cos(ang / 2)
        x, y, z, w = q[i - 1]
        q[i] = [w * bx + x * bw + y * bz - z * by, w * by - x * bz + y * bw + z * bx, w * bz + x * by - y * bx + z * bw, w * bw - x * bx - y * by - z * bz]
        q[i] /= np.linalg.norm(q[i])
    k["rotation"] = np.clip(q.astype(np.float32), -1.0, 1.0)
    return a, k


TIMES = (-10.0, -0.5, 0.0, 1e9, 8.0, 12.5, 100.25, 0.7, 1.3, 2.9, 3.1, 7.77, 19.4, 33.33, 47.01, 59.9)


def fuzz_times(animations, times=TIMES):
    """(which, times): every animation at every time of `times`, time-major (sample j * len(animations) + i is animation i at times[j]) — what
    one call of the evaluation over the whole table computes per time.  TIMES holds a time before every start (all skipped), one between the
    starts (some skipped), 1e9, and multiples of 0.25 that are exact keyframe instants (t == 0) of fuzz_table's grid animations; the wrap
    (index1 == 0) comes with the random ones"""
    n = len(animations)
    return np.tile(np.arange(n, dtype=np.uint32), len(times)), np.repeat(np.asarray(times, np.float64), n)
