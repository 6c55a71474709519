"""a second, independent restatement of the meshlet bounds (TEST INFRASTRUCTURE).  Plain and sequential,
pure Python over numpy.float32 scalars: one IEEE single operation per source operation, sums left to right, points in
triangle order — the published algorithm as oracle.c documents it (meshopt_computeClusterBounds with the three-axis Ritter
sphere, meshopt_quantizeSnorm(…, 8) with the error term, meshopt_quantizeHalf), sharing no code with oracle.c or bounds.hip.
The quantisers are written from their meaning (exact rationals), not from the library's bit tricks.

Defined semantics: counts clamp to 64 / 96, index bytes are masked with 63, shortRefs != 1 means 32-bit
references, comparisons are the ones written (x < NaN is false: a NaN is never an extreme unless it is point 0, and never
"outside"), the cutoff conversion is q < 127 ? (int)q : 127, and a NaN among the eight results is the canonical quiet NaN
0x7fc00000 before it is stored or quantised.

bounds(meshlet fields, data, vertices) -> dict with the eight floats ("f8", float32[8]), the twelve record bytes ("rec") and
the diagnostics the case builder asserts its conditions on."""
from fractions import Fraction

import numpy as np

F = np.float32
_ZERO, _HALF, _ONE, _TWO, _C127 = F(0), F(0.5), F(1), F(2), F(127)
_QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def half_to_float(h):
    """IEEE binary16 bits -> float32, by value (every binary16 is exact in binary32); a NaN keeps nothing but being a NaN"""
    h = int(h)
    sign, e, m = h >> 15, (h >> 10) & 31, h & 1023
    if e == 31:
        v = float("nan") if m else float("inf")
    elif e == 0:
        v = m * 2.0 ** -24
    else:
        v = (1024 + m) * 2.0 ** (e - 25)
    return F(-v if sign else v)


def quantize_half(v):
    """meshopt_quantizeHalf by its meaning: nearest binary16 with ties up in magnitude, below 2^-14 flushed to a signed
    zero, 65520 and above to infinity, NaN to 0x7e00 — the sign bit kept in every case"""
    v = F(v)
    sign = (int(np.array([v], np.float32).view(np.uint32)[0]) >> 16) & 0x8000
    if v != v:
        return sign | 0x7E00
    a = abs(float(v))
    if a == float("inf") or a >= 65536.0:
        return sign | 0x7C00
    if a < 2.0 ** -14:
        return sign
    x = Fraction(a)
    e = 0
    while x >= Fraction(2) ** (e + 1):
        e += 1
    while x < Fraction(2) ** e:
        e -= 1
    q = x / Fraction(2) ** (e - 10) + Fraction(1, 2)
    q = q.numerator // q.denominator  # floor(x / ulp + 1/2): a tie goes up
    if q == 2048:
        e, q = e + 1, 1024
    return sign | ((e + 15) << 10) + (q - 1024)  # e = 16 is 0x7c00: infinity


def quantize_snorm8(v):
    """meshopt_quantizeSnorm(v, 8): the rounding term takes the sign of v before the clamp, the clamp is written with
    comparisons (NaN -> -1), the conversion truncates"""
    v = F(v)
    r = _HALF if v >= _ZERO else -_HALF
    v = v if v >= -_ONE else -_ONE
    v = v if v <= _ONE else _ONE
    return int(v * _C127 + r)


def _sphere(points):
    """computeBoundingSphere, three-axis form, over a list of (x, y, z) float32 triples"""
    pmin, pmax = [0, 0, 0], [0, 0, 0]
    for i, p in enumerate(points):
        for a in range(3):
            if p[a] < points[pmin[a]][a]:
                pmin[a] = i
            if p[a] > points[pmax[a]][a]:
                pmax[a] = i
    paxisd2, paxis, axis_d2 = _ZERO, 0, []
    for a in range(3):
        p1, p2 = points[pmin[a]], points[pmax[a]]
        dx, dy, dz = p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]
        d2 = (dx * dx + dy * dy) + dz * dz
        axis_d2.append(d2)
        if d2 > paxisd2:
            paxisd2, paxis = d2, a
    p1, p2 = points[pmin[paxis]], points[pmax[paxis]]
    c = [(p1[0] + p2[0]) / _TWO, (p1[1] + p2[1]) / _TWO, (p1[2] + p2[2]) / _TWO]
    r = np.sqrt(paxisd2) / _TWO
    grown_at = []
    for i, p in enumerate(points):
        dx, dy, dz = p[0] - c[0], p[1] - c[1], p[2] - c[2]
        d2 = (dx * dx + dy * dy) + dz * dz
        if d2 > r * r:
            d = np.sqrt(d2)
            k = _HALF + (r / d) / _TWO
            c[0] = c[0] * k + p[0] * (_ONE - k)
            c[1] = c[1] * k + p[1] * (_ONE - k)
            c[2] = c[2] * k + p[2] * (_ONE - k)
            r = (r + d) / _TWO
            grown_at.append(i)
    return c, r, dict(pmin=pmin, pmax=pmax, paxis=paxis, axis_d2=axis_d2, grown_at=grown_at, rounds=len(grown_at))


def _canon(v):
    return _QNAN if v != v else v


def bounds(m, data, vertices):
    """m: one L.MESHLET record (only dataOffset, baseVertex, vertexCount, triangleCount, shortRefs are read); data: uint32[];
    vertices: L.VERTEX[]"""
    with np.errstate(all="ignore"):
        return _bounds(m, data, vertices)


def _bounds(m, data, vertices):
    vc, tc = min(int(m["vertexCount"]), 64), min(int(m["triangleCount"]), 96)
    short = int(m["shortRefs"]) == 1
    off, base = int(m["dataOffset"]), int(m["baseVertex"])
    d16, d8 = data.view(np.uint16), data.view(np.uint8)
    pos = [(_ZERO, _ZERO, _ZERO)] * 64
    for i in range(vc):
        vi = (int(d16[off * 2 + i]) if short else int(data[off + i])) + base
        v = vertices[vi]
        pos[i] = (half_to_float(v["vx"]), half_to_float(v["vy"]), half_to_float(v["vz"]))
    ioff = (off + ((vc + 1) // 2 if short else vc)) * 4
    corners, normals, kept_index = [], [], []
    for t in range(tc):
        a, b, c = (int(d8[ioff + t * 3 + k]) & 63 for k in range(3))
        p0, p1, p2 = pos[a], pos[b], pos[c]
        ux, uy, uz = p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]
        vx, vy, vz = p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]
        nx = uy * vz - uz * vy
        ny = uz * vx - ux * vz
        nz = ux * vy - uy * vx
        area = np.sqrt((nx * nx + ny * ny) + nz * nz)
        if area == _ZERO:
            continue
        normals.append((nx / area, ny / area, nz / area))
        corners += [p0, p1, p2]
        kept_index.append(t)
    center, radius, axis, cutoff = [_ZERO] * 3, _ZERO, [_ZERO] * 3, _ZERO
    a8, c8 = [0, 0, 0], 0
    diag = dict(kept=len(normals), kept_index=kept_index, pos=None, nrm=None, mindp=None, axislength=None, q=None)
    if normals:
        center, radius, diag["pos"] = _sphere(corners)
        axis, _, diag["nrm"] = _sphere(normals)
        length = np.sqrt((axis[0] * axis[0] + axis[1] * axis[1]) + axis[2] * axis[2])
        inv = _ZERO if length == _ZERO else _ONE / length
        axis = [axis[0] * inv, axis[1] * inv, axis[2] * inv]
        mindp = _ONE
        for n in normals:
            dp = (n[0] * axis[0] + n[1] * axis[1]) + n[2] * axis[2]
            if dp < mindp:
                mindp = dp
        diag["mindp"], diag["axislength"] = mindp, length
        if mindp <= F(0.1):
            axis, cutoff, c8 = [_ZERO] * 3, _ONE, 127
        else:
            cutoff = np.sqrt(_ONE - mindp * mindp)
            e = _ZERO
            for k in range(3):
                a8[k] = quantize_snorm8(axis[k])
                e = e + abs(F(a8[k]) / _C127 - axis[k])
            q = _C127 * (cutoff + e) + _ONE
            diag["q"] = q
            c8 = int(q) if q < _C127 else 127
    f8 = np.array([_canon(x) for x in (center[0], center[1], center[2], radius, axis[0], axis[1], axis[2], cutoff)], np.float32)
    rec = np.zeros(12, np.uint8)
    rec[:8] = np.array([quantize_half(x) for x in f8[:4]], "<u2").view(np.uint8)
    rec[8:] = np.array(a8 + [c8], np.int8).view(np.uint8)
    diag.update(f8=f8, rec=rec, corners=corners, normals=normals)
    return diag


def all_bounds(meshlets, data, vertices):
    return [bounds(m, data, vertices) for m in meshlets]
