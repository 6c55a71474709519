"""Named edge cases for the meshlet bounds (TEST INFRASTRUCTURE, CPU only).  build() returns
(meshlets, data, vertices, names): a few thousand meshlets, each with a vertex window of its own, the output fields of every
record pre-filled with 0xFF.  Every group asserts, on the diagnostics of tests/bounds_ref.py, that it reached the branch
it was built for — a green comparison over these cases is never vacuous.  conditions() returns what was reached."""
import functools

import numpy as np

import bounds_ref as R
from niagara_amd import layouts as L

QNAN, SNAN, NQNAN, PINF, NINF = 0x7E00, 0x7D01, 0xFE00, 0x7C00, 0xFC00
LEAD = 16  # vertices in front of the first window, so that a reference may be baseVertex + a positive number


def h16(x):
    """float(s) -> binary16 bits"""
    return np.asarray(x, np.float64).astype(np.float16).view(np.uint16)


def exact16(x):
    """like h16, for values the case needs exactly"""
    b = h16(x)
    assert (b.view(np.float16).astype(np.float64) == np.asarray(x, np.float64)).all(), x
    return b


class Builder:
    def __init__(self):
        self.verts = [np.full((LEAD, 3), 0x4900, np.uint16)]  # 10.0: a wrong reference is seen
        self.nverts = LEAD
        self.bytes = bytearray()
        self.recs, self.names, self.groups, self.meta = [], [], {}, []

    def add(self, group, name, hpos, tris, vc=None, tc=None, short=1, delta=0, pad=0, **meta):
        """hpos: uint16 [n, 3] binary16 position bits of this meshlet's own vertices; tris: raw index bytes [t, 3];
        vc / tc: the raw counts written into the record (default n, t); delta: baseVertex sits delta below the window and the
        references are delta higher; pad: zero words in front of the payload (alignment)"""
        hpos, tris = np.asarray(hpos, np.uint16).reshape(-1, 3), np.asarray(tris, np.int64).reshape(-1, 3)
        vc = len(hpos) if vc is None else vc
        tc = len(tris) if tc is None else tc
        vcc, tcc = min(vc, 64), min(tc, 96)
        assert len(hpos) >= vcc and len(tris) >= tcc and 0 <= delta <= LEAD and tris.min(initial=0) >= 0 and tris.max(initial=0) <= 255
        self.bytes += bytes(4 * pad)
        off = len(self.bytes) // 4
        refs = np.arange(vcc) + delta
        if short == 1:
            self.bytes += refs.astype("<u2").tobytes() + bytes(2 * (vcc % 2))
        else:
            self.bytes += refs.astype("<u4").tobytes()
        idx = tris[:tcc].astype(np.uint8).tobytes()
        self.bytes += idx + bytes(-len(idx) % 4)
        self.recs.append((off, self.nverts - delta, vc, tc, short))
        self.verts.append(hpos)
        self.nverts += len(hpos)
        self.names.append("%s/%s" % (group, name))
        self.groups.setdefault(group, []).append(len(self.recs) - 1)
        self.meta.append(meta)
        return len(self.recs) - 1

    def finish(self):
        meshlets = np.zeros(len(self.recs), L.MESHLET)
        meshlets.view(np.uint8).reshape(-1, 24)[:, :12] = 0xFF
        for k, (off, base, vc, tc, short) in enumerate(self.recs):
            m = meshlets[k]
            m["dataOffset"], m["baseVertex"], m["vertexCount"], m["triangleCount"], m["shortRefs"], m["padding"] = off, base, vc, tc, short, 0xA5
        data = np.frombuffer(bytes(self.bytes) + bytes(16), np.uint32).copy()
        hp = np.concatenate(self.verts)
        vertices = np.zeros(len(hp), L.VERTEX)
        vertices["vx"], vertices["vy"], vertices["vz"] = hp[:, 0], hp[:, 1], hp[:, 2]
        vertices["tp"], vertices["np"], vertices["tu"], vertices["tv"] = 0x7E00, 0xFFFFFFFF, 0x7C00, 0xFC00  # never positions
        return meshlets, data, vertices


def audit(meshlets, data, vertices):
    """every read the defined semantics make stays inside the arrays (checked before anything runs on a device)"""
    d16 = data.view(np.uint16)
    for m in meshlets:
        vc, tc, off, short = min(int(m["vertexCount"]), 64), min(int(m["triangleCount"]), 96), int(m["dataOffset"]), int(m["shortRefs"]) == 1
        refs = d16[off * 2:off * 2 + vc].astype(np.int64) if short else data[off:off + vc].astype(np.int64)
        assert len(refs) == vc
        if vc:
            assert 0 <= int(m["baseVertex"]) + refs.min() and int(m["baseVertex"]) + refs.max() < len(vertices)
        ioff = off + ((vc + 1) // 2 if short else vc)
        assert ioff * 4 + tc * 3 <= data.nbytes


# ---------------------------------------------------------------------------------------------------------------- geometry
def cloud(rng, n, scale=2.0):
    return h16(rng.uniform(-scale, scale, (n, 3)))


def random_tris(rng, t, n):
    """t triangles with three distinct corners below n"""
    return np.array([rng.choice(n, 3, replace=False) for _ in range(t)], np.int64)


VC_RAW = (0, 1, 2, 3, 63, 64, 65, 200, 255)
TC_RAW = (0, 1, 63, 64, 65, 95, 96, 97, 255)


def _counts(b, seen):
    rng = np.random.default_rng(11)
    for vc in VC_RAW:
        for tc in TC_RAW:
            vcc = min(vc, 64)
            hpos = cloud(rng, 64)
            tris = rng.integers(0, max(vcc, 1), (96, 3))
            kind = rng.random((96, 3))
            if vcc < 64:
                zero = kind < 0.08
                tris[zero] = rng.integers(vcc, 64, int(zero.sum()))  # zero slots: at or above the vertex count
            masked = kind > 0.85
            tris[masked] += 64 * rng.integers(1, 4, int(masked.sum()))  # 64..255: masked with 63
            used = tris[:min(tc, 96)]
            seen["counts: index bytes at or above the vertex count"] += int((((used & 63) >= vcc) & (used < 64)).sum())
            seen["counts: index bytes in 64..255"] += int((used >= 64).sum())
            b.add("counts", "vc%d tc%d" % (vc, tc), hpos, tris, vc=vc, tc=tc, short=(vc + tc) % 2, vc_raw=vc, tc_raw=tc)


def _references(b):
    rng = np.random.default_rng(12)
    for vc in range(3, 11):
        hpos, tris = cloud(rng, vc), random_tris(rng, 2 * vc, vc)
        for pad in range(4):
            for short in (0, 1, 2, 255):
                b.add("references", "vc%d pad%d shortRefs%d" % (vc, pad, short), hpos, tris, short=short, delta=(vc * 7 + pad) % (LEAD + 1), pad=pad,
                      same_as=(vc,))


def _compaction(b):
    rng = np.random.default_rng(13)
    hpos, tris = cloud(rng, 64), random_tris(rng, 96, 64)

    def case(name, keep, tc=96):
        keep = np.asarray(keep, bool)
        t = tris.copy()
        t[~keep, 1] = t[~keep, 0]  # (a, a, c): zero area
        b.add("compaction", name, hpos, t, tc=tc, keep=np.flatnonzero(keep[:tc]).tolist())

    every = np.ones(96, bool)
    case("all kept", every)
    case("none kept", ~every)
    for k in (0, 63, 64, 95):
        case("only %d kept" % k, np.arange(96) == k)
    case("even kept", np.arange(96) % 2 == 0)
    case("odd kept", np.arange(96) % 2 == 1)
    straddle = np.zeros(96, bool)
    straddle[rng.choice(64, 40, replace=False)] = True
    straddle[64 + rng.choice(32, 30, replace=False)] = True
    case("40 of the first 64 and 30 of the rest", straddle)
    case("first half dropped", np.arange(96) >= 64)
    case("second half dropped", np.arange(96) < 64)
    case("70 triangles, every third dropped", np.arange(96) % 3 != 1, tc=70)


# fillers of the hand-made orders: strictly inside (-1, 1) on every axis, no two equal on any axis
_FILL = np.array([[-0.5, -0.25, 0.125], [0.25, 0.5, -0.375], [-0.125, 0.75, 0.625], [0.625, -0.625, -0.75]])
_SPECIAL_YZ = np.array([[0.9375, 0.5625], [-0.9375, 0.3125], [0.5625, -0.9375]])


def _point_order(b, name, first, others, sign, value=4.0, later_value=None, shift=0.0):
    """corners in triangle order; the extreme of x (max for sign +1, min for -1) occurs first at corner `first` and again,
    with an equal x and another y / z, at the corners `others`"""
    where = [first] + list(others)
    ntri = max(44, max(where) // 3 + 1)
    verts = [[f[0] + shift, f[1], f[2]] for f in _FILL] + [[-sign * 4.0, 0.0625, -0.0625]]  # 4: the lone opposite extreme
    for k in range(len(where)):
        x = value if k == 0 or later_value is None else later_value
        verts.append([sign * x if x != 0 else x, _SPECIAL_YZ[k][0], _SPECIAL_YZ[k][1]])
    tris = np.array([[0, 1, 2], [1, 2, 3], [2, 3, 0]] * ntri)[:ntri]
    tris[ntri - 1, 0] = 4
    for k, p in enumerate(where):
        tris[p // 3, p % 3] = 5 + k
    expect = dict(pmax=first) if sign > 0 else dict(pmin=first)
    b.add("ties", name, exact16(verts), tris, expect_pos=expect, full=ntri)


def _normal_order(b, name, where, sign):
    """normals in triangle order: the triangles at `where` have bitwise equal normal x (the extreme) and different y / z"""
    P, Q, Rr = np.array([0.0, 0.0, 0.0]), np.array([0.25, 1.0, 0.5]), np.array([-0.5, 0.25, 1.0])
    if sign < 0:
        Q, Rr = Q * [-1, 1, 1], Rr * [-1, 1, 1]
        Q, Rr = Rr, Q
    my, mz = np.array([1, -1, 1]), np.array([1, 1, -1])
    verts = [[0, 0, 0], [1, 0, 0], [0, 1, 0], P, Q, Rr, Rr * my, Q * my, Rr * mz, Q * mz]
    special = [[3, 4, 5], [3, 6, 7], [3, 8, 9]]  # A, its mirror in y and in z with the winding turned back
    tris = np.array([[0, 1, 2]] * 96)
    for k, t in enumerate(where):
        tris[t] = special[k]
    b.add("ties", name, exact16(verts), tris, expect_nrm=(dict(pmax=where[0]) if sign > 0 else dict(pmin=where[0])), equal_normal_x=list(where), full=96)


def _ties(b):
    # axis-aligned planar grids: one coordinate equal everywhere (+0 / -0 mixed in the second), the others tie in rows
    ii, jj = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    quads = [(i * 8 + j, (i + 1) * 8 + j, (i + 1) * 8 + j + 1, i * 8 + j + 1) for i in range(7) for j in range(7)]
    tris = np.array([t for a, bb, c, d in quads for t in ((a, bb, c), (a, c, d))])[:96]
    for axis in range(3):
        for plane, label in ((0.5, "0.5"), (None, "signed zeros")):
            pos = np.zeros((64, 3))
            pos[:, (axis + 1) % 3], pos[:, (axis + 2) % 3] = ii.ravel() * 0.25 - 1, jj.ravel() * 0.5 - 2
            pos[:, axis] = plane if plane is not None else np.where((ii + jj).ravel() % 2 == 0, -0.0, 0.0)
            b.add("ties", "planar grid axis %d at %s" % (axis, label), exact16(pos), tris, planar=axis, full=96)
    for sign, word in ((1, "max"), (-1, "min")):
        _point_order(b, "%s first at corner 65, again at 130 and 66" % word, 65, (130, 66), sign)
        _point_order(b, "%s first at corner 2, again at 65" % word, 2, (65,), sign)
        _point_order(b, "%s first at corner 127, again at 128 and 191" % word, 127, (128, 191), sign)
        _normal_order(b, "normal %s first at 1, again at 65 and 66" % word, (1, 65, 66), sign)
        _normal_order(b, "normal %s first at 65, again at 66 and 70" % word, (65, 66, 70), sign)
    _point_order(b, "max -0 first at corner 2, +0 at 65", 2, (65,), 1, value=-0.0, later_value=0.0, shift=-1.0)
    _point_order(b, "max +0 first at corner 65, -0 at 130 and 66", 65, (130, 66), 1, value=0.0, later_value=-0.0, shift=-1.0)
    # two axes with exactly equal extent: d2 > paxisd2 keeps the first
    b.add("ties", "x and y extents equal", exact16([[-2, 1, 0], [2, 1, 0], [0.5, -1, 0], [0.5, 3, 0]]), [[0, 1, 2], [0, 1, 3]], equal_extent=(0, 1), full=2)
    b.add("ties", "y and z extents equal", exact16([[0, -2, 1], [0, 2, 1], [0, 0.5, -1], [0, 0.5, 3]]), [[0, 1, 2], [0, 1, 3]], equal_extent=(1, 2), full=2)


def _strip(n):
    return np.array([[i, i + 1, i + 2] for i in range(n - 2)])


def _shell(seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(64, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d[np.argsort(np.arctan2(d[:, 1], d[:, 0]), kind="stable")]  # once around the z axis
    return h16(d * np.linspace(1.0, 1.5, 64)[:, None]), _strip(64)


def _fan(seed):
    """31 triangles around an apex whose normals are random directions of the upper hemisphere, widest last"""
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(31, 3))
    n[:, 2] = np.abs(n[:, 2]) + 0.35
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n = n[np.argsort(-n[:, 2], kind="stable")]
    verts, tris = [[0.0, 0.0, 0.0]], []
    for k, d in enumerate(n):
        a = np.cross(d, [1.0, 0.0, 0.0] if abs(d[0]) < 0.9 else [0.0, 1.0, 0.0])
        a /= np.linalg.norm(a)
        verts += [a, np.cross(d, a)]
        tris.append([0, 1 + 2 * k, 2 + 2 * k])
    return h16(verts), np.array(tris)


def _search(make, rounds_of, want, seeds):
    best = (-1, None)
    for seed in seeds:
        hpos, tris = make(seed)
        b = Builder()
        b.add("x", "x", hpos, tris)
        meshlets, data, vertices = b.finish()
        r = rounds_of(R.bounds(meshlets[0], data, vertices))
        if r > best[0]:
            best = (r, seed)
        if r >= want:
            break
    return best


def _growth(b):
    r, seed = _search(_shell, lambda d: d["pos"]["rounds"], 24, range(300))
    assert r >= 24, r
    b.add("growth", "shell of rising radius, seed %d" % seed, *_shell(seed), min_pos_rounds=24)
    r, seed = _search(_fan, lambda d: d["nrm"]["rounds"], 8, range(300))
    assert r >= 8, r
    b.add("growth", "fan of hemisphere normals, seed %d" % seed, *_fan(seed), min_nrm_rounds=8)
    b.add("growth", "no growth", exact16([[-1, 0, 0], [1, 0, 0], [0, 0.5, 0]]), [[0, 1, 2]], grown_at=[])
    b.add("growth", "only the last point outside", exact16([[-1, 0, 0], [1, 0, 0], [0, 0.5, 0], [0, -0.5, 0], [0, 0, 1.5]]), [[0, 1, 2], [2, 3, 4]], grown_at=[5])
    for seed in range(1000, 1004):
        b.add("growth", "shell, seed %d" % seed, *_shell(seed))
        b.add("growth", "fan, seed %d" % seed, *_fan(seed))


_ROTATIONS = [((0, 1, 2), (1, 1, 1)), ((1, 2, 0), (1, -1, 1)), ((2, 0, 1), (-1, 1, 1)), ((0, 2, 1), (1, 1, -1)), ((1, 0, 2), (-1, -1, 1)), ((2, 1, 0), (1, -1, -1))]


def _cone(b):
    for k, tri in enumerate(([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0.5, -1, 2], [1.5, 0.25, -1], [-2, 1, 0.75]], [[0, 0, 0], [0, 0, 1], [0, 1, 0]])):
        b.add("cone", "single triangle %d" % k, exact16(tri), [[0, 1, 2]], single=True)
    b.add("cone", "two opposite normals", exact16([[0.5, -1, 2], [1.5, 0.25, -1], [-2, 1, 0.75]]), [[0, 1, 2], [0, 2, 1]], zero_axis=True)
    # the fold: triangles (A, B, C) and (B, A, D) over the edge AB, D = (x, 0, h) folded back over C; mindp = 0.1 at h / x = 0.2031
    heights = np.arange(h16(0.19), h16(0.22)).astype(np.uint16).view(np.float16).astype(np.float64)
    for xk in range(8):
        x = 1.0 + xk * 2.0 ** -10
        cos_t = -x / np.sqrt(heights ** 2 + x * x)
        near = heights[np.abs(np.sqrt((1 + cos_t) / 2) - 0.1) < 2.5e-4]
        for h in near:
            for perm, sg in _ROTATIONS[:1 + (xk % 2) * 5]:
                pos = (np.array([[0, -1, 0], [0, 1, 0], [1, 0, 0], [x, 0, h]])[:, perm]) * sg
                b.add("cone", "fold x %.6f h %.6f %s%s" % (x, h, perm, sg), exact16(pos), [[0, 1, 2], [1, 0, 3]], fold=True)


    # mindp == 0.1f exactly (found by a search over the fp16 grid): "<=" takes the no-cone branch
    for x, h in ((0.57861328125, 0.11749267578125), (1.1572265625, 0.2349853515625), (2.314453125, 0.469970703125)):
        b.add("cone", "fold at exactly 0.1f, x %r h %r" % (x, h), exact16([[0, -1, 0], [0, 1, 0], [1, 0, 0], [x, 0, h]]), [[0, 1, 2], [1, 0, 3]], fold=True, tenth=True)


def _quantiser(b):
    u = 2.0 ** -10
    def tri_on(t, ta, tb, name, long=2.0):
        """one triangle: the longest extent (long) on axis l = t + 1, the values ta / tb of axis t at its two ends"""
        l, o = (t + 1) % 3, (t + 2) % 3
        p = np.zeros((3, 3))
        p[0, l], p[1, l] = -long / 2, long / 2
        p[:, t] = ta, tb, ta
        p[2, o] = long / 8
        b.add("quantiser", "centre axis %d %s" % (t, name), exact16(p), [[0, 1, 2]], quant=True)
    for t in range(3):
        for s in (1.0, -1.0):
            tri_on(t, s * 1.0, s * (1 + u), "tie, even below, sign %+d" % s)
            tri_on(t, s * (1 + u), s * (1 + 2 * u), "tie, odd below, sign %+d" % s)
            tri_on(t, 0.0, s * 2.0 ** -13, "exactly 2^-14, sign %+d" % s)
            tri_on(t, 0.0, s * (2.0 ** -13 - 2.0 ** -24), "just below 2^-14, sign %+d" % s)
            tri_on(t, s * 3 * 2.0 ** -24, s * 5 * 2.0 ** -24, "subnormal vertices, sign %+d" % s)
            tri_on(t, s * 65504.0, s * 65504.0, "largest finite, sign %+d" % s)
            tri_on(t, s * 65472.0, s * 65504.0, "tie below the largest finite, sign %+d" % s)
    def radius_case(name, p):
        b.add("quantiser", "radius %s" % name, exact16(p), [[0, 1, 2]], quant=True)
    radius_case("tie, even below", [[-1, 0, 0], [1 + u, 0, 0], [0, 0.25, 0]])
    radius_case("tie, odd below", [[-1, 0, 0], [1 + 3 * u, 0, 0], [0, 0.25, 0]])
    radius_case("exactly 2^-14", [[0, 0, 0], [2.0 ** -13, 0, 0], [2.0 ** -14, 2.0 ** -20, 0]])
    radius_case("just below 2^-14", [[0, 0, 0], [2.0 ** -13 - 2.0 ** -24, 0, 0], [2.0 ** -14, 2.0 ** -20, 0]])
    radius_case("subnormal vertices", [[0, 0, 0], [9 * 2.0 ** -24, 0, 0], [4 * 2.0 ** -24, 2.0 ** -24, 0]])
    radius_case("largest finite", [[-65504, 0, 0], [65504, 0, 0], [0, 1, 0]])
    radius_case("far above the range", [[-65504, -65504, -65504], [65504, 65504, 65504], [0, 1, 0]])
    for dy in range(2880, 2914, 2):  # radius crosses 65520 at dy = 2895.8
        radius_case("near 65520, dy %d" % dy, [[-65504, 0, 0], [65504, dy, 0], [0, 1, 16]])
    # a second triangle that grows the sphere, so that centre and radius are no midpoints of inputs
    for k in range(24):
        rng = np.random.default_rng(500 + k)
        scale = (2.0 ** -12, 1.0, 30000.0)[k % 3]
        b.add("quantiser", "two triangles, scale %g, seed %d" % (scale, k), h16(rng.uniform(-1, 1, (4, 3)) * scale), [[0, 1, 2], [1, 2, 3]], quant=True)


_BASE = np.array([[-1, -0.5, 0.25], [1, 0.5, -0.25], [0.25, 1, 0.5], [-0.5, 0.75, -1], [0.5, -1, 0.75], [0.75, 0.25, 1], [0.125, -0.125, 0.375]])
_BASE_TRIS = [[0, 1, 2], [2, 3, 0], [3, 4, 5]]  # vertex 0 is point 0, vertex 5 only in the last triangle, vertex 6 in none


def _non_finite(b):
    base = exact16(_BASE)
    b.add("non-finite", "finite base", base, _BASE_TRIS, nf=("base",))
    for vname, bits in (("+inf", PINF), ("-inf", NINF), ("quiet NaN", QNAN), ("signalling NaN", SNAN), ("negative NaN", NQNAN)):
        for where, v in (("first", 0), ("later", 5), ("unused", 6)):
            for coords in ((0,), (1, 2), (0, 1, 2)):
                hp = base.copy()
                hp[v, list(coords)] = bits
                b.add("non-finite", "%s in the %s vertex, coordinates %s" % (vname, where, coords), hp, _BASE_TRIS, nf=(where, vname, coords))
    b.add("non-finite", "all vertices NaN", np.full((7, 3), QNAN, np.uint16), _BASE_TRIS, nf=("all",))
    hp = base.copy()
    hp[0, 0], hp[5, 0] = PINF, NINF
    b.add("non-finite", "+inf first and -inf later on one axis", hp, _BASE_TRIS, nf=("mixed",))
    hp = base.copy()
    hp[1, 0], hp[5, 0] = PINF, PINF
    b.add("non-finite", "+inf twice on one axis", hp, _BASE_TRIS, nf=("mixed",))
    hp = base.copy()
    hp[0, 0], hp[5, 1] = QNAN, PINF
    b.add("non-finite", "NaN first, +inf later", hp, _BASE_TRIS, nf=("mixed",))
    # inf / inf.  The growth step's radius / d cannot be one: a point grows the sphere only if d2 > radius * radius, which nothing
    # satisfies once the radius is infinite, and a finite radius over d = inf is 0 (k = 0.5, centre and radius become infinite: the
    # "+inf ... later" cases above).  Where inf / inf does occur is n / area: one infinite coordinate makes a normal component and
    # the area infinite
    hp = base.copy()
    hp[1, 0] = PINF
    b.add("non-finite", "inf / inf in the normal", hp, _BASE_TRIS, nf=("infinf",))


def _random(b):
    """everything at once: raw counts on both sides of the limits, every reference width, masked and zero-slot index bytes,
    degenerate triangles, scales from fp16 subnormals to the top of the range, and in one meshlet of eight a non-finite vertex"""
    rng = np.random.default_rng(19)
    specials = (PINF, NINF, QNAN, SNAN, NQNAN)
    for k in range(1400):
        vc = int(rng.choice([rng.integers(0, 66), rng.integers(0, 256), 64]))
        tc = int(rng.choice([rng.integers(0, 98), rng.integers(0, 256), 96, rng.integers(1, 6)]))
        scale = float(rng.choice([2.0 ** -18, 2.0 ** -12, 0.01, 1.0, 1.0, 50.0, 3000.0, 60000.0]))
        hpos = cloud(rng, 64, scale)
        if k % 3 == 0:
            hpos = h16(np.round(rng.uniform(-3, 3, (64, 3))) * scale * 0.25)  # a coarse lattice: ties and zero areas
        if k % 8 == 0:
            for _ in range(int(rng.integers(1, 4))):
                hpos[rng.integers(0, 64), rng.integers(0, 3)] = specials[rng.integers(0, 5)]
        tris = rng.integers(0, max(min(vc, 64), 1), (96, 3))
        odd = rng.random((96, 3))
        tris[odd > 0.9] = rng.integers(0, 256, int((odd > 0.9).sum()))
        dup = rng.random(96) < 0.15
        tris[dup, 2] = tris[dup, 0]
        b.add("random", "%d" % k, hpos, tris, vc=vc, tc=tc, short=int(rng.choice([0, 1, 1, 2, 255])), delta=int(rng.integers(0, LEAD + 1)), pad=int(rng.integers(0, 4)))


def _classify(v):
    """class of a float32 against meshopt_quantizeHalf's deviations from IEEE rounding"""
    a = abs(float(v))
    if v != v:
        return "nan"
    if a == 0 or a == float("inf"):
        return None
    if a < 2.0 ** -14:
        return "below 2^-14"
    if a == 2.0 ** -14:
        return "exactly 2^-14"
    if a >= 65520:
        return "saturates"
    if a == 65504:
        return "largest finite"
    e = int(np.floor(np.log2(a)))
    q = a / 2.0 ** (e - 10)
    if q - np.floor(q) == 0.5:
        return "tie, %s below" % ("even" if int(np.floor(q)) % 2 == 0 else "odd")
    return None


@functools.lru_cache(maxsize=None)
def _built():
    b = Builder()
    seen = {"counts: index bytes at or above the vertex count": 0, "counts: index bytes in 64..255": 0}
    _counts(b, seen)
    _references(b)
    _compaction(b)
    _ties(b)
    _growth(b)
    _cone(b)
    _quantiser(b)
    _non_finite(b)
    _random(b)
    meshlets, data, vertices = b.finish()
    audit(meshlets, data, vertices)
    ref = R.all_bounds(meshlets, data, vertices)
    reached = _conditions(b, meshlets, ref, seen)
    for a in (meshlets, data, vertices):
        a.setflags(write=False)
    return meshlets, data, vertices, tuple(b.names), {g: tuple(v) for g, v in b.groups.items()}, ref, reached, tuple(b.meta)


def _conditions(b, meshlets, ref, seen):
    g, meta, reached = b.groups, b.meta, dict(seen)
    # counts
    assert seen["counts: index bytes at or above the vertex count"] > 100 and seen["counts: index bytes in 64..255"] > 100
    assert {(meta[k]["vc_raw"], meta[k]["tc_raw"]) for k in g["counts"]} == {(v, t) for v in VC_RAW for t in TC_RAW}
    for k in g["counts"]:
        if meta[k]["vc_raw"] == 0 or meta[k]["tc_raw"] == 0:
            assert not ref[k]["f8"].view(np.uint32).any() and not ref[k]["rec"].any(), b.names[k]
    reached["counts: meshlets with a real sphere"] = sum(1 for k in g["counts"] if ref[k]["kept"])
    assert reached["counts: meshlets with a real sphere"] >= 40
    # references
    offs = {(int(meshlets[k]["dataOffset"]) % 4, int(meshlets[k]["shortRefs"])) for k in g["references"]}
    assert offs == {(a, s) for a in range(4) for s in (0, 1, 2, 255)}
    ioffs = set()
    for k in g["references"]:
        vc, short = int(meshlets[k]["vertexCount"]), meshlets[k]["shortRefs"] == 1
        ioffs.add((int(meshlets[k]["dataOffset"]) + ((vc + 1) // 2 if short else vc)) % 4)
    assert ioffs == {0, 1, 2, 3}
    assert {int(meshlets[k]["vertexCount"]) % 2 for k in g["references"] if meshlets[k]["shortRefs"] == 1} == {0, 1}
    by_geometry = {}
    for k in g["references"]:
        by_geometry.setdefault(meta[k]["same_as"], set()).add(ref[k]["f8"].tobytes() + ref[k]["rec"].tobytes())
        assert meshlets[k]["baseVertex"] != 0 and ref[k]["kept"]
    assert all(len(v) == 1 for v in by_geometry.values())  # the width of the references does not change the result
    # compaction
    for k in g["compaction"]:
        assert ref[k]["kept_index"] == meta[k]["keep"], b.names[k]
    reached["compaction: kept counts"] = [ref[k]["kept"] for k in g["compaction"]]
    assert reached["compaction: kept counts"][:9] == [96, 0, 1, 1, 1, 1, 48, 48, 70]
    # ties
    for k in g["ties"]:
        m, d = meta[k], ref[k]
        assert d["kept"] == m["full"], b.names[k]
        for which in ("pos", "nrm"):
            for key, idx in m.get("expect_" + which, {}).items():
                assert d[which][key][0] == idx, (b.names[k], d[which])
        if "equal_normal_x" in m:
            n = [d["normals"][t] for t in m["equal_normal_x"]]
            assert len({x[0].tobytes() for x in n}) == 1 and len({(x[1].tobytes(), x[2].tobytes()) for x in n}) == len(n)
        if "planar" in m:
            a = m["planar"]
            assert d["pos"]["pmin"][a] == 0 and d["pos"]["pmax"][a] == 0 and d["pos"]["axis_d2"][a] == 0
        if "equal_extent" in m:
            a0, a1 = m["equal_extent"]
            assert d["pos"]["axis_d2"][a0] == d["pos"]["axis_d2"][a1] > 0 and d["pos"]["paxis"] == a0
    # growth
    rounds = {b.names[k]: (ref[k]["pos"]["rounds"], ref[k]["nrm"]["rounds"]) for k in g["growth"]}
    for k in g["growth"]:
        m, d = meta[k], ref[k]
        assert d["pos"]["rounds"] >= m.get("min_pos_rounds", 0) and d["nrm"]["rounds"] >= m.get("min_nrm_rounds", 0)
        if "grown_at" in m:
            assert d["pos"]["grown_at"] == m["grown_at"], b.names[k]
    reached["growth: (position, normal) rounds"] = rounds
    assert max(r[0] for r in rounds.values()) >= 24 and max(r[1] for r in rounds.values()) >= 8
    # cone
    assert all(ref[k]["kept"] == 1 and ref[k]["q"] is not None for k in g["cone"] if meta[k].get("single"))
    assert all(ref[k]["axislength"] == 0 and ref[k]["rec"][11] == 127 for k in g["cone"] if meta[k].get("zero_axis"))
    fold = [k for k in g["cone"] if meta[k].get("fold")]
    tenth = float(np.float32(0.1))
    above = [float(ref[k]["mindp"]) - tenth for k in fold if ref[k]["q"] is not None]
    below = [tenth - float(ref[k]["mindp"]) for k in fold if ref[k]["q"] is None and not meta[k].get("tenth")]  # the scanned ones only
    assert above and below and 0 < min(above) < 1e-4 and 0 < min(below) < 1e-4
    exact = [k for k in fold if meta[k].get("tenth")]
    assert len(exact) == 3 and all(ref[k]["mindp"] == R.F(0.1) and ref[k]["q"] is None and ref[k]["rec"][11] == 127 for k in exact)
    reached["cone: no-cone cases with mindp == 0.1f exactly"] = len(exact)
    qs = [float(ref[k]["q"]) for k in g["cone"] if ref[k]["q"] is not None]
    reached["cone: real cones closest above 0.1f (mindp - 0.1f)"] = min(above)
    reached["cone: no-cone cases closest below 0.1f (0.1f - mindp)"] = min(below)
    reached["cone: real cones with 127 (cutoff + e) + 1 >= 128 (clamped)"] = sum(1 for q in qs if q >= 128)
    reached["cone: real cones with the value in [127, 128) (truncated to 127)"] = sum(1 for q in qs if 127 <= q < 128)
    reached["cone: fold cases (real, none)"] = (len(above), len(below))
    assert reached["cone: real cones with 127 (cutoff + e) + 1 >= 128 (clamped)"] >= 1
    assert reached["cone: real cones with the value in [127, 128) (truncated to 127)"] >= 1
    # quantiser
    classes = {f: {} for f in range(4)}
    for k in g["quantiser"]:
        assert ref[k]["kept"] >= 1
        for f in range(4):
            c = _classify(ref[k]["f8"][f])
            if c:
                c += ", negative" if ref[k]["f8"][f] < 0 and c.startswith("tie") else ""
                classes[f][c] = classes[f].get(c, 0) + 1
    for f in range(3):
        assert {"tie, even below", "tie, odd below", "tie, even below, negative", "tie, odd below, negative", "below 2^-14", "exactly 2^-14",
                "largest finite"} <= set(classes[f]), (f, classes[f])
    assert {"tie, even below", "tie, odd below", "below 2^-14", "exactly 2^-14", "largest finite", "saturates"} <= set(classes[3]), classes[3]
    reached["quantiser: classes per field (x, y, z, radius)"] = classes
    # non-finite
    nf = {meta[k]["nf"]: ref[k] for k in g["non-finite"] if meta[k]["nf"][0] in ("base", "first", "later", "unused")}
    base = nf[("base",)]
    assert np.isfinite(base["f8"]).all()
    differ = 0
    for key, d in nf.items():
        if key[0] == "unused":
            assert d["f8"].tobytes() == base["f8"].tobytes() and d["rec"].tobytes() == base["rec"].tobytes(), key
        elif key[0] in ("first", "later"):
            assert "inf" not in key[1] or not np.isfinite(d["f8"]).all(), key
            differ += key[0] == "first" and d["f8"].tobytes() != nf[("later",) + key[1:]]["f8"].tobytes()
    infinf = [ref[k] for k in g["non-finite"] if meta[k]["nf"] == ("infinf",)][0]
    assert any(x != x for n in infinf["normals"] for x in n) and any(x == 0 for n in infinf["normals"] for x in n)  # inf / inf next to finite / inf
    assert np.isinf(nf[("later", "+inf", (0,))]["f8"][3])  # a growth step with d = inf
    assert differ >= 1  # the order of the points changes the result
    reached["non-finite: cases whose result depends on where the value sits"] = differ
    reached["non-finite: meshlets with a NaN cutoff argument (q is NaN)"] = sum(1 for k in g["non-finite"] if ref[k]["q"] is not None and ref[k]["q"] != ref[k]["q"])
    assert reached["non-finite: meshlets with a NaN cutoff argument (q is NaN)"] >= 1
    kept = [ref[k]["kept"] for k in g["random"]]
    reached["random: meshlets with a sphere / with a real cone / with a non-finite result"] = (
        sum(1 for x in kept if x), sum(1 for k in g["random"] if ref[k]["q"] is not None), sum(1 for k in g["random"] if not np.isfinite(ref[k]["f8"]).all()))
    assert min(reached["random: meshlets with a sphere / with a real cone / with a non-finite result"]) >= 50
    reached["meshlets"] = len(meshlets)
    return reached


def build():
    """(meshlets, data, vertices, names); the arrays are shared and read-only: copy before writing"""
    return _built()[:4]


def groups():
    return _built()[4]


def reference():
    """bounds_ref's result per meshlet (computed once)"""
    return _built()[5]


def conditions():
    return _built()[6]
