"""The rule set of nv_visibility_attributes on the CPU: tests/visattr_ref.c in fp32 against its fp64 build and against
geometry worked out independently in numpy.  No GPU.

Error bounds are derived, not fitted.  With u = 2^-24 and gamma(k) = k u / (1 - k u), a value computed by a fixed expression tree of depth k
in fp32 differs from the exact value of the same expression by at most gamma(k) times the expression evaluated with every term replaced by
its magnitude (the standard model; Higham, Accuracy and Stability, §3).  The depths along the vertex stage, counting every rounding:
rotateQuat 6 (cross: mul, sub; + q.w v: mul... add; cross: mul, sub; v + 2 u: add — the longest path), * scale + position 2 more (wpos: <= 11
is used), the view product 4 more (<= 15), the projection 4 more (<= 19: the clip coordinates).  From there `lambda_bound` follows the
barycentric statements one by one (each difference of products adds the propagated input error plus gamma(2) of its magnitude; the
quotient adds one rounding), and `point_bound` the interpolation (gamma(3)).  Where |s| does not exceed its own error bound the bound is
infinite (nothing is claimed there); the tests require that this happens at no shaded pixel of their scenes."""
import os
import re

import numpy as np
import pytest

import oracle
import raster_ref as RR
import visattr_ref as VA
import visbuffer_ref as VB
from niagara_amd import _lib as N
from niagara_amd import host, synth
from niagara_amd import layouts as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def gamma(k):
    return k * U / (1.0 - k * U)


@pytest.fixture(scope="session")
def vref(tmp_path_factory):
    return VB.load(tmp_path_factory.mktemp("visbuffer_ref_attr_cpu"))


@pytest.fixture(scope="session")
def aref(tmp_path_factory):
    return VA.load(tmp_path_factory.mktemp("visattr_ref_cpu"))


# ---- 0. the interface

def test_entry_point_layouts_and_header():
    assert "nv_visibility_attributes" in N.EXPORTS and hasattr(N.lib, "nv_visibility_attributes")
    assert L.MATERIAL.itemsize == 64 and L.PIXELATTR.itemsize == 64
    assert [L.MATERIAL.fields[n][1] for n in ("diffuseFactor", "specularFactor", "emissiveFactor", "padding")] == [16, 32, 48, 60]
    assert [L.PIXELATTR.fields[n][1] for n in ("uv", "bary", "normal", "drawId", "tangent", "wpos", "materialIndex")] == [0, 8, 16, 28, 32, 48, 60]
    h = open(os.path.join(ROOT, "include", "niagara_vis.h")).read()
    assert re.search(r"static_assert\(sizeof\(NvMaterial\) == 64", h) and re.search(r"static_assert\(sizeof\(NvPixelAttributes\) == 64", h)


# ---- the independent fp64 geometry and the bounds

def _abs_cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] + b[..., 1] * a[..., 2], a[..., 2] * b[..., 0] + b[..., 2] * a[..., 0],
                     a[..., 0] * b[..., 1] + b[..., 0] * a[..., 1]], -1)


def _matrices(g):
    M = g["cullData"]["view"][0].astype(np.float64).reshape(4, 4).T  # column-major
    P = g["projection"][0].astype(np.float64).reshape(4, 4).T
    return M, P


def corner_chain(s, draws, g, records):
    """For every record (n): the vertex ids of its triangle's corners decoded in numpy, and the vertex stage in fp64 next to its magnitude
    expression: dict of clip (n, 3, 4), a_clip, wpos (n, 3, 3), a_wpos, uv (n, 3, 2)"""
    rec = np.ascontiguousarray(records, L.VISRECORD).reshape(-1)
    keys, inv = np.unique(rec[["drawId", "meshletIndex", "triangle"]], return_inverse=True)
    d16, d8, data = s["data"].view(np.uint16), s["data"].view(np.uint8), s["data"]
    vid = np.zeros((len(keys), 3), np.int64)
    for k, (d, mi, t) in enumerate(keys.tolist()):
        m = s["meshlets"][mi]
        vc, off, short = int(m["vertexCount"]), int(m["dataOffset"]), m["shortRefs"] == 1
        io = (off + ((vc + 1) // 2 if short else vc)) * 4 + 3 * t
        idx = d8[io:io + 3].astype(np.int64)
        vid[k] = (d16[off * 2 + idx] if short else data[off + idx]).astype(np.int64) + int(m["baseVertex"])
    v = s["vertices"][vid]
    p = np.stack([v["vx"], v["vy"], v["vz"]], -1).view(np.float16).astype(np.float64)  # (k, 3, 3)
    uv = np.stack([v["tu"], v["tv"]], -1).view(np.float16).astype(np.float64)
    dr = draws[keys["drawId"]]
    q = dr["orientation"].astype(np.float64)[:, None, :]
    qv, qw = q[..., :3], q[..., 3:]
    sc, pos = dr["scale"].astype(np.float64)[:, None, None], dr["position"].astype(np.float64)[:, None, :]
    t = np.cross(qv, p) + qw * p
    rot = p + 2.0 * np.cross(qv, t)
    a_t = _abs_cross(np.abs(qv) + 0 * p, np.abs(p)) + np.abs(qw) * np.abs(p)
    a_rot = np.abs(p) + 2.0 * _abs_cross(np.abs(qv) + 0 * p, a_t)
    wpos, a_w = rot * sc + pos, a_rot * np.abs(sc) + np.abs(pos)
    M, P = _matrices(g)
    one = np.ones(wpos.shape[:-1] + (1,))
    v4, a_v = np.concatenate([wpos, one], -1) @ M.T, np.concatenate([a_w, one], -1) @ np.abs(M).T
    clip, a_c = v4 @ P.T, a_v @ np.abs(P).T
    return dict(clip=clip[inv], a_clip=a_c[inv], wpos=wpos[inv], a_wpos=a_w[inv], uv=uv[inv])


def pixel_ndc(w, h):
    px, py = np.meshgrid(np.arange(w), np.arange(h))
    return ((px.reshape(-1) + 0.5) / w) * 2.0 - 1.0, 1.0 - ((py.reshape(-1) + 0.5) / h) * 2.0


def lambda_bound(ch, nx, ny):
    """(lambda (n, 3) in fp64 from the independent chain, its fp32 error bound (n, 3)) following DESIGN.md §4.13's statements"""
    x, y, w = ch["clip"][..., 0], ch["clip"][..., 1], ch["clip"][..., 3]
    ex, ey, ew = (gamma(19) * ch["a_clip"][..., k] for k in (0, 1, 3))
    e_n = 3.0 * U  # fx / W: one rounding of a value below 1; * 2 exact; - 1: one rounding of a value of magnitude <= 1
    nx, ny = nx[:, None], ny[:, None]
    dx, dy = x - nx * w, y - ny * w
    edx = ex + np.abs(nx) * ew + e_n * (np.abs(w) + ew) + gamma(2) * (np.abs(x) + np.abs(nx * w))
    edy = ey + np.abs(ny) * ew + e_n * (np.abs(w) + ew) + gamma(2) * (np.abs(y) + np.abs(ny * w))
    pdx, pdy = np.abs(dx) + edx, np.abs(dy) + edy
    b, eb = np.zeros_like(dx), np.zeros_like(dx)
    for i, (j, k) in enumerate(((1, 2), (2, 0), (0, 1))):
        b[:, i] = dx[:, j] * dy[:, k] - dy[:, j] * dx[:, k]
        m1, m2 = pdx[:, j] * pdy[:, k], pdy[:, j] * pdx[:, k]
        eb[:, i] = (m1 - np.abs(dx[:, j] * dy[:, k])) + (m2 - np.abs(dy[:, j] * dx[:, k])) + gamma(2) * (m1 + m2)
    sm = b.sum(axis=1)
    es = eb.sum(axis=1) + gamma(2) * (np.abs(b) + eb).sum(axis=1)
    lam = b / sm[:, None]
    room = np.abs(sm) - es
    with np.errstate(divide="ignore", invalid="ignore"):
        el = (eb + np.abs(lam) * es[:, None]) / room[:, None]
        el = el + U * (np.abs(lam) + el)
    el[room <= 0] = np.inf
    return lam, el


def point_bound(lam, el, a, ea):
    """error bound of (l0 a0 + l1 a1) + l2 a2 in fp32 against sum(lam64 a64): a (n, 3, c) corner values, ea their error bounds"""
    pl = (np.abs(lam) + el)[..., None]
    with np.errstate(invalid="ignore"):  # (an infinite lambda bound times a zero: no bound there either)
        return np.nan_to_num((pl * ea).sum(axis=1) + (el[..., None] * np.abs(a)).sum(axis=1) + gamma(3) * (pl * (np.abs(a) + ea)).sum(axis=1), nan=np.inf)


def _plane_scene():
    """a tessellated plane (occluder_scene's wall alone) tilted about two axes"""
    s = synth.occluder_scene(hidden=0, beside=0, meshlet_bounds=oracle.meshlet_bounds)
    q = np.array([0.35, -0.25, 0.1, 0.0])
    q[3] = np.sqrt(1.0 - (q[:3] ** 2).sum())
    s["draws"]["orientation"][0] = q.astype(np.float32)
    s["draws"]["materialIndex"][0] = 1
    return s, 0


def _scene(name):
    if name == "plane":
        s, clip = _plane_scene()
    elif name == "occluder":
        s, clip = synth.occluder_scene(meshlet_bounds=oracle.meshlet_bounds), 0
    elif name == "interior":
        s, clip = synth.interior_scene(meshlet_bounds=oracle.meshlet_bounds), 1
    else:
        s, clip = VA.kitten_scene(meshlet_bounds=oracle.meshlet_bounds), 0
    mat = s["draws"]["materialIndex"].copy()
    s = VA.with_attributes(s)
    if name == "plane":
        s["draws"]["materialIndex"] = mat
    return s, clip


_CACHE = {}


def _frame(name, vref, aref):
    if name not in _CACHE:
        s, clip = _scene(name)
        rec, out = VA.reference_frame(s, clip, vref, aref)
        w, h = s["viewport"]
        g = RR.globals_for(s["cull"], (w, h))
        o64 = aref.attributes(g, rec["resolve"]["records"], w, h, rec["draws"], s["meshlets"], s["data"], s["vertices"], s["materials"], real="f64")
        _CACHE[name] = (s, rec, g, out, o64)
    return _CACHE[name]


# ---- 1. reprojection, lambdas against the double build

@pytest.mark.parametrize("name", ["plane", "occluder", "interior"])
def test_wpos_reprojects_to_the_pixel_centre_and_lambdas_agree_with_the_double_build(name, vref, aref):
    s, rec, g, out, o64 = _frame(name, vref, aref)
    w, h = s["viewport"]
    sh = (out["flags"] & VA.SHADED) != 0
    # non-vacuity: a fifth of the screen is shaded, nothing invalid or degenerate; the interior scene shows near-clipped triangles
    assert sh.mean() >= 0.2 and out["totals"][1] == 0 and out["totals"][2] == 0 and out["totals"].tolist() == o64["totals"].tolist()
    if name == "interior":
        assert ((out["flags"] & VA.CLIPPED) != 0).sum() > 1000
    if name != "plane":
        assert len(np.unique(out["ids"][sh, 1])) >= 3
    ch = corner_chain(s, rec["draws"], g, rec["resolve"]["records"].reshape(-1)[sh])
    nx, ny = pixel_ndc(w, h)
    lam, el = lambda_bound(ch, nx[sh], ny[sh])
    assert np.isfinite(el).all() and np.median(el) < 1e-4
    # the independent chain agrees with the double build (fp64 noise only)
    assert np.abs(lam[:, 1:] - o64["bary"][sh]).max() < 1e-9
    d = np.abs(out["bary"][sh].astype(np.float64) - o64["bary"][sh])
    ratio_l = float((d / el[:, 1:]).max())
    assert (d <= el[:, 1:]).all(), ratio_l
    # wpos: the interpolated fp32 point within its bound of the fp64 point, and through view * projection in fp64 on the pixel centre
    ew = point_bound(lam, el, ch["wpos"], gamma(11) * ch["a_wpos"])
    dw = np.abs(out["wpos"][sh].astype(np.float64) - o64["wpos"][sh])
    assert (dw <= ew).all(), float((dw / ew).max())
    M, P = _matrices(g)
    W4 = np.concatenate([out["wpos"][sh].astype(np.float64), np.ones((int(sh.sum()), 1))], -1)
    c = W4 @ M.T @ P.T
    ec = ew @ np.abs(M[:, :3]).T @ np.abs(P).T
    assert (c[:, 3] > ec[:, 3]).all()
    ndc = c[:, :2] / c[:, 3:]
    en = (ec[:, :2] + np.abs(ndc) * ec[:, 3:]) / (c[:, 3:] - ec[:, 3:]) + 1e-12
    dev = np.abs(ndc - np.stack([nx[sh], ny[sh]], -1)) * np.array([w, h]) / 2.0
    bound = en * np.array([w, h]) / 2.0
    ratio_p = float((dev / bound).max())
    print("%s: %d shaded; lambda error / bound <= %.3f (largest error %.3g); reprojection error / bound <= %.3f (largest %.3g px, median bound %.3g px)"
          % (name, int(sh.sum()), ratio_l, float(d.max()), ratio_p, float(dev.max()), float(np.median(bound))))
    assert (dev <= bound).all(), ratio_p
    assert np.median(bound) < 0.05  # the bound says something: a twentieth of a pixel


# ---- 2. watertight attributes

def test_two_triangles_sharing_an_edge_give_the_same_uv(aref):
    """a flat 8 x 8 grid whose positions and texcoords are exact in fp16, so that uv is one affine function of the plane: the two triangles of
    a quad, each evaluated at the samples on both sides of their shared edge, must give the same uv up to their rounding-error bounds"""
    pos, groups = synth._grid_meshlets(8, 8, 4)
    tris = [t for grp in groups for t in grp]
    draws = np.zeros(1, L.MESHDRAW)
    q = np.array([0.3, 0.2, -0.1, 0.0])
    q[3] = np.sqrt(1.0 - (q[:3] ** 2).sum())
    draws["scale"], draws["orientation"], draws["position"] = 3.0, q.astype(np.float32), (0.2, -0.1, -6.0)
    w, h = 192, 128
    s = RR.mesh_scene(pos, tris, (w, h), draws=draws)
    s["vertices"] = VA.fill_attributes(s["vertices"], s["meshlets"], s["data"])
    uvh = np.stack([s["vertices"]["tu"], s["vertices"]["tv"]], -1).view(np.float16).astype(np.float64)
    assert np.array_equal(uvh, pos[:, :2].astype(np.float64) * 0.5 + 0.5)  # exact: the planar map survives fp16
    nx, ny = pixel_ndc(w, h)
    checked = 0
    for mi, t0 in ((0, 10), (1, 4), (0, 40)):  # triangles 2k and 2k + 1 are the halves (a, b, c), (a, c, d) of one quad
        outs = []
        for t in (t0, t0 + 1):
            rec = np.zeros(w * h, L.VISRECORD)
            rec["meshletIndex"], rec["triangle"] = mi, t
            o = aref.attributes(s["g"], rec, w, h, s["draws"], s["meshlets"], s["data"], s["vertices"])
            ch = corner_chain(s, s["draws"], s["g"], rec)
            lam, el = lambda_bound(ch, nx, ny)
            zero = np.zeros_like(ch["uv"])
            outs.append((o, lam, el, point_bound(lam, el, ch["uv"], zero)))
        (oa, la, ela, ea), (ob, lb, elb, eb) = outs
        # samples of the quad near the diagonal a-c, on either side: the vertex off the edge (b: index 1 of the first half; d: index 2 of the
        # second) has a small weight of either sign in its own triangle
        near = (np.abs(la[:, 1]) < 0.3) & (np.abs(lb[:, 2]) < 0.3) & (la[:, 0] > 0) & (la[:, 2] > 0) & np.isfinite(ea).all(axis=1) & np.isfinite(eb).all(axis=1)
        assert near.sum() > 20 and (la[near, 1] < 0).any() and (la[near, 1] > 0).any()
        d = np.abs(oa["uv"][near].astype(np.float64) - ob["uv"][near].astype(np.float64))
        assert (d <= ea[near] + eb[near]).all()
        assert (ea[near] + eb[near]).max() < 1e-3  # the bound says something: uv spans [0, 1] over the grid, a quad an eighth of it
        checked += int(near.sum())
    assert checked > 100


# ---- 3. the homogeneous form

@pytest.mark.parametrize("behind", [1, 2])
def test_near_clipped_triangle_interpolates_the_planes_true_attributes(behind, vref, aref):
    """one triangle of the plane y = -1 with one / two vertices behind the camera, rasterised with near-plane clipping: on its visible pixels
    wpos is the point where the pixel's ray meets the plane and uv the planar map of it (fp64 ray casting, no barycentrics)"""
    pos = np.array([(-5, -1, -10), (5, -1, -10), (0, -1, 5)] if behind == 1 else [(-5, -1, 5), (5, -1, 5), (0, -1, -10)], np.float32)
    tris = [(0, 1, 2)] if behind == 1 else [(0, 2, 1)]  # counter-clockwise seen from above
    w, h = 160, 96
    s = RR.mesh_scene(pos, tris, (w, h))
    s["vertices"] = VA.fill_attributes(s["vertices"], s["meshlets"], s["data"])
    g = RR.globals_for(s["cull"], (w, h), 1)  # both faces
    _, vis, _ = vref.raster(g, s["commands"], s["draws"], s["meshlets"], s["data"], s["vertices"], s["cib"], s["cc4"], w, h, near_clip=1)
    covered = vis.reshape(-1) != 0
    assert covered.sum() > w * h // 10
    rec = np.zeros(w * h, L.VISRECORD)
    rec["drawId"] = np.where(covered, 0, 0xFFFFFFFF)
    o = aref.attributes(g, rec, w, h, s["draws"], s["meshlets"], s["data"], s["vertices"])
    assert o["totals"].tolist() == [int(covered.sum()), 0, 0, 0] and ((o["flags"][covered] & VA.CLIPPED) != 0).all()
    ch = corner_chain(s, s["draws"], g, rec[covered])
    assert ((ch["clip"][..., 3] <= 0).sum(axis=1) == behind).all()
    nx, ny = pixel_ndc(w, h)
    lam, el = lambda_bound(ch, nx[covered], ny[covered])
    assert np.isfinite(el).all()
    M, P = _matrices(g)
    Mi = np.linalg.inv(M)
    # clip = P v: x = P00 vx, y = P11 vy, w = vz (synth.make_globals), so the pixel's view-space ray is (nx / P00, ny / P11, 1) t
    dirs = np.stack([nx[covered] / P[0, 0], ny[covered] / P[1, 1], np.ones(int(covered.sum()))], -1) @ Mi[:3, :3].T
    origin = Mi[:3, 3]
    t = (-1.0 - origin[1]) / dirs[:, 1]
    true_w = origin + t[:, None] * dirs
    true_uv = np.stack([true_w[:, 0] + 0.25 * true_w[:, 2], true_w[:, 1] - 0.25 * true_w[:, 2]], -1) * 0.5 + 0.5
    ew = point_bound(lam, el, ch["wpos"], gamma(11) * ch["a_wpos"]) + 1e-9
    euv = point_bound(lam, el, ch["uv"], np.zeros_like(ch["uv"])) + 1e-9
    dw, duv = np.abs(o["wpos"][covered] - true_w), np.abs(o["uv"][covered] - true_uv)
    print("behind %d: %d pixels, wpos error / bound <= %.3f, uv error / bound <= %.3f" % (behind, int(covered.sum()), (dw / ew).max(), (duv / euv).max()))
    assert (dw <= ew).all() and (duv <= euv).all()
    assert np.median(ew) < 1e-3 and np.median(euv) < 1e-3


# ---- 4. the encode

@pytest.mark.parametrize("name", ["occluder", "interior", "kitten"])
def test_gbuffers_decode_to_what_was_shaded(name, vref, aref):
    s, rec, g, out, o64 = _frame(name, vref, aref)
    w, h = s["viewport"]
    sh = (out["flags"] & VA.SHADED) != 0
    # gbuffer1: R, G decode (decodeOct) to the normalised interpolated normal.  Each channel is off by at most half a code (the rounding) plus
    # the deband term, |deband| (0.5 / 1023) <= half a code: 1 / 1023 in e, 2 / 1023 in the octahedral coordinate.  decodeOct moves x and y by
    # up to that plus the fold's t (4 / 1023: it sums both) and z by 4 / 1023: a vector error of at most sqrt(36 + 36 + 16) / 1023 before
    # the normalisation, whose input has L1 norm 1, hence length >= 1 / sqrt(3): at most 9.4 sqrt(3) / 1023 = 0.0159 after it.
    g1 = out["gbuffer1"][sh]
    e = np.stack([g1 & 1023, g1 >> 10 & 1023], -1).astype(np.float64) / 1023.0 * 2.0 - 1.0
    n = o64["normal"][sh]
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    err = np.linalg.norm(VA.decode_oct(e) - n, axis=1)
    print("%s: decoded normal error <= %.4f (bound 0.0159)" % (name, err.max()))
    assert err.max() <= np.sqrt(88.0) * np.sqrt(3.0) / 1023.0 + 1e-5
    mats = s["materials"][out["ids"][sh, 1]]
    spec = np.clip(mats["specularFactor"][:, 3].astype(np.float64), 0, 1) * 1023.0
    assert (np.abs((g1 >> 20 & 1023).astype(np.float64) - spec) <= 0.5 + 1e-3).all() and (g1 >> 30 == 0).all()
    # gbuffer0: albedo^(1 / 2.2) and log2(1 + emissivef) / 5 in fp64 numpy, half a code
    g0 = out["gbuffer0"][sh]
    want = np.power(np.clip(mats["diffuseFactor"][:, :3].astype(np.float64), 0, None), 1.0 / 2.2)
    lum = lambda c: c[:, 0] * 0.3 + c[:, 1] * 0.6 + c[:, 2] * 0.1
    em = np.log2(1.0 + lum(mats["emissiveFactor"].astype(np.float64)) / (lum(mats["diffuseFactor"].astype(np.float64)) + 1e-3)) / 5.0
    want = np.clip(np.concatenate([want, em[:, None]], -1), 0, 1) * 255.0
    got = np.stack([g0 >> k & 255 for k in (0, 8, 16, 24)], -1).astype(np.float64)
    assert (np.abs(got - want) <= 0.5 + 1e-3).all()
    # the restatement in fp32 against its double build: within one code, and at least 90 % of the channels equal (the share the GPU test asks)
    c64 = np.stack([o64["gbuffer0"][sh] >> k & 255 for k in (0, 8, 16, 24)], -1).astype(np.int64)
    assert np.abs(got.astype(np.int64) - c64).max() <= 1 and (got.astype(np.int64) == c64).mean() >= 0.9
    # a material that names textures is shaded from its factors, and counted
    textured = out["ids"][:, 1][sh] == 2
    assert textured.any() and out["totals"][3] == textured.sum() == ((out["flags"] & VA.TEXTURED) != 0).sum()
    plain = s["materials"].copy()
    for f in ("albedoTexture", "normalTexture", "specularTexture", "emissiveTexture"):
        plain[f] = 0
    o2 = aref.attributes(g, rec["resolve"]["records"], w, h, rec["draws"], s["meshlets"], s["data"], s["vertices"], plain)
    assert o2["gbuffer0"].tobytes() == out["gbuffer0"].tobytes() and o2["gbuffer1"].tobytes() == out["gbuffer1"].tobytes() and o2["totals"][3] == 0
    # no sample: zeros with drawId all ones, both words 0
    assert (out["gbuffer0"][~sh] == 0).all() and (out["gbuffer1"][~sh] == 0).all()
    blank = out["attributes"][~sh]
    assert (blank["drawId"] == 0xFFFFFFFF).all() and not blank.view(np.uint32).reshape(-1, 16)[:, [c for c in range(16) if c != 7]].any()


# ---- 5. validation

def invalid_cases(s, records):
    """The frame's records with hand-made ones of one invalid class each among them: a list of (records, meshlets, data, capacity overrides,
    the number of records made invalid).  Shared with tests/test_visattr_gpu.py."""
    base = np.ascontiguousarray(records, L.VISRECORD).reshape(-1)
    named = np.nonzero(base["drawId"] != 0xFFFFFFFF)[0]
    pick = named[::37]
    cases = []

    def case(edit=None, meshlets=None, data=None, counts=None, count=None):
        r = base.copy()
        if edit is not None:
            edit(r)
        cases.append((r, s["meshlets"] if meshlets is None else meshlets, s["data"] if data is None else data, counts or {}, len(pick) if count is None else count))

    def draw_past(r):
        r["drawId"][pick] = len(s["draws"])
        r["drawId"][pick[::2]] = 0xFFFFFFFE
    case(draw_past)

    def meshlet_past(r):
        r["meshletIndex"][pick] = len(s["meshlets"])
        r["meshletIndex"][pick[::2]] = 0xFFFFFFFF
    case(meshlet_past)

    def triangle_past(r):
        r["triangle"][pick] = s["meshlets"]["triangleCount"][r["meshletIndex"][pick]]
        r["triangle"][pick[::2]] = 96
        r["triangle"][pick[::3]] = 0xFFFFFFFF
    case(triangle_past)
    # an index byte at or past the vertex count: triangle 0 of the wall's first meshlet
    m0 = s["meshlets"][0]
    d = s["data"].copy()
    d.view(np.uint8)[(int(m0["dataOffset"]) + int(m0["vertexCount"])) * 4 + 1] = int(m0["vertexCount"])
    hit = int(((base["meshletIndex"] == 0) & (base["triangle"] == 0) & (base["drawId"] != 0xFFFFFFFF)).sum())

    def first_triangle(r):
        r["meshletIndex"][pick], r["triangle"][pick] = 0, 0
        r["drawId"][pick] = 0
    case(first_triangle, data=d, count=len(pick) + hit - int(np.isin(pick, np.nonzero((base["meshletIndex"] == 0) & (base["triangle"] == 0))[0]).sum()))
    # a vertex reference that resolves past the vertex buffer (the wall's references are 32-bit words)
    assert m0["shortRefs"] == 0
    d2 = s["data"].copy()
    i0 = int(d2.view(np.uint8)[(int(m0["dataOffset"]) + int(m0["vertexCount"])) * 4])
    d2[int(m0["dataOffset"]) + i0] = 0xFFFFFFF0
    case(first_triangle, data=d2, count=1)
    # capacities: half the data words, half the vertices, two materials, one draw, one meshlet
    for counts in (dict(data=len(s["data"]) // 2), dict(data=int(s["meshlets"]["dataOffset"][-1]) + 1), dict(vertices=len(s["vertices"]) // 2),
                   dict(materials=2), dict(draws=1), dict(meshlets=1)):
        case(counts=counts, count=1)
    return cases


def test_every_invalid_class_is_counted_and_written_like_no_sample(vref, aref):
    s, rec, g, out, _ = _frame("occluder", vref, aref)
    w, h = s["viewport"]
    base = rec["resolve"]["records"].reshape(-1)
    for records, meshlets, data, counts, expect in invalid_cases(s, base):
        o = aref.attributes(g, records, w, h, rec["draws"], meshlets, data, s["vertices"], s["materials"], counts=counts)
        inv = (o["flags"] & VA.INVALID) != 0
        assert o["totals"][1] == inv.sum() >= expect > 0, (counts, int(inv.sum()), expect)
        assert o["totals"][0] + o["totals"][1] == (records["drawId"] != 0xFFFFFFFF).sum() and o["totals"][0] > 0
        changed = np.nonzero((records != base))[0]
        assert inv[changed].all()
        a = o["attributes"][inv]
        assert (a["drawId"] == 0xFFFFFFFF).all() and not a.view(np.uint32).reshape(-1, 16)[:, [c for c in range(16) if c != 7]].any()
        assert (o["gbuffer0"][inv] == 0).all() and (o["gbuffer1"][inv] == 0).all()
        # every other pixel is what the frame's records give
        same = ~inv
        assert o["attributes"][same].tobytes() == out["attributes"][same].tobytes() and (o["gbuffer1"][same] == out["gbuffer1"][same]).all()


def test_degenerate_triangle_is_counted_and_takes_its_first_corner(aref):
    """a triangle of three equal vertices: s = 0 at every pixel -> lambda = (1, 0, 0), counted"""
    pos = np.array([(0.5, 0.25, -4.0)] * 3, np.float32)
    s = RR.mesh_scene(pos, [(0, 1, 2)], (16, 8))
    s["vertices"] = VA.fill_attributes(s["vertices"], s["meshlets"], s["data"])
    rec = np.zeros(16 * 8, L.VISRECORD)
    o = aref.attributes(s["g"], rec, 16, 8, s["draws"], s["meshlets"], s["data"], s["vertices"])
    assert o["totals"].tolist() == [128, 0, 128, 0]
    assert (o["bary"] == 0).all() and np.allclose(o["wpos"], pos[0]) and np.isfinite(o["vals"]).all()
