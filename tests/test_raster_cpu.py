"""nv_rasterdepth's rule set on the CPU: the reference raster (tests/raster_ref.c) against the oracle's vertex stage,
the fill rule, depth, facing, rejections and malformed meshlets; plus the ABI of the new entry point."""
import os
import re

import numpy as np
import pytest

import oracle
import raster_ref as RR
from niagara_amd import layouts as L
from scenes import make_triangle_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="session")
def rref(tmp_path_factory):
    return RR.load(tmp_path_factory.mktemp("raster_ref"))


def test_abi_declares_and_exports_rasterdepth():
    from niagara_amd import _lib
    from niagara_amd import pipeline as P
    header = open(os.path.join(ROOT, "include", "niagara_vis.h")).read()
    m = re.search(r"#define NV_OPT_RASTER_SMALL_LIMIT (\d+)", header)
    assert m and int(m.group(1)) == P.NV_OPT_RASTER_SMALL_LIMIT
    assert re.search(r"\bint nv_rasterdepth\(", header)
    assert "nv_rasterdepth" in _lib.EXPORTS and hasattr(_lib.lib, "nv_rasterdepth")


CAMERAS = [dict(), dict(cam_pos=(3.0, -2.0, 5.0), cam_quat=(0.0, 0.3826834, 0.0, 0.9238795)), dict(cam_pos=(0, 0, -8.0), viewport=(1920, 1080)),
           dict(scene_radius=3.0), dict(scene_radius=6.0, specials=True)]  # tests/test_trianglecull.py's cases


def _cluster_list(s):
    cd = s["cull"].copy()
    cd["clusterBackfaceEnabled"], cd["cullingEnabled"] = 0, 1
    cib, cc4 = np.zeros(s["n"] * 64 + 256, np.uint32), np.zeros(4, np.uint32)
    oracle.clustercull(cd, 0, s["commands"], s["count4"], s["draws"], s["meshlets"], None, None, cib, cc4)
    oracle.clustersubmit(cc4, cib)
    return cib, cc4


def _gl_min(x, y):
    return np.where(y < x, y, x)


def _gl_max(x, y):
    return np.where(x < y, y, x)


@pytest.mark.parametrize("case", range(len(CAMERAS)))
def test_vertex_stage_is_trianglecull_s(case, rref):
    """nv_trianglecull's keep rule recomputed from the reference raster's sx / sy / w equals oracle.trianglecull's masks bit for bit"""
    s = make_triangle_scene(seed=40 + case, **CAMERAS[case])
    cib, cc4 = _cluster_list(s)
    args = (s["globals"], s["commands"], s["draws"], s["meshlets"], s["data"], s["vertices"], cib, cc4)
    vc = rref.vertices(*args)
    slots = int(cc4[2]) * 256
    masks, totals = np.zeros(slots, L.TRIMASK), np.zeros(3, np.uint64)
    oracle.trianglecull(*args, masks, totals)
    d8 = s["data"].view(np.uint8)
    ml = s["meshlets"]
    keep = np.zeros((slots, 96), bool)
    live = 0
    for k in range(slots):
        ci = int(cib[k])
        if ci == 0xffffffff:
            continue
        cmd = s["commands"][ci & 0xffffff]
        m = ml[int(cmd["taskOffset"]) + (ci >> 24)]
        vcount, tcount = int(m["vertexCount"]), min(int(m["triangleCount"]), 96)
        io = (int(m["dataOffset"]) + ((vcount + 1) // 2 if m["shortRefs"] == 1 else vcount)) * 4
        idx = d8[io:io + 3 * tcount].reshape(-1, 3).astype(np.int64) & 63
        pa, pb, pc = vc[k][idx[:, 0]], vc[k][idx[:, 1]], vc[k][idx[:, 2]]
        with np.errstate(invalid="ignore", over="ignore"):
            ebx, eby, ecx, ecy = pb[:, 0] - pa[:, 0], pb[:, 1] - pa[:, 1], pc[:, 0] - pa[:, 0], pc[:, 1] - pa[:, 1]
            culled = ebx * ecy <= eby * ecx
            bminx, bminy = _gl_min(pa[:, 0], _gl_min(pb[:, 0], pc[:, 0])), _gl_min(pa[:, 1], _gl_min(pb[:, 1], pc[:, 1]))
            bmaxx, bmaxy = _gl_max(pa[:, 0], _gl_max(pb[:, 0], pc[:, 0])), _gl_max(pa[:, 1], _gl_max(pb[:, 1], pc[:, 1]))
            sb = np.float32(1.0 / 256.0)
            culled = culled | (np.rint(bminx - sb) == np.rint(bmaxx)) | (np.rint(bminy) == np.rint(bmaxy + sb))
            culled = culled & (pa[:, 2] > 0) & (pb[:, 2] > 0) & (pc[:, 2] > 0)
        keep[k, :tcount] = ~culled
        live += 1
    bits = np.packbits(keep, axis=1, bitorder="little").view(np.uint32)
    assert live > 50
    assert (bits == masks["keep"]).all()


def _grid(nx, ny, half_w, half_h, jitter, seed):
    rng = np.random.default_rng(seed)
    xs, ys = np.linspace(-half_w, half_w, nx + 1), np.linspace(-half_h, half_h, ny + 1)
    pos = np.array([(x, y, 0.0) for y in ys for x in xs], np.float64)
    inner = (np.abs(pos[:, 0]) < half_w) & (np.abs(pos[:, 1]) < half_h)
    pos[inner, :2] += rng.uniform(-jitter, jitter, (int(inner.sum()), 2)) * [2 * half_w / nx, 2 * half_h / ny]
    vid = lambda i, j: j * (nx + 1) + i
    tris = []
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = vid(i, j), vid(i + 1, j), vid(i + 1, j + 1), vid(i, j + 1)
            tris += [(a, b, c), (a, c, d)] if (i + j) % 2 else [(a, b, d), (b, c, d)]
    return pos, tris


def _at(dist):
    d = np.zeros(1, dtype=L.MESHDRAW)
    d["position"], d["scale"], d["orientation"] = (0.0, 0.0, -dist), 1.0, (0, 0, 0, 1)
    return d


@pytest.mark.parametrize("viewport", [(97, 61), (64, 64), (131, 77), (13, 7), (1, 1)])
def test_fill_rule_covers_every_sample_exactly_once(viewport, rref):
    """a jittered, tessellated plane larger than the screen: every pixel centre is covered by exactly one triangle (samples covered ==
    pixels) and the depth of a plane parallel to the screen is one constant"""
    pos, tris = _grid(31, 17, 20.0, 10.0, 0.3, seed=viewport[0])
    s = RR.mesh_scene(pos, tris, viewport, draws=_at(12.0))  # (the screen spans 8.4 units up and down, 8.4 x its aspect across)
    depth, vis, tot = rref.raster(*RR.raster_args(s), *viewport, visibility=True)
    w, h = viewport
    assert tot[3] == w * h and tot[2] <= len(tris)  # (at 1 x 1 a sliver can snap to zero area)
    assert (depth > 0).all() and len(np.unique(depth)) == 1
    assert depth[0, 0] == np.float32(np.float32(0.1) / np.float32(12.0))
    assert len(np.unique(vis & 0xffffffff)) > min(w * h, len(tris)) // 4  # many triangles own samples


@pytest.mark.parametrize("seed", range(4))
def test_fill_rule_fans_of_shared_vertices(seed, rref):
    """triangle fans around one vertex whose rim runs along a rectangle larger than the screen: every centre exactly once"""
    rng = np.random.default_rng(seed)
    vp = (int(rng.integers(5, 90)), int(rng.integers(5, 70)))
    hw, hh = 40.0, 10.0  # (at distance 3 the screen spans 2.1 units up and down, at most 2.1 x 18 across)
    per_side = int(rng.integers(2, 9))
    rim = []
    for (x0, y0), (x1, y1) in (((-hw, -hh), (hw, -hh)), ((hw, -hh), (hw, hh)), ((hw, hh), (-hw, hh)), ((-hw, hh), (-hw, -hh))):
        ts = np.sort(rng.uniform(0, 1, per_side - 1))
        rim += [(x0, y0)] + [(x0 + (x1 - x0) * t, y0 + (y1 - y0) * t) for t in ts]
    c = rng.uniform(-1.0, 1.0, 2)
    pos = [(c[0], c[1], 0.0)] + [(x, y, 0.0) for x, y in rim]
    n = len(rim)
    tris = [(0, 1 + i, 1 + (i + 1) % n) for i in range(n)]  # counter-clockwise seen from +z
    s = RR.mesh_scene(pos, tris, vp, draws=_at(3.0))
    depth, _, tot = rref.raster(*RR.raster_args(s), *vp)
    assert tot[3] == vp[0] * vp[1] and (depth > 0).all()


def test_facing_follows_post_pass(rref):
    """postPass 0: front faces (counter-clockwise seen by the camera) only; postPass 1: both; zero area never"""
    pos = [(-3, -1, 0), (-1, -1, 0), (-2, 1, 0), (1, -1, 0), (3, -1, 0), (2, 1, 0), (0, 2, 0), (0.5, 2, 0), (1, 2, 0)]
    tris = [(0, 1, 2), (3, 5, 4), (6, 7, 8)]  # front, back, degenerate
    vp = (64, 48)
    for pp, drawn in ((0, 1), (1, 2)):
        s = RR.mesh_scene(pos, tris, vp, draws=_at(5.0), flags=dict(postPass=pp))
        depth, vis, tot = rref.raster(*RR.raster_args(s), *vp, visibility=True)
        assert tot[2] == drawn and tot[1] == 3
        left, right = depth[:, :vp[0] // 2], depth[:, vp[0] // 2:]
        assert (left > 0).any() and ((right > 0).any() == (pp == 1))
        tri_ids = np.unique(vis[vis != 0] & 0x7f)
        assert tri_ids.tolist() == ([0] if pp == 0 else [0, 1])


def test_near_plane_and_guard_band_rejections_are_counted(rref):
    """a vertex behind the camera, one at the near plane's wrong side and one past the 2^21-pixel guard band each reject their triangle"""
    pos = [(-1, -1, -5), (1, -1, -5), (0, 1, -5),   # drawn
           (-1, -1, -5), (1, -1, -5), (0, 1, 3),    # behind the camera
           (-1, -1, -5), (1, -1, -5), (0, 1, -0.05),  # in front of the near plane (z < znear = 0.1)
           (-1, -1, -5), (1, -1, -5), (60000, 1, -0.2)]  # |sx| > 2^21
    tris = [(0, 1, 2), (3, 4, 5), (6, 7, 8), (9, 10, 11)]
    vp = (64, 48)
    s = RR.mesh_scene(pos, tris, vp)
    vx = rref.vertices(*RR.raster_args(s))
    assert abs(vx[0, 11, 0]) >= 2 ** 21 and vx[0, 5, 2] < 0 and vx[0, 8, 3] > 1  # (the cases are what they claim)
    depth, _, tot = rref.raster(*RR.raster_args(s), *vp)
    assert tot.tolist() == [1, 4, 1, int((depth > 0).sum())] and tot[3] > 0


def test_malformed_meshlets_follow_the_documented_rule(rref):
    """index bytes >= min(vertexCount, 64) reject their triangle; triangleCount above 96 walks 96 (totals count the stored byte)"""
    pos, tris = _grid(12, 8, 6.0, 4.0, 0.0, seed=1)
    s = RR.mesh_scene(pos, tris, (80, 60), draws=_at(4.0))
    ml, d8 = s["meshlets"], s["data"].view(np.uint8)
    base = rref.raster(*RR.raster_args(s), 80, 60)[2]
    vc0, tc0 = int(ml[0]["vertexCount"]), int(ml[0]["triangleCount"])
    io = (int(ml[0]["dataOffset"]) + vc0) * 4
    d8[io + 1] = vc0  # triangle 0 names a vertex the meshlet does not have
    d8[io + 5] = 200                     # triangle 1: beyond 64 whatever the count
    _, _, tot = rref.raster(*RR.raster_args(s), 80, 60)
    assert tot[2] == base[2] - 2 and tot[1] == base[1]
    ml["triangleCount"][0] = 250  # reads 96 triangles' bytes: the rest of this meshlet's words and the next meshlet's refs as indices
    _, _, tot2 = rref.raster(*RR.raster_args(s), 80, 60)
    assert int(tot2[1]) == int(base[1]) - tc0 + 250 and tc0 < 96
