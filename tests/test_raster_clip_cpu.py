"""Near-plane clipping of the depth rasterisers (NV_OPT_RASTER_NEAR_CLIP) on the CPU: the clip reference
(tests/raster_clip_ref.c) against the unclipped references, against the analytic plane (coverage and depth), on the cases of the rule, cluster
path against indexed path; plus the ABI of the option."""
import os
import re

import numpy as np
import pytest

import oracle
import raster_clip_ref as RC
import raster_indexed_ref as RI
import raster_ref as RR
import test_raster_cpu as T
from niagara_amd import layouts as L
from niagara_amd import synth
from scenes import make_triangle_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="session")
def rref(tmp_path_factory):
    return RR.load(tmp_path_factory.mktemp("raster_ref_clip"))


@pytest.fixture(scope="session")
def iref(tmp_path_factory):
    return RI.load(tmp_path_factory.mktemp("raster_indexed_ref_clip"))


@pytest.fixture(scope="session")
def clib(tmp_path_factory):
    return RC.load(tmp_path_factory.mktemp("raster_clip_ref"))


def test_abi_declares_the_option():
    from niagara_amd import pipeline as P
    header = open(os.path.join(ROOT, "include", "niagara_vis.h")).read()
    m = re.search(r"#define NV_OPT_RASTER_NEAR_CLIP (\d+)", header)
    assert m and int(m.group(1)) == 10 == P.NV_OPT_RASTER_NEAR_CLIP


def _bits(d):
    return d.view(np.uint32).tobytes()


# ---- 1. off means off

@pytest.mark.parametrize("case", range(len(T.CAMERAS)))
def test_off_equals_the_unclipped_references(case, rref, iref, clib):
    s = make_triangle_scene(seed=40 + case, **T.CAMERAS[case])
    cib, cc4 = T._cluster_list(s)
    w, h = s["viewport"]
    for pp in (0, 1):
        g = s["globals"].copy()
        g["cullData"]["postPass"] = pp
        args = (g, s["commands"], s["draws"], s["meshlets"], s["data"], s["vertices"], cib, cc4)
        a, b = rref.raster(*args, w, h, visibility=True), clib.cluster(0).raster(*args, w, h, visibility=True)
        assert _bits(a[0]) == _bits(b[0]) and a[1].tobytes() == b[1].tobytes() and a[2].tolist() == b[2].tolist()
        ix = RI.from_cluster_scene(s)
        ia = (g, ix["commands"], ix["count"], ix["draws"], ix["indices"], ix["vertices"], w, h)
        c, d = iref.raster(*ia), clib.indexed(0).raster(*ia)
        assert _bits(c[0]) == _bits(d[0]) and c[1].tolist() == d[1].tolist()
        assert a[2][2] > 0


# ---- 2. no crossing, no change

def test_no_crossing_no_change(rref, clib):
    """scenes without a triangle that has both inside and outside vertices: the option changes no bit"""
    scenes = [RR.mesh_scene(*T._grid(31, 17, 20.0, 10.0, 0.3, seed=3), (97, 61), draws=T._at(12.0)),  # everything in front
              RR.mesh_scene([(-1, -1, 3), (1, -1, 3), (0, 1, 3), (-1, -1, -5), (1, -1, -5), (0, 1, -5)], [(0, 1, 2), (3, 4, 5)], (64, 48))]  # one behind
    for s in scenes:
        assert RC.crossing_triangles(rref, s) == 0
        w, h = s["viewport"]
        ref = clib.cluster(1)
        a, b = rref.raster(*RR.raster_args(s), w, h, visibility=True), ref.raster(*RR.raster_args(s), w, h, visibility=True)
        assert ref.stats[RC.CROSSING] == 0
        assert _bits(a[0]) == _bits(b[0]) and a[1].tobytes() == b[1].tobytes() and a[2].tolist() == b[2].tolist() and a[2][3] > 0


# ---- 3 / 4. the ground plane

def _grid(nx, ny, half_w, half_h, jitter, seed):
    """test_raster_cpu._grid's construction (a copy: a jittered tessellated rectangle at z = 0, border vertices on the border)"""
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


HALF_W, HALF_H = 24.0, 40.0  # exact in fp16, as are the border coordinates +-24 and +-40 the outline runs through


def ground_plane(viewport, seed=5):
    """a floor 1.5 units under niagara's default camera: 48 wide, from 10 units behind the camera to 70 ahead, 6 x 8 quads (10 units long:
    whole rows of triangles cross the near plane), the grid's +z turned to +y"""
    pos, tris = _grid(6, 8, HALF_W, HALF_H, 0.3, seed)
    d = np.zeros(1, dtype=L.MESHDRAW)
    r = np.float32(np.sqrt(0.5))
    d["position"], d["scale"], d["orientation"] = (0.0, -1.5, -30.0), 1.0, (-r, 0.0, 0.0, r)
    return RR.mesh_scene(pos, tris, viewport, draws=d), tris


def _plane_forms(s):
    """fp64: the plane (u, v, 0) under the draw's transform and the camera as clip = A u + B v + C (the transform is linear in the position)"""
    g, d = s["g"], s["draws"][0]
    P = np.asarray(g["projection"], np.float64).reshape(4, 4).T  # stored column-major
    V = np.asarray(g["cullData"]["view"], np.float64).reshape(4, 4).T
    q = np.asarray(d["orientation"], np.float64)
    sc, pos = float(d["scale"]), np.asarray(d["position"], np.float64)

    def world(p):
        t = np.cross(q[:3], p) + q[3] * p
        return (p + 2.0 * np.cross(q[:3], t)) * sc + pos

    def clip(p):
        return P @ (V @ np.append(world(np.asarray(p, np.float64)), 1.0))
    C = clip((0, 0, 0))
    return clip((1, 0, 0)) - C, clip((0, 1, 0)) - C, C


def plane_truth(s):
    """per pixel centre, in fp64: covered (the view ray hits the rectangle in front of the near plane), the distance in pixels to the nearest
    line of the outline that decides it (inside: to the outline; outside: a lower bound of it), z = clip.z / clip.w of the hit and its
    screen-space gradient magnitude"""
    w, h = s["viewport"]
    A, B, C = _plane_forms(s)

    def forms(x, y):  # x, y: pixel coordinates (row 0 at the top)
        nx, ny = x / w * 2.0 - 1.0, (h - y) / h * 2.0 - 1.0
        a11, a12, b1 = A[0] - nx * A[3], B[0] - nx * B[3], -(C[0] - nx * C[3])
        a21, a22, b2 = A[1] - ny * A[3], B[1] - ny * B[3], -(C[1] - ny * C[3])
        D = a11 * a22 - a12 * a21
        Du, Dv = b1 * a22 - a12 * b2, a11 * b2 - b1 * a21
        Wn = A[3] * Du + B[3] * Dv + C[3] * D
        Zn = A[2] * Du + B[2] * Dv + C[2] * D
        sg = np.where(D < 0, -1.0, 1.0)
        # every one of these is affine in (x, y) (the products' x y terms cancel): a straight line on the screen
        return np.stack([sg * (HALF_W * D - Du), sg * (HALF_W * D + Du), sg * (HALF_H * D - Dv), sg * (HALF_H * D + Dv), sg * (Wn - Zn)]), sg * Wn, sg * Zn

    ys, xs = np.mgrid[0:h, 0:w]
    x, y = xs + 0.5, ys + 0.5
    Lk, Wn, Zn = forms(x, y)
    Lx, Wx, Zx = forms(x + 1.0, y)
    Ly, Wy, Zy = forms(x, y + 1.0)
    norm = np.sqrt((Lx - Lk) ** 2 + (Ly - Lk) ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        dist = Lk / norm
        front = Wn > 0
        covered = front & (dist >= 0).all(axis=0)
        edge = np.where(covered, dist.min(axis=0), np.where(front, -np.where(dist < 0, dist, 0).min(axis=0), np.inf))
        z = Zn / Wn
        zx, zy = ((Zx - Zn) * Wn - Zn * (Wx - Wn)) / Wn ** 2, ((Zy - Zn) * Wn - Zn * (Wy - Wn)) / Wn ** 2
    return covered, edge, z, np.sqrt(zx ** 2 + zy ** 2)


PLANE_VIEWPORTS = [(320, 192), (97, 61), (64, 64), (131, 77), (13, 7), (1, 1)]


@pytest.mark.parametrize("viewport", PLANE_VIEWPORTS)
def test_clipped_ground_plane_is_watertight_and_is_the_plane(viewport, rref, clib):
    """Tests 3 and 4 of the issue.  No sample is covered twice; the covered set is the set of centres whose view ray hits the rectangle
    (centres within 1/128 pixel of its projected outline left out); the depth is the plane's within 2^-20 (seven fp32 roundings on terms
    <= 1) + |grad z| / 128 (two 1/256-pixel snaps).  Largest deviation seen at 320 x 192: see DESIGN.md §4.10."""
    s, tris = ground_plane(viewport)
    w, h = viewport
    ref = clib.cluster(1)
    depth, _, tot = ref.raster(*RR.raster_args(s), w, h)
    assert ref.stats[RC.CROSSING] >= 12 and ref.stats[RC.CLIPPED] == ref.stats[RC.CROSSING]  # whole rows cross; every new vertex inside the guard band
    assert RC.crossing_triangles(rref, s) == ref.stats[RC.CROSSING]
    assert tot[3] == (depth > 0).sum()
    if w < 64:
        return
    covered, edge, z, grad = plane_truth(s)
    sure = edge >= 1.0 / 128.0
    share = float((covered & ~sure).sum()) / float(covered.sum())
    print("viewport %s: covered %d, left out %d (%.3f %%)" % (viewport, covered.sum(), (covered & ~sure).sum(), 100 * share))
    assert share <= 0.02
    assert ((depth > 0) == covered)[sure].all()
    unclipped = rref.raster(*RR.raster_args(s), w, h)[0]
    assert (covered & sure & (unclipped == 0)).sum() > w * h // 10  # without the option a large part of the set stays at 0
    m = covered & sure
    dev = np.abs(depth.astype(np.float64) - z)[m]
    bound = (2.0 ** -20 + grad / 128.0)[m]
    print("viewport %s: largest depth deviation %.3e (%.3f of its bound)" % (viewport, dev.max(), (dev / bound).max()))
    assert (dev <= bound).all()


@pytest.mark.parametrize("seed", range(3))
def test_clipped_fan_with_its_hub_behind_the_camera(seed, clib):
    """a fan on the floor whose hub lies behind the camera: every spoke crosses the near plane; no sample twice, and the union is what the
    rim polygon covers (compared with the same floor as one fan from a hub in front)"""
    rng = np.random.default_rng(seed)
    vp = (int(rng.integers(40, 120)), int(rng.integers(30, 90)))
    rim = [(-20.0, 30.0), (-20.0, 8.0), (-20.0, -30.0), (-3.0, -30.0), (9.0, -30.0), (20.0, -30.0), (20.0, 11.0), (20.0, 30.0), (2.0, 30.0)]  # counter-clockwise in (x, y)
    d = np.zeros(1, dtype=L.MESHDRAW)
    r = np.float32(np.sqrt(0.5))
    d["position"], d["scale"], d["orientation"] = (0.0, -1.5, -20.0), 1.0, (-r, 0.0, 0.0, r)  # grid y = 30 is 50 ahead, y = -30 is 10 behind
    n = len(rim)
    out = []
    for hub in ((float(rng.uniform(-2, 2)), float(rng.uniform(-26.0, -22.0))), (0.5, 9.0)):  # 2 - 6 units behind the camera; 29 ahead
        pos = [(hub[0], hub[1], 0.0)] + [(x, y, 0.0) for x, y in rim]
        tris = [(0, 1 + i, 1 + (i + 1) % n) for i in range(n)]
        ref = clib.cluster(1)
        s = RR.mesh_scene(pos, tris, vp, draws=d)
        depth, _, tot = ref.raster(*RR.raster_args(s), *vp)
        assert tot[3] == (depth > 0).sum() and tot[3] > vp[0] * vp[1] // 4
        out.append((depth > 0, ref.stats.copy()))
    assert out[0][1][RC.CLIPPED] == n - 3 and out[0][1][RC.REFUSED_VERTEX] == 0  # the hub behind: every triangle crosses but the three on the far-behind edge
    # both fans tile the same rectangle
    differ = int((out[0][0] != out[1][0]).sum())
    assert differ <= 2 * (vp[0] + vp[1])  # only centres on the snapped outline may fall differently


# ---- 5. the cases of the rule

TRI_FRONT = [(-1, -1, -5), (1, -1, -5)]  # two vertices in front (counter-clockwise with a third one above them)


def _one(pos, tris, clib, near_clip=1, vp=(64, 48), flags=None, visibility=True, patch=None):
    s = RR.mesh_scene(pos, tris, vp, flags=flags)
    if patch:
        patch(s)
    ref = clib.cluster(near_clip)
    depth, vis, tot = ref.raster(*RR.raster_args(s), *vp, visibility=visibility)
    return depth, vis, tot, ref.stats


def test_one_vertex_outside_gives_two_pieces(clib):
    depth, vis, tot, st = _one(TRI_FRONT + [(0, 1, 3)], [(0, 1, 2)], clib)
    assert tot.tolist() == [1, 1, 2, int((depth > 0).sum())] and tot[3] > 0 and st.tolist() == [1, 1, 0, 0]
    assert depth.max() == 1.0 or depth[0].max() > 0  # the pieces run to the near plane: off the top of the screen or depth 1
    assert np.unique(vis[vis != 0] & 0xffffffff).tolist() == [0]  # both pieces carry the triangle's id (slot 0, triangle 0)
    assert _one(TRI_FRONT + [(0, 1, 3)], [(0, 1, 2)], clib, near_clip=0)[2].tolist() == [1, 1, 0, 0]


def test_visibility_ids_of_both_pieces(clib):
    """triangle 1 of the meshlet is the clipped one: both pieces write id 1; the order of the vertices does not matter for the count"""
    pos = [(-4, -1, -5), (-2, -1, -5), (-3, 1, -5)] + TRI_FRONT + [(0, 1, 3)]  # triangle 0 stands to the left of the clipped one
    for order in ((3, 4, 5), (4, 5, 3), (5, 3, 4)):
        depth, vis, tot, st = _one(pos, [(0, 1, 2), order], clib)
        assert tot[2] == 3 and st[RC.CLIPPED] == 1
        ids = np.unique(vis[vis != 0] & 0x7f).tolist()
        assert ids == [0, 1]
        assert (vis >> 32).astype(np.uint32).tobytes() == depth.view(np.uint32).tobytes()


def test_rotations_of_a_crossing_triangle_cover_the_same_samples(clib):
    """the fan starts at another vertex for each stored order, the union stays the polygon (interior samples; depth on the diagonal may
    differ in the last bit)"""
    for third in ((0, 1, 3), (0.3, 0.5, 0.5)):
        for base in ([(-1, -1, -5), (1, -1, -5), third], [(-1, -1, 2), (1, -1, -5), (0, 1, -6)]):  # one outside / (second base) one or two outside
            cov = []
            for order in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
                depth, _, tot, _ = _one(base, [order], clib, visibility=False)
                assert tot[3] == (depth > 0).sum() and tot[3] > 0
                cov.append(depth > 0)
            assert (cov[0] == cov[1]).all() and (cov[0] == cov[2]).all()


def test_two_vertices_outside_give_one_piece(clib):
    depth, _, tot, st = _one([(-1, -1, 3), (0, -1, -5), (1, 1, 3)], [(0, 1, 2)], clib, flags=dict(postPass=1))
    assert tot.tolist() == [1, 1, 1, int((depth > 0).sum())] and tot[3] > 0 and st.tolist() == [1, 1, 0, 0]


def test_three_vertices_outside_draw_nothing(clib):
    depth, _, tot, st = _one([(-1, -1, 3), (1, -1, 3), (0, 1, 0.5)], [(0, 1, 2)], clib, flags=dict(postPass=1))
    assert tot.tolist() == [1, 1, 0, 0] and st.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_non_finite_clip_component_refuses_the_triangle(value, clib):
    """clip.x of every vertex made non-finite through the projection's translation column (P[12] * 1): crossing triangles are refused for
    the rule, not clipped"""
    def patch(s):
        s["g"]["projection"][0][12] = value
    depth, _, tot, st = _one(TRI_FRONT + [(0, 1, 3)], [(0, 1, 2)], clib, patch=patch, visibility=False)
    assert tot.tolist() == [1, 1, 0, 0] and st.tolist() == [1, 0, 1, 0]


def test_outside_vertex_with_non_negative_d_refuses_the_triangle(clib):
    """a hand-made projection with clip.w = vz and clip.z = 2 vz - 3 (vz = -z under the default camera): inside iff 0 < vz <= 3.  The vertex at vz = -5 is outside with
    d = w - z = 3 - vz = 8 >= 0 (w <= 0 while z <= w), so the triangle is refused although two vertices are inside"""
    def patch2(s):
        p = s["g"]["projection"][0]
        p[11], p[10], p[14] = 1.0, 2.0, -3.0
    depth, _, tot, st = _one([(-1, -1, -1), (1, -1, -1), (0, 1, 5)], [(0, 1, 2)], clib, patch=patch2, flags=dict(postPass=1), visibility=False)
    assert st.tolist() == [1, 0, 1, 0] and tot.tolist() == [1, 1, 0, 0]


def test_vertex_exactly_on_the_plane_is_inside(rref, clib):
    """d == 0: inside; its crossing edges start at t = 0, so one piece is degenerate and is not counted"""
    # view z = -0.125: with niagara's projection clip.z = znear = 0.1 (fp32) and clip.w = 0.125: not on the plane.  A projection with
    # clip.z = clip.w for vz = -0.125 exactly: P[14] = 0.125
    def patch(s):
        s["g"]["projection"][0][14] = 0.125
    pos = [(-1, -1, -0.125), (1, -1, -5), (0, 1, 3)]
    s = RR.mesh_scene(pos, [(0, 1, 2)], (64, 48), flags=dict(postPass=1))
    patch(s)
    vx = rref.vertices(*RR.raster_args(s))
    assert vx[0, 0, 3] == 1.0 and vx[0, 0, 2] == 0.125  # z / w == 1 exactly: on the plane
    depth, _, tot, st = _one(pos, [(0, 1, 2)], clib, patch=patch, flags=dict(postPass=1), visibility=False)
    assert st.tolist() == [1, 1, 0, 0] and tot[2] == 1 and tot[3] == (depth > 0).sum()


def test_new_vertex_beyond_the_guard_band_refuses_both_pieces(clib):
    """the edge to the outside vertex meets the near plane 4500 units to the side: |sx| of the new vertex > 2^21 at 640 x 480; neither piece is
    drawn"""
    pos = TRI_FRONT + [(60000, 1, 60)]
    depth, _, tot, st = _one(pos, [(0, 1, 2)], clib, vp=(640, 480), flags=dict(postPass=1), visibility=False)
    assert st.tolist() == [1, 0, 0, 1] and tot.tolist() == [1, 1, 0, 0]


def test_back_facing_crossing_triangle_follows_post_pass(clib):
    pos = [(1, -1, -5), (-1, -1, -5), (0, 1, 3)]  # clockwise seen by the camera
    for pp, pieces in ((0, 0), (1, 2)):
        depth, _, tot, st = _one(pos, [(0, 1, 2)], clib, flags=dict(postPass=pp), visibility=False)
        assert st.tolist() == [1, 1, 0, 0] and tot[2] == pieces and (tot[3] > 0) == (pp == 1)


# ---- 6. both paths, same bits

def test_indexed_path_equals_cluster_path_with_clipping(clib):
    """synth.interior_scene: every meshlet of every draw through the cluster path, every draw's index range through the indexed path"""
    s = synth.interior_scene_indexed(meshlet_bounds=oracle.meshlet_bounds)
    draws = s["draws"].copy()
    oracle.assign_visibility_offsets(draws, s["meshes"])
    w, h = s["viewport"]
    cmds, ids = np.zeros(len(draws), dtype=L.TASKCMD), []
    dc = np.zeros(len(draws), dtype=L.DRAWCMD)
    for i, d in enumerate(draws):
        lod = s["meshes"][int(d["meshIndex"])]["lods"][0]
        cmds[i]["drawId"], cmds[i]["taskOffset"], cmds[i]["taskCount"] = i, int(lod["meshletOffset"]), int(lod["meshletCount"])
        ids += [i | j << 24 for j in range(int(lod["meshletCount"]))]
        dc[i]["drawId"], dc[i]["indexCount"], dc[i]["instanceCount"], dc[i]["firstIndex"] = i, int(lod["indexCount"]), 1, int(lod["indexOffset"])
        dc[i]["vertexOffset"] = int(s["meshes"][int(d["meshIndex"])]["vertexOffset"])
    cc4 = np.array([len(ids), 0, 0, 0], np.uint32)
    cib = np.concatenate([np.array(ids, np.uint32), np.zeros(512, np.uint32)])
    oracle.clustersubmit(cc4, cib)
    for pp in (0, 1):
        g = RR.globals_for(s["cull"], (w, h), pp)
        cref, xref = clib.cluster(1), clib.indexed(1)
        a = cref.raster(g, cmds, draws, s["meshlets"], s["data"], s["vertices"], cib, cc4, w, h)
        b = xref.raster(g, dc, len(dc), draws, s["indices"], s["vertices"], w, h)
        assert cref.stats[RC.CLIPPED] >= 16 and cref.stats.tolist() == xref.stats.tolist()
        assert _bits(a[0]) == _bits(b[0]) and a[2][2:].tolist() == b[1][2:].tolist()


# ---- the closed-loop scene's intent (GPU test 10 compares the device with these frames)

@pytest.mark.parametrize("task", [True, False])
def test_interior_scene_hides_its_boxes_only_with_clipping(task, clib):
    s = synth.interior_scene_indexed(meshlet_bounds=oracle.meshlet_bounds)
    for near_clip in (1, 0):
        if task:
            fr = RR.oracle_frames(s, 3, rref=clib.cluster(near_clip))
        else:
            fr = RI.oracle_frames_classic(s, 3, iref=clib.indexed(near_clip))
        dvb = fr[2]["late"]["dvb"]
        assert all(dvb[i] == 1 for i in s["open"] + s["surfaces"])
        assert all(dvb[i] == (0 if near_clip else 1) for i in s["hidden"])
