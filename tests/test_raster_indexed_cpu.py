"""nv_rasterdepth_indexed on the CPU: its ABI, the reference of the indexed path (tests/raster_indexed_ref.c) against the
cluster path's reference on the same triangles, and each skip rule on hand-built draws."""
import os
import re

import numpy as np
import pytest

import raster_indexed_ref as RI
import raster_ref as RR
from niagara_amd import layouts as L
from niagara_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="session")
def rref(tmp_path_factory):
    return RR.load(tmp_path_factory.mktemp("raster_ref_ix"))


@pytest.fixture(scope="session")
def iref(tmp_path_factory):
    return RI.load(tmp_path_factory.mktemp("raster_indexed_ref"))


def test_abi_declares_and_exports_rasterdepth_indexed():
    from niagara_amd import _lib
    header = open(os.path.join(ROOT, "include", "niagara_vis.h")).read()
    assert re.search(r"\bint nv_rasterdepth_indexed\(", header)
    assert "nv_rasterdepth_indexed" in _lib.EXPORTS and hasattr(_lib.lib, "nv_rasterdepth_indexed")


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


def _draws(rng, n, dist):
    d = np.zeros(n, dtype=L.MESHDRAW)
    for i in range(n):
        q = rng.normal(size=4)
        q[3] = abs(q[3]) + 2.0  # mostly facing the camera
        d[i]["orientation"] = (q / np.linalg.norm(q)).astype(np.float32)
        d[i]["position"] = (rng.uniform(-3, 3), rng.uniform(-2, 2), -dist * rng.uniform(0.8, 1.3))
        d[i]["scale"] = rng.uniform(0.3, 1.2)
    return d


@pytest.mark.parametrize("post_pass", [0, 1])
@pytest.mark.parametrize("case", range(4))
def test_indexed_reference_equals_cluster_reference(case, post_pass, rref, iref):
    """the same triangles under the same draws: depth bit for bit, triangles rasterised and samples covered equal; commands and triangles
    count the draws and their index ranges"""
    rng = np.random.default_rng(70 + case)
    vp = [(97, 61), (17, 9), (1, 1), (333, 207)][case]
    if case % 2:
        pos = rng.normal(0, 2.0, (300, 3))
        tris = rng.integers(0, 300, (400, 3)).tolist()  # random triples: slivers, both facings, degenerate ones
    else:
        pos, tris = _grid(14, 9, 4.0, 3.0, 0.3, seed=case)
    draws = _draws(rng, 5, 9.0)
    s = RR.mesh_scene(pos, tris, vp, draws=draws, flags=dict(postPass=post_pass))
    dc, _, tc = rref.raster(*RR.raster_args(s), *vp)
    ix = RI.from_mesh_scene(s, tris)
    di, ti = iref.raster(ix["g"], ix["commands"], ix["count"], ix["draws"], ix["indices"], ix["vertices"], *vp)
    assert di.view(np.uint32).tobytes() == dc.view(np.uint32).tobytes()
    assert ti[2:].tolist() == tc[2:].tolist() and ti[0] == 5 and ti[1] == 5 * len(tris)
    assert ti[2] > 0 and (vp == (1, 1) or ti[3] > 0)


def _one_quad(vp=(64, 48)):
    """two front-facing triangles filling most of the screen, one draw"""
    pos = [(-2, -1.5, 0), (2, -1.5, 0), (2, 1.5, 0), (-2, 1.5, 0)]
    tris = [(0, 1, 2), (0, 2, 3)]
    d = np.zeros(1, dtype=L.MESHDRAW)
    d["position"], d["scale"], d["orientation"] = (0.0, 0.0, -4.0), 1.0, (0, 0, 0, 1)
    s = RR.mesh_scene(pos, tris, vp, draws=d)
    return RI.from_mesh_scene(s, tris), vp


def _run(iref, ix, vp, **kw):
    args = dict(commands=ix["commands"], count=ix["count"], draws=ix["draws"], indices=ix["indices"], vertices=ix["vertices"])
    args.update(kw)
    return iref.raster(ix["g"], args.pop("commands"), args.pop("count"), args.pop("draws"), args.pop("indices"), args.pop("vertices"), *vp, **args)


def test_skip_rules(iref):
    ix, vp = _one_quad()
    d0, t0 = _run(iref, ix, vp)
    assert t0.tolist()[:3] == [1, 2, 2] and t0[3] > 0
    half = lambda t: int(t[3])
    # an index position at or past indexCapacity: the second triangle's last index is out
    d, t = _run(iref, ix, vp, index_capacity=5)
    assert t.tolist()[:3] == [1, 2, 1] and 0 < half(t) < half(t0)
    # 0xFFFFFFFF (no primitive restart) and a corner at or past vertexCapacity
    ind = ix["indices"].copy()
    ind[4] = 0xFFFFFFFF
    d, t = _run(iref, ix, vp, indices=ind)
    assert t[2] == 1
    d, t = _run(iref, ix, vp, vertex_capacity=3)  # triangle 1 names vertex 3
    assert t[2] == 1
    # vertexOffset wraps mod 2^32: indices + 2^32 - 4 + 4 name the same vertices
    c = ix["commands"].copy()
    c["vertexOffset"] = 2 ** 32 - 4
    d, t = _run(iref, ix, vp, commands=c, indices=ix["indices"] + 4)
    assert d.tobytes() == d0.tobytes() and t.tolist() == t0.tolist()
    # remainder indices are ignored; instanceCount 0 skips the command, > 1 draws the same depth
    c = ix["commands"].copy()
    c["indexCount"] = 5
    d, t = _run(iref, ix, vp, commands=c)
    assert t.tolist()[:3] == [1, 1, 1]
    c = ix["commands"].copy()
    c["instanceCount"] = 0
    d, t = _run(iref, ix, vp, commands=c)
    assert t.tolist() == [0, 0, 0, 0] and not d.any()
    c["instanceCount"] = 7
    d, t = _run(iref, ix, vp, commands=c)
    assert d.tobytes() == d0.tobytes() and t.tolist() == t0.tolist()
    # drawId >= drawCount
    c = ix["commands"].copy()
    c["drawId"] = 1
    d, t = _run(iref, ix, vp, commands=c)
    assert t.tolist() == [0, 0, 0, 0]
    # a count above drawCount reads drawCount commands; a zero count reads none
    d, t = _run(iref, ix, vp, count=1000)
    assert d.tobytes() == d0.tobytes() and t.tolist() == t0.tolist()
    d, t = _run(iref, ix, vp, count=0)
    assert t.tolist() == [0, 0, 0, 0]
    # zero capacities: nothing is read
    d, t = _run(iref, ix, vp, index_capacity=0)
    assert t.tolist()[:3] == [1, 2, 0]
    d, t = _run(iref, ix, vp, vertex_capacity=0)
    assert t.tolist()[:3] == [1, 2, 0]


def test_commands_select_their_index_ranges(iref):
    """firstIndex picks the range; two commands over disjoint halves write what one command over both writes"""
    ix, vp = _one_quad()
    d0, t0 = _run(iref, ix, vp)
    two = RI.commands_for([(0, 3), (3, 3)], draw_ids=[0, 0])
    d, t = _run(iref, ix, vp, commands=two, count=2, draws=np.concatenate([ix["draws"], ix["draws"]]))
    assert d.tobytes() == d0.tobytes() and t.tolist()[1:] == t0.tolist()[1:] and t[0] == 2


def test_occluder_scene_indexed_keeps_occluder_scene():
    """the indexed variant only adds the index buffer and the LODs' index ranges; its triangles are the meshlets' triangles"""
    import oracle
    a = synth.occluder_scene(meshlet_bounds=oracle.meshlet_bounds)
    b = synth.occluder_scene_indexed(meshlet_bounds=oracle.meshlet_bounds)
    for k in ("meshlets", "draws", "data", "vertices", "cull"):
        assert a[k].tobytes() == b[k].tobytes(), k
    lods = b["meshes"]["lods"]
    assert (lods["indexCount"][:, 0] == a["meshes"]["lods"]["indexCount"][:, 0]).all()
    assert int(lods["indexOffset"][1, 0]) == int(lods["indexCount"][0, 0]) and len(b["indices"]) == int(lods["indexCount"][:, 0].sum())
    strip = lambda m: m.copy()
    ma, mb = strip(a["meshes"]), strip(b["meshes"])
    ma["lods"]["indexOffset"] = mb["lods"]["indexOffset"] = 0
    assert ma.tobytes() == mb.tobytes()
    assert int(b["indices"].max()) < max(int(b["meshes"]["vertexCount"][0]), int(b["meshes"]["vertexCount"][1]))
