"""nv_rasterdepth_indexed on the MI355X: depth and totals bit-identical to the CPU reference (tests/raster_indexed_ref.c) on
random indexed scenes with every skip rule, equal to nv_rasterdepth on the same triangles, balanced over one huge draw and over many tiny ones;
and niagara's classic frame (VisibilityPipeline.frame(task=False)) bit-identical to the oracle chain, phase by phase."""
import json
import os

import numpy as np
import pytest

import oracle
import raster_indexed_ref as RI
import raster_ref as RR
from niagara_amd import host, synth
from niagara_amd import layouts as L
from scenes import make_triangle_scene

INT_MAX = 2 ** 31 - 1
HERE = os.path.dirname(os.path.abspath(__file__))
CAMERAS = [dict(), dict(cam_pos=(3.0, -2.0, 5.0), cam_quat=(0.0, 0.3826834, 0.0, 0.9238795)), dict(cam_pos=(0, 0, -8.0), viewport=(1920, 1080)),
           dict(scene_radius=3.0), dict(scene_radius=6.0, specials=True),  # tests/test_raster_gpu.py's camera set
           dict(viewport=(333, 207)), dict(viewport=(17, 9), scene_radius=6.0), dict(viewport=(1, 1), scene_radius=4.0)]


@pytest.fixture(scope="session")
def iref(tmp_path_factory):
    return RI.load(tmp_path_factory.mktemp("raster_indexed_ref_gpu"))


@pytest.fixture(scope="session")
def rref(tmp_path_factory):
    return RR.load(tmp_path_factory.mktemp("raster_ref_ix_gpu"))


@pytest.fixture(scope="module")
def ctx():
    from niagara_amd import pipeline as P
    c = P.Context()
    yield c
    c.close()


def _dev(a, dev, empty_bytes):
    import torch
    from niagara_amd import pipeline as P
    return P.to_device(a, dev) if len(a) else torch.zeros(empty_bytes, dtype=torch.uint8, device=dev)


def _gpu(ctx, g, commands, count, draws, indices, vertices, w, h, limit=None, depth=None, draw_count=None, index_capacity=None,
         vertex_capacity=None):
    """nv_rasterdepth_indexed through Context.rasterdepth_indexed: (depth, totals)"""
    import torch
    from niagara_amd import pipeline as P
    dev = ctx.device
    if limit is not None:
        ctx.set_option(P.NV_OPT_RASTER_SMALL_LIMIT, limit)
    try:
        dcb = _dev(np.ascontiguousarray(commands, L.DRAWCMD), dev, 24)
        dccb = P.to_device(np.array([count, 0, 0, 0], np.uint32), dev)
        db, ib, vb = _dev(draws, dev, 48), _dev(np.ascontiguousarray(indices, np.uint32), dev, 4), _dev(vertices, dev, 16)
        d = torch.zeros((h, w), dtype=torch.float32, device=dev) if depth is None else torch.from_numpy(np.ascontiguousarray(depth)).to(dev)
        tot = torch.zeros(4, dtype=torch.int64, device=dev)
        ctx.rasterdepth_indexed(g, dcb, dccb, db, len(draws) if draw_count is None else draw_count, ib,
                                len(indices) if index_capacity is None else index_capacity, vb,
                                len(vertices) if vertex_capacity is None else vertex_capacity, d, w, h, tot)
        ctx.status()
        return d.cpu().numpy(), tot.cpu().numpy().view(np.uint64)
    finally:
        ctx.set_option(P.NV_OPT_RASTER_SMALL_LIMIT, 16)


def _same(gpu, ref):
    assert gpu[1].tolist() == ref[1].tolist()
    assert gpu[0].view(np.uint32).tobytes() == ref[0].view(np.uint32).tobytes()


def _args(ix):
    return ix["commands"], ix["count"], ix["draws"], ix["indices"], ix["vertices"]


def _perturb(ix):
    """every skip rule on a few commands: instanceCount 0 and 5, drawId past drawCount, remainder indices, a wrapping vertexOffset, a
    0xFFFFFFFF index, a last range that runs past the index buffer, and a count above drawCount"""
    c, ind = ix["commands"].copy(), ix["indices"].copy()
    n = len(c)
    assert n > 8
    c[1]["instanceCount"] = 0
    c[2]["drawId"] = n + 3
    c[3]["instanceCount"] = 5
    c[4]["indexCount"] += 2
    f, k = int(c[5]["firstIndex"]), int(c[5]["indexCount"])
    c[5]["vertexOffset"] = 2 ** 32 - 7
    ind[f:f + k] += np.uint32(7)
    if int(c[6]["indexCount"]) >= 3:
        ind[int(c[6]["firstIndex"]) + 1] = 0xFFFFFFFF
    c[n - 1]["indexCount"] += 30
    return dict(ix, commands=c, indices=ind, count=n + 9)


@pytest.mark.gpu
@pytest.mark.parametrize("limit", [None, 0, INT_MAX])
@pytest.mark.parametrize("case", range(len(CAMERAS)))
def test_hip_equals_reference(case, limit, ctx, iref):
    s = make_triangle_scene(seed=140 + case, n_draws=200, commands_per_draw=3, **CAMERAS[case])
    ix = _perturb(RI.from_cluster_scene(s))
    w, h = s["viewport"]
    for pp in (0, 1):
        g = RR.globals_for(s["cull"], (w, h), pp)
        ref = iref.raster(g, *_args(ix), w, h)
        _same(_gpu(ctx, g, *_args(ix), w, h, limit=limit), ref)
        assert ref[1][0] == 198 and ref[1][2] > 0 and (w * h < 1000 or ref[1][3] > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [0, 2, 4])
def test_hip_equals_cluster_path(case, ctx):
    """GPU indexed == GPU nv_rasterdepth on the same triangles under the same draws: depth bits, triangles rasterised, samples"""
    import torch
    from niagara_amd import pipeline as P
    s = make_triangle_scene(seed=240 + case, n_draws=200, commands_per_draw=3, **CAMERAS[case])
    ix = RI.from_cluster_scene(s)
    w, h = s["viewport"]
    for pp in (0, 1):
        g = RR.globals_for(s["cull"], (w, h), pp)
        di, ti = _gpu(ctx, g, *_args(ix), w, h)
        t = [P.to_device(a, ctx.device) for a in (s["commands"], s["draws"], s["meshlets"], s["data"], s["vertices"], ix["cib"], ix["cc4"])]
        dc = torch.zeros((h, w), dtype=torch.float32, device=ctx.device)
        tc = torch.zeros(4, dtype=torch.int64, device=ctx.device)
        ctx.rasterdepth(g, *t, dc, w, h, None, tc)
        ctx.status()
        tc = tc.cpu().numpy()
        assert di.view(np.uint32).tobytes() == dc.cpu().numpy().view(np.uint32).tobytes()
        assert ti[2:].tolist() == tc[2:].tolist() and ti[2] > 0


def _grid(nx, ny, half_w, half_h):
    xs, ys = np.linspace(-half_w, half_w, nx + 1), np.linspace(-half_h, half_h, ny + 1)
    pos = np.array([(x, y, 0.0) for y in ys for x in xs], np.float32)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny))
    a = (j * (nx + 1) + i).reshape(-1)
    b, c, d = a + 1, a + nx + 2, a + nx + 1
    return pos, np.stack([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], 1).reshape(-1).astype(np.uint32)


def _vertices(pos):
    v = np.zeros(len(pos), dtype=L.VERTEX)
    hp = np.asarray(pos, np.float32).astype(np.float16)
    v["vx"], v["vy"], v["vz"] = (hp[:, k].view(np.uint16) for k in range(3))
    return v


def _draw_at(positions, scale=1.0):
    d = np.zeros(len(positions), dtype=L.MESHDRAW)
    d["position"], d["scale"], d["orientation"] = positions, scale, (0, 0, 0, 1)
    return d


@pytest.mark.gpu
def test_hip_one_huge_draw_and_many_tiny_ones(ctx, iref):
    """a single 120 k-triangle command (the balance case: every wave of the launch takes a share of one command), and 100 k one-triangle
    commands, at every raster path split"""
    w, h = 640, 480
    cd = host.build_cull_data(viewport=(w, h))
    g = RR.globals_for(cd, (w, h))
    pos, ind = _grid(300, 200, 6.0, 4.0)
    assert len(ind) == 3 * 120000
    draws = _draw_at([(0.3, -0.2, -5.0)])
    for limit in (None, 0, INT_MAX):
        ref = iref.raster(g, RI.commands_for([(0, len(ind))]), 1, draws, ind, _vertices(pos), w, h)
        _same(_gpu(ctx, g, RI.commands_for([(0, len(ind))]), 1, draws, ind, _vertices(pos), w, h, limit=limit), ref)
    assert ref[1][2] == 120000 and ref[1][3] > w * h // 2
    rng = np.random.default_rng(5)
    n = 100000
    tri = rng.normal(0, 0.05, (n, 3, 3)).astype(np.float32)
    tri[:, 1, 0] += 0.1
    tri[:, 2, 1] += 0.1  # counter-clockwise seen from +z
    draws = _draw_at(np.stack([rng.uniform(-4, 4, n), rng.uniform(-3, 3, n), rng.uniform(-12, -5, n)], 1).astype(np.float32))
    ind = np.arange(3 * n, dtype=np.uint32)
    cmds = RI.commands_for([(3 * i, 3) for i in range(n)])
    ref = iref.raster(g, cmds, n, draws, ind, _vertices(tri.reshape(-1, 3)), w, h)
    _same(_gpu(ctx, g, cmds, n, draws, ind, _vertices(tri.reshape(-1, 3)), w, h), ref)
    assert ref[1][0] == n and ref[1][2] > n // 2


@pytest.mark.gpu
def test_hip_zero_count_and_skipped_commands_leave_the_target_alone(ctx):
    s = make_triangle_scene(seed=7, n_draws=20, commands_per_draw=1)
    ix = RI.from_cluster_scene(s)
    w, h = s["viewport"]
    loaded = np.random.default_rng(8).uniform(0, 1, (h, w)).astype(np.float32)
    skipped = ix["commands"].copy()
    skipped["instanceCount"][::2] = 0
    skipped["drawId"][1::2] = 1000
    for commands, count, kw in ((ix["commands"], 0, {}), (skipped, 20, {}), (ix["commands"], 20, dict(index_capacity=0)),
                                (ix["commands"], 20, dict(vertex_capacity=0))):
        d, tot = _gpu(ctx, s["globals"], commands, count, ix["draws"], ix["indices"], ix["vertices"], w, h, depth=loaded, **kw)
        assert d.tobytes() == loaded.tobytes() and tot[2:].tolist() == [0, 0]
        assert tot[0] == (0 if count == 0 or commands is skipped else 20)


@pytest.mark.gpu
def test_hip_argument_checks(ctx):
    import torch
    from niagara_amd import pipeline as P
    from niagara_amd._lib import NvError
    s = make_triangle_scene(seed=3, n_draws=4, commands_per_draw=1, viewport=(64, 48))
    ix = RI.from_cluster_scene(s)
    dev = ctx.device
    dcb, db = P.to_device(ix["commands"], dev), P.to_device(ix["draws"], dev)
    dccb = P.to_device(np.array([4, 0, 0, 0], np.uint32), dev)
    ib, vb = P.to_device(ix["indices"], dev), P.to_device(ix["vertices"], dev)
    d = torch.zeros((48, 64), dtype=torch.float32, device=dev)
    ni, nv = len(ix["indices"]), len(ix["vertices"])
    g = s["globals"]
    for w, h in ((65, 48), (64, 47), (0, 48)):
        with pytest.raises(NvError):
            ctx.rasterdepth_indexed(g, dcb, dccb, db, 4, ib, ni, vb, nv, d, w, h)
    big = g.copy()
    big["screenWidth"], big["screenHeight"] = 16385, 48
    with pytest.raises(NvError):
        ctx.rasterdepth_indexed(big, dcb, dccb, db, 4, ib, ni, vb, nv, d, 16385, 48)
    for bad in ((None, dccb, db, ib, vb, d), (dcb, None, db, ib, vb, d), (dcb, dccb, None, ib, vb, d), (dcb, dccb, db, None, vb, d),
                (dcb, dccb, db, ib, None, d), (dcb, dccb, db, ib, vb, None)):
        with pytest.raises(NvError):
            ctx.rasterdepth_indexed(g, bad[0], bad[1], bad[2], 4, bad[3], ni, bad[4], nv, bad[5], 64, 48)
    with pytest.raises(NvError, match="NV_ENOMEM"):  # more command slots than nv_create reserved (1 M): a pass never allocates
        ctx.rasterdepth_indexed(g, dcb, dccb, db, (1 << 20) + 1, ib, ni, vb, nv, d, 64, 48)
    ctx.rasterdepth_indexed(g, dcb, dccb, db, 4, ib, ni, vb, nv, d, 64, 48)
    ctx.status()


def _kitten_scene(n_draws, scene_radius, viewport=(1024, 768)):
    b = json.load(open(os.path.join(HERE, "golden", "kitten_bounds.json")))
    vertices, indices, _ = RI.kitten_geometry()
    meshes = np.zeros(1, dtype=L.MESH)
    meshes["center"], meshes["radius"] = np.array(b["center"], np.float32), np.float32(b["radius"])
    meshes["vertexCount"], meshes["lodCount"] = len(vertices), 1
    meshes["lods"]["indexCount"][0, 0], meshes["lods"]["meshletCount"][0, 0] = len(indices), 1
    meshlets = np.zeros(64, dtype=L.MESHLET)
    draws = host.synth_draws(n_draws, 1, scene_radius)
    pw, ph = host.previous_pow2(viewport[0]), host.previous_pow2(viewport[1])
    cd = host.build_cull_data(viewport=viewport, pyramid=(pw, ph), draw_count=n_draws, cullingEnabled=1, occlusionEnabled=1)
    return dict(meshes=meshes, meshlets=meshlets, draws=draws, indices=indices, vertices=vertices, cull=cd, viewport=viewport)


@pytest.mark.gpu
def test_hip_kitten_1024(ctx, iref):
    """BASELINE config 1's mesh drawn 1024 times at 1024 x 768 (every draw, as one command each)"""
    s = _kitten_scene(1024, 25.0)
    w, h = s["viewport"]
    cmds = RI.commands_for([(0, len(s["indices"]))] * 1024)
    g = RR.globals_for(s["cull"], (w, h))
    ref = iref.raster(g, cmds, 1024, s["draws"], s["indices"], s["vertices"], w, h)
    _same(_gpu(ctx, g, cmds, 1024, s["draws"], s["indices"], s["vertices"], w, h), ref)
    assert ref[1][1] == 1024 * 28944 and ref[1][3] > 0


# ---- the classic closed loop

def _gpu_frames(s, frames, fused, post_pass):
    from niagara_amd import pipeline as P
    pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], task_capacity=4096, cluster_capacity=4096 * 64, fused=fused,
                                vertices=s["vertices"], indices=s["indices"])
    out = []
    try:
        for _ in range(frames):
            rec = {}

            def grab(name):
                c4 = pipe.dccb.cpu().numpy().view(np.uint32).copy()
                rec[name] = dict(count4=c4, commands=P.from_device(pipe.dcb[:int(c4[0]) * L.DRAWCMD.itemsize], L.DRAWCMD).copy(),
                                 dvb=pipe.dvb.cpu().numpy().view(np.uint32).copy(), depth=pipe.depth.cpu().numpy().copy())
            pipe.frame(s["cull"], post_pass=post_pass, on_phase=grab, task=False)
            rec["pyramid"] = pipe.pyramid.data.cpu().numpy().copy()
            out.append(rec)
        pipe.ctx.status()
    finally:
        pipe.ctx.close()
    return out


def _occluder():
    return synth.occluder_scene_indexed(meshlet_bounds=oracle.meshlet_bounds)


@pytest.mark.gpu
@pytest.mark.parametrize("post_pass", [False, True])
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("scene", ["occluder", "kitten"])
def test_classic_frames_equal_the_oracle_chain(scene, fused, post_pass, iref):
    s = _occluder() if scene == "occluder" else _kitten_scene(128, 12.0, viewport=(256, 192))
    g = _gpu_frames(s, 3, fused, post_pass)
    o = RI.oracle_frames_classic(s, 3, post_pass=post_pass, iref=iref)
    for f, (gr, orc) in enumerate(zip(g, o)):
        assert gr["pyramid"].tobytes() == orc["pyramid"].tobytes(), f
        for ph in ["early", "late"] + (["post"] if post_pass else []):
            for k in ("count4", "commands", "dvb"):
                assert gr[ph][k].tobytes() == orc[ph][k].tobytes(), (f, ph, k)
            assert gr[ph]["depth"].view(np.uint32).tobytes() == orc[ph]["depth"].view(np.uint32).tobytes(), (f, ph, "depth")
    assert (o[-1]["late"]["depth"] > 0).any()
    if scene == "occluder":
        hidden, beside = set(s["hidden"]), set(s["beside"])
        for f in (2,):  # frame 0 draws everything late, frame 1 early still draws what frame 0 found visible
            drawn = set()
            for ph in ("early", "late"):
                drawn |= set(g[f][ph]["commands"]["drawId"].tolist())
            assert not (drawn & hidden) and beside <= drawn and 0 in drawn
            assert all(g[f]["late"]["dvb"][i] == 0 for i in hidden) and all(g[f]["late"]["dvb"][i] == 1 for i in beside)
