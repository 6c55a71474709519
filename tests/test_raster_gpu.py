"""nv_rasterdepth on the MI355X: depth, visibility buffer and totals bit-identical to the CPU reference
(tests/raster_ref.c) on both raster paths, and the closed two-phase occlusion loop (VisibilityPipeline.frame) bit-identical to the
oracle chain with the reference raster, phase by phase."""
import numpy as np
import pytest

import oracle
import raster_ref as RR
from niagara_amd import layouts as L
from niagara_amd import synth
from scenes import make_scene, make_triangle_scene

INT_MAX = 2 ** 31 - 1
CAMERAS = [dict(), dict(cam_pos=(3.0, -2.0, 5.0), cam_quat=(0.0, 0.3826834, 0.0, 0.9238795)), dict(cam_pos=(0, 0, -8.0), viewport=(1920, 1080)),
           dict(scene_radius=3.0), dict(scene_radius=6.0, specials=True),  # tests/test_trianglecull.py's cases
           dict(viewport=(333, 207)), dict(viewport=(17, 9), scene_radius=6.0), dict(viewport=(1, 1), scene_radius=4.0)]


@pytest.fixture(scope="session")
def rref(tmp_path_factory):
    return RR.load(tmp_path_factory.mktemp("raster_ref_gpu"))


@pytest.fixture(scope="module")
def ctx():
    from niagara_amd import pipeline as P
    c = P.Context()
    yield c
    c.close()


def _cluster_list(s):
    cd = s["cull"].copy()
    cd["clusterBackfaceEnabled"], cd["cullingEnabled"] = 0, 1
    cib, cc4 = np.zeros(s["n"] * 64 + 256, np.uint32), np.zeros(4, np.uint32)
    oracle.clustercull(cd, 0, s["commands"], s["count4"], s["draws"], s["meshlets"], None, None, cib, cc4)
    oracle.clustersubmit(cc4, cib)
    return cib, cc4


def _args(s, cib, cc4, post_pass=0):
    g = s["globals"].copy()
    g["cullData"]["postPass"] = post_pass
    return (g, s["commands"], s["draws"], s["meshlets"], s["data"], s["vertices"], cib, cc4)


def _gpu(ctx, args, w, h, visibility=True, limit=None, depth=None):
    """nv_rasterdepth through Context.rasterdepth: (depth, visibility or None, totals)"""
    import torch
    from niagara_amd import pipeline as P
    dev = ctx.device
    if limit is not None:
        ctx.set_option(P.NV_OPT_RASTER_SMALL_LIMIT, limit)
    try:
        g = args[0]
        t = [P.to_device(a, dev) for a in args[1:]]
        d = torch.zeros((h, w), dtype=torch.float32, device=dev) if depth is None else torch.from_numpy(np.ascontiguousarray(depth)).to(dev)
        v = torch.zeros((h, w), dtype=torch.int64, device=dev) if visibility else None
        tot = torch.zeros(4, dtype=torch.int64, device=dev)
        ctx.rasterdepth(g, *t, d, w, h, v, tot)
        ctx.status()
        return (d.cpu().numpy(), None if v is None else v.cpu().numpy().view(np.uint64), tot.cpu().numpy().view(np.uint64))
    finally:
        ctx.set_option(P.NV_OPT_RASTER_SMALL_LIMIT, 16)


def _same(gpu, ref):
    dg, vg, tg = gpu
    dr, vr, tr = ref
    assert tg.tolist() == tr.tolist()
    assert dg.view(np.uint32).tobytes() == dr.view(np.uint32).tobytes()
    if vr is not None:
        assert vg.tobytes() == vr.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("limit", [None, 0, INT_MAX])
@pytest.mark.parametrize("case", range(len(CAMERAS)))
def test_hip_equals_reference(case, limit, ctx, rref):
    """depth, visibility and totals equal the reference with the default split and with each path pinned"""
    s = make_triangle_scene(seed=40 + case, n_draws=200, commands_per_draw=3, **CAMERAS[case])
    cib, cc4 = _cluster_list(s)
    w, h = s["viewport"]
    for pp in (0, 1):
        args = _args(s, cib, cc4, pp)
        ref = rref.raster(*args, w, h, visibility=True)
        _same(_gpu(ctx, args, w, h, limit=limit), ref)
        assert ref[2][0] > 0 and (w * h < 1000 or ref[2][3] > 0)


@pytest.mark.gpu
def test_hip_paths_agree_on_a_full_screen_plane(ctx, rref):
    """large triangles (wave path) and the same scene walked lane by lane write the same bits"""
    s = RR.mesh_scene(*_plane(), (1920, 1080), draws=_at(12.0))
    args = RR.raster_args(s)
    ref = rref.raster(*args, 1920, 1080, visibility=True)
    assert ref[2][3] == 1920 * 1080
    for limit in (None, 0, INT_MAX):
        _same(_gpu(ctx, args, 1920, 1080, limit=limit), ref)


def _plane():
    xs, ys = np.linspace(-20, 20, 13), np.linspace(-10, 10, 7)
    pos = [(x, y, 0.0) for y in ys for x in xs]
    tris = []
    for j in range(6):
        for i in range(12):
            a, b, c, d = j * 13 + i, j * 13 + i + 1, (j + 1) * 13 + i + 1, (j + 1) * 13 + i
            tris += [(a, b, c), (a, c, d)]
    return pos, tris


def _at(dist):
    d = np.zeros(1, dtype=L.MESHDRAW)
    d["position"], d["scale"], d["orientation"] = (0.0, 0.0, -dist), 1.0, (0, 0, 0, 1)
    return d


@pytest.mark.gpu
def test_hip_empty_and_padding_grids_leave_the_target_alone(ctx, rref):
    s = make_triangle_scene(seed=7, n_draws=20, commands_per_draw=1)
    w, h = s["viewport"]
    rng = np.random.default_rng(8)
    loaded = rng.uniform(0, 1, (h, w)).astype(np.float32)  # a late pass loads the target
    for cib, cc4 in ((np.zeros(256, np.uint32), np.array([0, 16, 0, 16], np.uint32)),
                     (np.full(512, 0xffffffff, np.uint32), np.array([0, 16, 2, 16], np.uint32))):
        d, _, tot = _gpu(ctx, _args(s, cib, cc4), w, h, visibility=False, depth=loaded)
        assert tot.tolist() == [0, 0, 0, 0] and d.tobytes() == loaded.tobytes()


@pytest.mark.gpu
def test_hip_long_list_several_chunks_per_wave(ctx, rref):
    """more than 64 slots per wave of the launch (6 workgroups x 4 waves per CU), with ~0 holes: several header chunks per wave"""
    s = make_triangle_scene(seed=91, n_draws=60, commands_per_draw=2, scene_radius=5.0, viewport=(160, 120))
    m = s["n"] * 64
    ids = (np.arange(m, dtype=np.uint32) // 64) | ((np.arange(m, dtype=np.uint32) % 64) << 24)
    ids = np.tile(ids, (6 * 4 * 256 * 64 * 2) // m + 1)
    ids[np.random.default_rng(92).random(len(ids)) < 0.01] = 0xffffffff
    cc4 = np.array([len(ids), 0, 0, 0], np.uint32)
    cib = np.concatenate([ids, np.zeros(512, np.uint32)])
    oracle.clustersubmit(cc4, cib)
    args = _args(s, cib, cc4)
    ref = rref.raster(*args, 160, 120, visibility=True)
    assert ref[2][0] > 6 * 4 * 256 * 64
    _same(_gpu(ctx, args, 160, 120), ref)


@pytest.mark.gpu
def test_hip_depth_only_equals_depth_with_visibility(ctx, rref):
    s = make_triangle_scene(seed=44, n_draws=200, commands_per_draw=3, scene_radius=6.0)
    cib, cc4 = _cluster_list(s)
    w, h = s["viewport"]
    a = _gpu(ctx, _args(s, cib, cc4), w, h, visibility=False)
    b = _gpu(ctx, _args(s, cib, cc4), w, h, visibility=True)
    assert a[0].tobytes() == b[0].tobytes() and a[2].tolist() == b[2].tolist()
    assert (b[1] >> 32).astype(np.uint32).tobytes() == b[0].view(np.uint32).tobytes()  # the visibility word carries the depth bits


@pytest.mark.gpu
def test_hip_argument_checks(ctx):
    import torch
    from niagara_amd import pipeline as P
    from niagara_amd._lib import NvError
    s = make_triangle_scene(seed=3, n_draws=4, commands_per_draw=1, viewport=(64, 48))
    cib, cc4 = _cluster_list(s)
    t = [P.to_device(a, ctx.device) for a in _args(s, cib, cc4)[1:]]
    d = torch.zeros((48, 64), dtype=torch.float32, device=ctx.device)
    for w, h in ((65, 48), (64, 47), (0, 48)):
        with pytest.raises(NvError):
            ctx.rasterdepth(s["globals"], *t, d, w, h)
    g = s["globals"].copy()
    g["screenWidth"], g["screenHeight"] = 16385, 48
    with pytest.raises(NvError):
        ctx.rasterdepth(g, *t, d, 16385, 48)
    with pytest.raises(NvError):
        ctx.rasterdepth(s["globals"], *t, None, 64, 48)
    ctx.rasterdepth(s["globals"], *t, d, 64, 48)
    ctx.status()


# ---- the closed loop

def _make_scene_with_geometry():
    sc = make_scene(seed=5, n_draws=300, viewport=(256, 192))
    data, vertices = synth.make_geometry(sc["meshlets"], seed=6)
    cd = sc["cull"].copy()
    cd["occlusionEnabled"], cd["clusterOcclusionEnabled"], cd["clusterBackfaceEnabled"] = 1, 1, 1
    return dict(meshes=sc["meshes"], meshlets=sc["meshlets"], draws=sc["draws"], data=data, vertices=vertices, cull=cd, viewport=sc["viewport"])


def _occluder():
    return synth.occluder_scene(meshlet_bounds=oracle.meshlet_bounds)


def _pipeline(s, fused):
    from niagara_amd import pipeline as P
    return P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], task_capacity=4096, cluster_capacity=4096 * 64, fused=fused,
                                meshlet_data=s["data"], vertices=s["vertices"])


def _gpu_frames(s, frames, fused, post_pass):
    from niagara_amd import pipeline as P
    pipe = _pipeline(s, fused)
    out = []
    try:
        for _ in range(frames):
            rec = {}

            def grab(name):
                c4 = pipe.dccb.cpu().numpy().view(np.uint32).copy()
                cc4 = pipe.ccb.cpu().numpy().view(np.uint32).copy()
                ncmd, nv = int(c4[1]) * 64, int(cc4[2]) * 256
                rec[name] = dict(count4=c4, commands=P.from_device(pipe.dcb, L.TASKCMD)[:ncmd].copy(), cc4=cc4,
                                 cib=pipe.cib.cpu().numpy().view(np.uint32)[:nv].copy(), dvb=pipe.dvb.cpu().numpy().view(np.uint32).copy(),
                                 mvb=pipe.mvb.cpu().numpy().view(np.uint32).copy(), depth=pipe.depth.cpu().numpy().copy())
            pipe.frame(s["cull"], post_pass=post_pass, on_phase=grab)
            rec["pyramid"] = pipe.pyramid.data.cpu().numpy().copy()
            out.append(rec)
        pipe.ctx.status()
    finally:
        pipe.ctx.close()
    return out


def _compare_frames(g, o, phases):
    for f, (gr, orc) in enumerate(zip(g, o)):
        assert gr["pyramid"].tobytes() == orc["pyramid"].tobytes(), f
        for ph in phases:
            for k in ("count4", "commands", "cc4", "cib", "dvb", "mvb"):
                assert gr[ph][k].tobytes() == orc[ph][k].tobytes(), (f, ph, k)
            assert gr[ph]["depth"].view(np.uint32).tobytes() == orc[ph]["depth"].view(np.uint32).tobytes(), (f, ph, "depth")


@pytest.mark.gpu
@pytest.mark.parametrize("post_pass", [False, True])
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("scene", ["occluder", "make_scene"])
def test_frames_equal_the_oracle_chain(scene, fused, post_pass, rref):
    s = _occluder() if scene == "occluder" else _make_scene_with_geometry()
    g = _gpu_frames(s, 3, fused, post_pass)
    o = RR.oracle_frames(s, 3, post_pass=post_pass, rref=rref)
    _compare_frames(g, o, ["early", "late"] + (["post"] if post_pass else []))
    assert (o[-1]["late"]["depth"] > 0).any()


@pytest.mark.gpu
def test_occlusion_actually_happens(rref):
    """From frame 2 the boxes behind the wall are neither drawn nor in any list; the boxes beside it are drawn; the final depth is the
    reference raster of exactly what the two passes drew"""
    s = _occluder()
    g = _gpu_frames(s, 4, fused=True, post_pass=False)
    hidden, beside = set(s["hidden"]), set(s["beside"])
    w, h = s["viewport"]
    slots, _ = oracle.assign_visibility_offsets(s["draws"].copy(), s["meshes"])
    for f in (2, 3):
        drawn = set()
        for ph in ("early", "late"):
            r = g[f][ph]
            ids = r["cib"][:int(r["cc4"][0])]
            ids = ids[ids != 0xffffffff]
            drawn |= set(r["commands"][ids & 0xffffff]["drawId"].tolist())
        assert not (drawn & hidden) and beside <= drawn and 0 in drawn
        assert all(g[f]["late"]["dvb"][i] == 0 for i in hidden) and all(g[f]["late"]["dvb"][i] == 1 for i in beside)
    # the final depth of the last frame = the reference raster of its early list, then its late list
    draws = s["draws"].copy()
    oracle.assign_visibility_offsets(draws, s["meshes"])
    depth = None
    for ph in ("early", "late"):
        r = g[-1][ph]
        gl = RR.globals_for(s["cull"], (w, h))
        depth, _, _ = rref.raster(gl, r["commands"], draws, s["meshlets"], s["data"], s["vertices"], r["cib"], r["cc4"], w, h, depth=depth)
    assert depth.view(np.uint32).tobytes() == g[-1]["late"]["depth"].view(np.uint32).tobytes()
    assert (depth > 0).sum() > w * h // 3
