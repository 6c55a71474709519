"""Near-plane clipping on the MI355X (NV_OPT_RASTER_NEAR_CLIP): nv_rasterdepth and nv_rasterdepth_indexed with the option on
equal the clip reference (tests/raster_clip_ref.c) bit for bit on both raster paths; switched off again they equal the unclipped
references; the closed loop on synth.interior_scene equals the oracle chain with the clip reference and culls what the clipped surfaces
hide."""
import numpy as np
import pytest

import oracle
import raster_clip_ref as RC
import raster_indexed_ref as RI
import raster_ref as RR
import test_raster_clip_cpu as TC
import test_raster_gpu as TG
from niagara_amd import layouts as L
from niagara_amd import synth
from scenes import make_triangle_scene

INT_MAX = 2 ** 31 - 1
# test_raster_gpu.py's scenes with the camera moved into the triangle cloud
INSIDE = [dict(scene_radius=0.5), dict(scene_radius=0.8, cam_quat=(0.0, 0.3826834, 0.0, 0.9238795)), dict(scene_radius=0.5, viewport=(1920, 1080)),
          dict(scene_radius=1.0, specials=True), dict(scene_radius=0.5, viewport=(333, 207)), dict(scene_radius=0.5, viewport=(17, 9)),
          dict(scene_radius=0.5, viewport=(1, 1))]


@pytest.fixture(scope="session")
def rref(tmp_path_factory):
    return RR.load(tmp_path_factory.mktemp("raster_ref_clip_gpu"))


@pytest.fixture(scope="session")
def iref(tmp_path_factory):
    return RI.load(tmp_path_factory.mktemp("raster_indexed_ref_clip_gpu"))


@pytest.fixture(scope="session")
def clib(tmp_path_factory):
    return RC.load(tmp_path_factory.mktemp("raster_clip_ref_gpu"))


@pytest.fixture(scope="module")
def ctx():
    from niagara_amd import pipeline as P
    c = P.Context()
    yield c
    c.close()


def _gpu(ctx, args, w, h, near_clip=1, limit=None, depth=None):
    from niagara_amd import pipeline as P
    ctx.set_option(P.NV_OPT_RASTER_NEAR_CLIP, near_clip)
    try:
        return TG._gpu(ctx, args, w, h, limit=limit, depth=depth)
    finally:
        ctx.set_option(P.NV_OPT_RASTER_NEAR_CLIP, 0)


def _gpu_indexed(ctx, ix, g, w, h, near_clip=1, limit=None, depth=None):
    """nv_rasterdepth_indexed through Context.rasterdepth_indexed: (depth, totals)"""
    import torch
    from niagara_amd import pipeline as P
    dev = ctx.device
    ctx.set_option(P.NV_OPT_RASTER_NEAR_CLIP, near_clip)
    if limit is not None:
        ctx.set_option(P.NV_OPT_RASTER_SMALL_LIMIT, limit)
    try:
        cmds = np.ascontiguousarray(ix["commands"], L.DRAWCMD)
        ind = np.ascontiguousarray(ix["indices"], np.uint32)
        dcb, db, ib, vb = P.to_device(cmds, dev), P.to_device(ix["draws"], dev), P.to_device(ind, dev), P.to_device(ix["vertices"], dev)
        dccb = P.to_device(np.array([int(ix["count"]), 0, 0, 0], np.uint32), dev)
        d = torch.zeros((h, w), dtype=torch.float32, device=dev) if depth is None else torch.from_numpy(np.ascontiguousarray(depth)).to(dev)
        tot = torch.zeros(4, dtype=torch.int64, device=dev)
        ctx.reserve(len(ix["draws"]))
        ctx.rasterdepth_indexed(g, dcb, dccb, db, len(ix["draws"]), ib, len(ind), vb, len(ix["vertices"]), d, w, h, tot)
        ctx.status()
        return d.cpu().numpy(), tot.cpu().numpy().view(np.uint64)
    finally:
        ctx.set_option(P.NV_OPT_RASTER_SMALL_LIMIT, 16)
        ctx.set_option(P.NV_OPT_RASTER_NEAR_CLIP, 0)


def _same_indexed(gpu, ref):
    assert gpu[1].tolist() == ref[1].tolist()
    assert gpu[0].view(np.uint32).tobytes() == ref[0].view(np.uint32).tobytes()


_CLOUD = {}


def _cloud(case, pp, clib):
    """the scene of `case` with its two references (computed once for the three limits: the camera inside the cloud overdraws heavily)"""
    if (case, pp) not in _CLOUD:
        s = make_triangle_scene(seed=140 + case, n_draws=24, commands_per_draw=2, **INSIDE[case])
        cib, cc4 = TG._cluster_list(s)
        w, h = s["viewport"]
        ix = RI.from_cluster_scene(s)
        args = TG._args(s, cib, cc4, pp)
        cref = clib.cluster(1)
        ref = cref.raster(*args, w, h, visibility=True)
        assert cref.stats[RC.CLIPPED] >= 300, cref.stats  # at least a few hundred triangles are clipped
        iref_ = clib.indexed(1).raster(args[0], ix["commands"], ix["count"], ix["draws"], ix["indices"], ix["vertices"], w, h)
        _CLOUD[(case, pp)] = (args, ix, w, h, ref, iref_)
    return _CLOUD[(case, pp)]


@pytest.mark.gpu
@pytest.mark.parametrize("limit", [None, 0, INT_MAX])
@pytest.mark.parametrize("case", range(len(INSIDE)))
def test_hip_equals_clip_reference_inside_the_cloud(case, limit, ctx, clib):
    """both entry points, both faces: depth, visibility and totals equal the clip reference with the default split and each path pinned"""
    for pp in (0, 1):
        args, ix, w, h, ref, iref_ = _cloud(case, pp, clib)
        TG._same(_gpu(ctx, args, w, h, limit=limit), ref)
        _same_indexed(_gpu_indexed(ctx, ix, args[0], w, h, limit=limit), iref_)


@pytest.mark.gpu
@pytest.mark.parametrize("limit", [None, 0, INT_MAX])
def test_hip_ground_plane_at_1080p(limit, ctx, clib):
    """large pieces: the wave path and its queue, through both entry points"""
    s, tris = TC.ground_plane((1920, 1080))
    args = RR.raster_args(s)
    cref = clib.cluster(1)
    ref = cref.raster(*args, 1920, 1080, visibility=True)
    assert cref.stats[RC.CLIPPED] >= 12 and ref[2][3] > 1920 * 1080 // 3
    TG._same(_gpu(ctx, args, 1920, 1080, limit=limit), ref)
    ix = RI.from_mesh_scene(s, tris)
    iref_ = clib.indexed(1).raster(ix["g"], ix["commands"], ix["count"], ix["draws"], ix["indices"], ix["vertices"], 1920, 1080)
    assert iref_[0].tobytes() == ref[0].tobytes()
    _same_indexed(_gpu_indexed(ctx, ix, ix["g"], 1920, 1080, limit=limit), iref_)


@pytest.mark.gpu
def test_hip_late_pass_onto_a_loaded_target(ctx, clib):
    s = make_triangle_scene(seed=151, n_draws=24, commands_per_draw=2, scene_radius=0.5)
    cib, cc4 = TG._cluster_list(s)
    w, h = s["viewport"]
    loaded = np.random.default_rng(152).uniform(0, 1, (h, w)).astype(np.float32)
    args = TG._args(s, cib, cc4)
    ref = clib.cluster(1).raster(*args, w, h, depth=loaded, visibility=True)
    TG._same(_gpu(ctx, args, w, h, depth=loaded), ref)
    assert (ref[0] != loaded).any() and (ref[0] == loaded).any()
    ix = RI.from_cluster_scene(s)
    iref_ = clib.indexed(1).raster(args[0], ix["commands"], ix["count"], ix["draws"], ix["indices"], ix["vertices"], w, h, depth=loaded)
    _same_indexed(_gpu_indexed(ctx, ix, args[0], w, h, depth=loaded), iref_)


@pytest.mark.gpu
def test_hip_long_list_several_chunks_per_wave(ctx, clib):
    """test_raster_gpu's long list (more than 64 slots per wave, ~0 holes) with the camera inside the cloud"""
    s = make_triangle_scene(seed=191, n_draws=60, commands_per_draw=2, scene_radius=0.5, viewport=(64, 48))
    m = s["n"] * 64
    ids = (np.arange(m, dtype=np.uint32) // 64) | ((np.arange(m, dtype=np.uint32) % 64) << 24)
    ids = np.tile(ids, (6 * 4 * 256 * 64 * 2) // m + 1)
    ids[np.random.default_rng(192).random(len(ids)) < 0.01] = 0xffffffff
    cc4 = np.array([len(ids), 0, 0, 0], np.uint32)
    cib = np.concatenate([ids, np.zeros(512, np.uint32)])
    oracle.clustersubmit(cc4, cib)
    args = TG._args(s, cib, cc4)
    cref = clib.cluster(1)
    ref = cref.raster(*args, 64, 48, visibility=True)
    assert ref[2][0] > 6 * 4 * 256 * 64 and cref.stats[RC.CLIPPED] >= 300
    TG._same(_gpu(ctx, args, 64, 48), ref)


@pytest.mark.gpu
def test_hip_option_switched_off_again_matches_the_unclipped_references(ctx, rref, iref, clib):
    s = make_triangle_scene(seed=141, n_draws=24, commands_per_draw=2, scene_radius=0.5)
    cib, cc4 = TG._cluster_list(s)
    w, h = s["viewport"]
    args = TG._args(s, cib, cc4)
    ix = RI.from_cluster_scene(s)
    ia = (args[0], ix["commands"], ix["count"], ix["draws"], ix["indices"], ix["vertices"], w, h)
    on = clib.cluster(1).raster(*args, w, h, visibility=True)
    off = rref.raster(*args, w, h, visibility=True)
    assert on[0].tobytes() != off[0].tobytes()
    TG._same(_gpu(ctx, args, w, h, near_clip=1), on)
    TG._same(_gpu(ctx, args, w, h, near_clip=0), off)
    _same_indexed(_gpu_indexed(ctx, ix, args[0], w, h, near_clip=1), clib.indexed(1).raster(*ia))
    _same_indexed(_gpu_indexed(ctx, ix, args[0], w, h, near_clip=0), iref.raster(*ia))


@pytest.mark.gpu
def test_hip_option_values_other_than_0_and_1_raise(ctx):
    from niagara_amd import pipeline as P
    from niagara_amd._lib import NvError
    for v in (2, -1, INT_MAX):
        with pytest.raises(NvError):
            ctx.set_option(P.NV_OPT_RASTER_NEAR_CLIP, v)
    ctx.set_option(P.NV_OPT_RASTER_NEAR_CLIP, 1)
    ctx.set_option(P.NV_OPT_RASTER_NEAR_CLIP, 0)


# ---- the closed loop

def _interior():
    return synth.interior_scene_indexed(meshlet_bounds=oracle.meshlet_bounds)


def _gpu_frames(s, frames, fused, post_pass, task, near_clip):
    from niagara_amd import pipeline as P
    pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], task_capacity=4096, cluster_capacity=4096 * 64, fused=fused,
                                meshlet_data=s["data"], vertices=s["vertices"], indices=s["indices"], near_clip=near_clip)
    out = []
    try:
        for _ in range(frames):
            rec = {}

            def grab(name):
                c4 = pipe.dccb.cpu().numpy().view(np.uint32).copy()
                r = dict(count4=c4, dvb=pipe.dvb.cpu().numpy().view(np.uint32).copy(), depth=pipe.depth.cpu().numpy().copy())
                if task:
                    cc4 = pipe.ccb.cpu().numpy().view(np.uint32).copy()
                    ncmd, nv = int(c4[1]) * 64, int(cc4[2]) * 256
                    r.update(commands=P.from_device(pipe.dcb, L.TASKCMD)[:ncmd].copy(), cc4=cc4, cib=pipe.cib.cpu().numpy().view(np.uint32)[:nv].copy(),
                             mvb=pipe.mvb.cpu().numpy().view(np.uint32).copy())
                else:
                    r.update(commands=P.from_device(pipe.dcb, L.DRAWCMD)[:int(c4[0])].copy())
                rec[name] = r
            pipe.frame(s["cull"], post_pass=post_pass, on_phase=grab, task=task)
            rec["pyramid"] = pipe.pyramid.data.cpu().numpy().copy()
            out.append(rec)
        pipe.ctx.status()
    finally:
        pipe.ctx.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("task", [True, False])
@pytest.mark.parametrize("post_pass", [False, True])
@pytest.mark.parametrize("fused", [False, True])
def test_interior_frames_equal_the_oracle_chain(fused, post_pass, task, clib):
    s = _interior()
    g = _gpu_frames(s, 3, fused, post_pass, task, near_clip=True)
    if task:
        o = RR.oracle_frames(s, 3, post_pass=post_pass, rref=clib.cluster(1))
        keys = ("count4", "commands", "cc4", "cib", "dvb", "mvb")
    else:
        o = RI.oracle_frames_classic(s, 3, post_pass=post_pass, iref=clib.indexed(1))
        keys = ("count4", "commands", "dvb")
    for f, (gr, orc) in enumerate(zip(g, o)):
        assert gr["pyramid"].tobytes() == orc["pyramid"].tobytes(), f
        for ph in ["early", "late"] + (["post"] if post_pass else []):
            for k in keys:
                assert gr[ph][k].tobytes() == orc[ph][k].tobytes(), (f, ph, k)
            assert gr[ph]["depth"].view(np.uint32).tobytes() == orc[ph]["depth"].view(np.uint32).tobytes(), (f, ph, "depth")
    assert (o[-1]["late"]["depth"] > 0).mean() > 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("task", [True, False])
def test_interior_occlusion_needs_the_clipped_surfaces(task):
    """from frame 2 on no box under the floor or behind the wall is in any list and their dvb words are 0 with near_clip=True; with
    near_clip=False the same boxes are drawn; the boxes in the open are drawn either way"""
    s = _interior()
    hidden, open_ = set(s["hidden"]), set(s["open"])
    for near_clip in (True, False):
        g = _gpu_frames(s, 4, fused=True, post_pass=False, task=task, near_clip=near_clip)
        for f in (2, 3):
            drawn = set()
            for ph in ("early", "late"):
                r = g[f][ph]
                if task:
                    ids = r["cib"][:int(r["cc4"][0])]
                    ids = ids[ids != 0xffffffff]
                    drawn |= set(r["commands"][ids & 0xffffff]["drawId"].tolist())
                else:
                    drawn |= set(r["commands"]["drawId"].tolist())
            dvb = g[f]["late"]["dvb"]
            assert open_ <= drawn and all(dvb[i] == 1 for i in open_) and set(s["surfaces"]) <= drawn
            if near_clip:
                assert not (drawn & hidden) and all(dvb[i] == 0 for i in hidden)
            else:
                assert hidden <= drawn and all(dvb[i] == 1 for i in hidden)
