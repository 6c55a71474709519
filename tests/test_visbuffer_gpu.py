"""The frame-stable visibility buffer on the MI355X: nv_rasterdepth with NV_OPT_RASTER_VISIBILITY_ID 1 bit-identical to
tests/visbuffer_ref.c, frame(visibility=) and nv_visibility_resolve against the reference frame, the sharded composite against the
unsharded buffer, nv_visibility_merge against numpy, and the whole of it replayed from a captured graph."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import raster_clip_ref as RC
import raster_ref as RR
import test_raster_clip_gpu as TCG
import test_raster_gpu as TG
import test_sharded_frame_gpu as TSG
import visbuffer_ref as VB
from niagara_amd import layouts as L
from niagara_amd import shard, synth
from scenes import make_triangle_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2 ** 31 - 1
FRAMES = 2


@pytest.fixture(scope="session")
def vref(tmp_path_factory):
    return VB.load(tmp_path_factory.mktemp("visbuffer_ref_gpu"))


@pytest.fixture(scope="session")
def rref(tmp_path_factory):
    return RR.load(tmp_path_factory.mktemp("raster_ref_vis_gpu"))


@pytest.fixture(scope="session")
def clib(tmp_path_factory):
    return RC.load(tmp_path_factory.mktemp("raster_clip_ref_vis_gpu"))


@pytest.fixture(scope="module")
def ctx():
    from niagara_amd import pipeline as P
    c = P.Context()
    yield c
    c.close()


def _gpu(ctx, args, w, h, stable, near_clip, limit=None, depth=None, vis=None):
    """nv_rasterdepth with both options set for the call: (depth, visibility, totals); vis: the target to load"""
    import torch
    from niagara_amd import pipeline as P
    dev = ctx.device
    ctx.set_option(P.NV_OPT_RASTER_VISIBILITY_ID, stable)
    ctx.set_option(P.NV_OPT_RASTER_NEAR_CLIP, near_clip)
    if limit is not None:
        ctx.set_option(P.NV_OPT_RASTER_SMALL_LIMIT, limit)
    try:
        t = [P.to_device(a, dev) for a in args[1:]]
        d = torch.zeros((h, w), dtype=torch.float32, device=dev) if depth is None else torch.from_numpy(np.ascontiguousarray(depth)).to(dev)
        v = torch.zeros((h, w), dtype=torch.int64, device=dev) if vis is None else torch.from_numpy(np.ascontiguousarray(vis).view(np.int64)).to(dev)
        tot = torch.zeros(4, dtype=torch.int64, device=dev)
        ctx.rasterdepth(args[0], *t, d, w, h, v, tot)
        ctx.status()
        return d.cpu().numpy(), v.cpu().numpy().view(np.uint64), tot.cpu().numpy().view(np.uint64)
    finally:
        ctx.set_option(P.NV_OPT_RASTER_SMALL_LIMIT, 16)
        ctx.set_option(P.NV_OPT_RASTER_NEAR_CLIP, 0)
        ctx.set_option(P.NV_OPT_RASTER_VISIBILITY_ID, 0)


def _same(gpu, ref):
    assert gpu[2].tolist() == ref[2].tolist()
    assert gpu[0].view(np.uint32).tobytes() == ref[0].view(np.uint32).tobytes()
    assert gpu[1].tobytes() == ref[1].tobytes()


_REFS = {}


def _scene_refs(kind, case, pp, vref, rref, clib):
    """args, size, the stable reference with clip off / on and the slot-form references (computed once for the three limits)"""
    key = (kind, case, pp)
    if key not in _REFS:
        if kind == "outside":
            s = make_triangle_scene(seed=40 + case, n_draws=200, commands_per_draw=3, **TG.CAMERAS[case])
        else:
            s = make_triangle_scene(seed=140 + case, n_draws=24, commands_per_draw=2, **TCG.INSIDE[case])
        cib, cc4 = TG._cluster_list(s)
        w, h = s["viewport"]
        args = TG._args(s, cib, cc4, pp)
        stable = {c: vref.raster(*args, w, h, near_clip=c) for c in (0, 1)}
        slot = {0: rref.raster(*args, w, h, visibility=True), 1: clib.cluster(1).raster(*args, w, h, visibility=True)}
        _REFS[key] = (args, w, h, stable, slot)
    return _REFS[key]


# ---- 5. the rasteriser

@pytest.mark.gpu
@pytest.mark.parametrize("limit", [0, None, INT_MAX])  # None: the default, 16
@pytest.mark.parametrize("kind,case", [("outside", c) for c in range(len(TG.CAMERAS))] + [("inside", c) for c in range(len(TCG.INSIDE))])
def test_stable_raster_equals_reference(kind, case, limit, ctx, vref, rref, clib):
    """depth, words and totals equal the reference with the option on, clip off and on; the depth does not depend on the option; with the
    option off the words are the slot-form reference's"""
    for pp in (0, 1):
        args, w, h, stable, slot = _scene_refs(kind, case, pp, vref, rref, clib)
        for clip in (0, 1):
            on = _gpu(ctx, args, w, h, 1, clip, limit=limit)
            off = _gpu(ctx, args, w, h, 0, clip, limit=limit)
            _same(on, stable[clip])
            _same(off, slot[clip])
            assert on[0].tobytes() == off[0].tobytes() and on[2].tolist() == off[2].tolist()
            assert ((on[1] == 0) == (off[1] == 0)).all()
        assert w * h < 1000 or (stable[0][1] != 0).sum() > 0


@pytest.mark.gpu
def test_two_lists_into_one_target_and_depth_only_launch(ctx, vref):
    """the stable words of two disjoint lists rasterised one after the other into one target are the one-list target's (what frame() relies on);
    a launch without a visibility target writes the same depth and totals"""
    import torch
    from niagara_amd import pipeline as P
    s = make_triangle_scene(seed=41, n_draws=200, commands_per_draw=3, scene_radius=6.0, viewport=(333, 207))
    cib, cc4 = TG._cluster_list(s)
    w, h = s["viewport"]
    args = TG._args(s, cib, cc4)
    one = vref.raster(*args, w, h)
    ids = cib[:int(cc4[0])]
    pick = np.random.default_rng(2).random(len(ids)) < 0.5
    d = v = None
    tot = np.zeros(4, np.uint64)
    for part in (ids[pick], ids[~pick]):
        c4 = np.array([len(part), 0, 0, 0], np.uint32)
        cb = np.concatenate([part, np.zeros(512, np.uint32)])
        oracle.clustersubmit(c4, cb)
        d, v, t = _gpu(ctx, args[:6] + (cb, c4), w, h, 1, 0, depth=d, vis=v)
        tot += t
    _same((d, v, tot), one)
    ctx.set_option(P.NV_OPT_RASTER_VISIBILITY_ID, 1)
    try:
        t = [P.to_device(a, ctx.device) for a in args[1:]]
        dd = torch.zeros((h, w), dtype=torch.float32, device=ctx.device)
        tt = torch.zeros(4, dtype=torch.int64, device=ctx.device)
        ctx.rasterdepth(args[0], *t, dd, w, h, None, tt)
        ctx.status()
    finally:
        ctx.set_option(P.NV_OPT_RASTER_VISIBILITY_ID, 0)
    assert dd.cpu().numpy().tobytes() == one[0].tobytes() and tt.cpu().numpy().view(np.uint64).tolist() == one[2].tolist()


@pytest.mark.gpu
def test_cluster_past_the_id_range_and_option_values(ctx, vref):
    from niagara_amd import pipeline as P
    from niagara_amd._lib import NvError
    s = make_triangle_scene(seed=42, n_draws=20, commands_per_draw=1, scene_radius=6.0, viewport=(160, 120))
    cib, cc4 = TG._cluster_list(s)
    co = s["commands"].copy()
    co["meshletVisibilityOffset"][::2] = VB.MVI_END - 3
    args = (s["globals"], co, s["draws"], s["meshlets"], s["data"], s["vertices"], cib, cc4)
    ref = vref.raster(*args, 160, 120)
    assert 0 < (ref[1] != 0).sum() < (ref[0] > 0).sum()
    for limit in (0, None, INT_MAX):
        _same(_gpu(ctx, args, 160, 120, 1, 0, limit=limit), ref)
    for bad in (-1, 2, 34):
        with pytest.raises(NvError):
            ctx.set_option(P.NV_OPT_RASTER_VISIBILITY_ID, bad)


# ---- 6, 7. the frame and the resolve

def _scene(name):
    if name == "occluder":
        return synth.occluder_scene(meshlet_bounds=oracle.meshlet_bounds), 0
    return synth.interior_scene(meshlet_bounds=oracle.meshlet_bounds), 1


def _kw(s, near_clip):
    return dict(task_capacity=4096, cluster_capacity=4096 * 64, fused=True, vertices=s["vertices"], meshlet_data=s["data"], near_clip=bool(near_clip),
                stable_ids=True)


def _resolved(out):
    from niagara_amd import pipeline as P
    return dict(records=P.from_device(out["records"], L.VISRECORD).copy(), seen=out["meshlet_seen"].cpu().numpy().view(np.uint32).copy(),
                draw_pixels=out["draw_pixels"].cpu().numpy().view(np.uint32).copy(), totals=out["totals"].cpu().numpy().view(np.uint64).copy())


def _same_resolve(got, want, n_draws):
    if got["records"].tobytes() != want["records"].tobytes():  # say where before failing
        bad = np.nonzero(got["records"].reshape(-1) != want["records"].reshape(-1))[0]
        print("records differ at %d pixels; first:" % len(bad), [(int(i), tuple(got["records"].reshape(-1)[i]), tuple(want["records"].reshape(-1)[i])) for i in bad[:12]])
    assert got["totals"].tolist() == want["totals"].tolist()
    assert got["records"].tobytes() == want["records"].tobytes()
    assert got["seen"].tobytes() == want["seen"].tobytes()
    assert got["draw_pixels"][:n_draws].tolist() == want["draw_pixels"][:n_draws].tolist()


_FRAMES = {}


def _reference_frames(name, vref):
    if name not in _FRAMES:
        s, near_clip = _scene(name)
        frames = VB.oracle_frames(s, FRAMES, True, vref, near_clip)
        for rec in frames:
            rec["resolve"] = vref.resolve(s["cull"], rec["visibility"], rec["draws"], s["meshes"], len(rec["post"]["mvb"]))
        _FRAMES[name] = (s, near_clip, frames)
    return _FRAMES[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["occluder", "interior"])
def test_frame_visibility_and_resolve_equal_the_reference_frame(name, vref):
    from niagara_amd import pipeline as P
    s, near_clip, want = _reference_frames(name, vref)
    w, h = s["viewport"]
    pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], **_kw(s, near_clip))
    got = []
    try:
        vis = pipe.new_visibility()
        for f in range(FRAMES):
            pipe.frame(s["cull"], post_pass=True, visibility=vis)
            got.append((vis.cpu().numpy().view(np.uint64).copy(), pipe.depth.cpu().numpy().copy(), _resolved(pipe.resolve(s["cull"], vis))))
        pipe.ctx.status()
    finally:
        pipe.ctx.close()
    g = RR.globals_for(s["cull"], (w, h))
    for f in range(FRAMES):
        v, depth, res = got[f]
        assert v.tobytes() == want[f]["visibility"].tobytes(), f
        assert depth.view(np.uint32).tobytes() == want[f]["post"]["depth"].view(np.uint32).tobytes()
        _same_resolve(res, want[f]["resolve"], len(s["draws"]))
        covered = int((v != 0).sum())
        assert res["totals"].tolist() == [covered, 0, 0, 0] and covered > w * h // 20  # unresolved = 0 (a condition: checked on the CPU too)
        # every set bit of d_meshletSeen names a cluster of one of the frame's rasterised lists
        seen = {int(i) * 32 + b for i in np.nonzero(res["seen"])[0] for b in range(32) if res["seen"][i] >> b & 1}
        assert seen and seen <= VB.rasterised_clusters(want[f], True)
        # every record's triangle, rasterised alone on the CPU, covers its pixel at that depth
        r = res["records"].reshape(h, w)
        named = r["drawId"] != 0xFFFFFFFF
        assert (named == (v != 0)).all() and (r["depthBits"][named] == depth.view(np.uint32)[named]).all()
        keys = np.unique(r[named])
        for k in keys:
            z = vref.single_triangle(g, want[f]["draws"][k["drawId"]], s["meshlets"][k["meshletIndex"]], s["data"], s["vertices"], int(k["triangle"]), w, h,
                                     near_clip)
            at = named & (r["drawId"] == k["drawId"]) & (r["meshletIndex"] == k["meshletIndex"]) & (r["triangle"] == k["triangle"])
            assert (z[at] == r["depthBits"][at]).all() and (z[at] != 0).all() | (r["depthBits"][at] == 0).all(), k
        if name == "occluder":  # the wall's pixels resolve to the wall: at the wall's depth, and most of the covered screen
            wall = s["wall"] if isinstance(s["wall"], (list, tuple)) else [s["wall"]]
            is_wall = named & np.isin(r["drawId"], wall)
            assert is_wall.sum() > covered // 2
            assert set(r["drawId"][named].tolist()) & set(s["hidden"]) == set() or f == 0  # from frame 2 nothing behind the wall owns a pixel


@pytest.mark.gpu
def test_frame_visibility_needs_stable_ids_and_resolve_checks_arguments():
    import torch
    from niagara_amd import pipeline as P
    from niagara_amd._lib import NvError
    s, _ = _scene("occluder")
    kw = _kw(s, 0)
    kw["stable_ids"] = False
    pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], **kw)
    try:
        vis = pipe.new_visibility()
        with pytest.raises(NvError):
            pipe.frame(s["cull"], visibility=vis)
        with pytest.raises(NvError):
            pipe.resolve(s["cull"], vis)
        w, h = s["viewport"]
        c = pipe.ctx
        with pytest.raises(NvError):
            c.visibility_resolve(s["cull"], None, w, h, pipe.db, pipe.draw_count, pipe.mb, pipe.mesh_count)
        with pytest.raises(NvError):
            c.visibility_resolve(s["cull"], vis, 0, h, pipe.db, pipe.draw_count, pipe.mb, pipe.mesh_count)
        with pytest.raises(NvError):
            c.visibility_resolve(s["cull"], vis, w, 16385, pipe.db, pipe.draw_count, pipe.mb, pipe.mesh_count)
        with pytest.raises(NvError):
            c.visibility_resolve(s["cull"], vis, w, h, None, pipe.draw_count, pipe.mb, pipe.mesh_count)
        with pytest.raises(NvError):
            c.visibility_merge(vis, [vis], w, h)
        with pytest.raises(NvError):
            c.visibility_merge(vis, [], w, h)
        tot = torch.zeros(4, dtype=torch.int64, device=c.device)
        c.visibility_resolve(s["cull"], vis, w, h, pipe.db, pipe.draw_count, pipe.mb, pipe.mesh_count, totals4=tot)  # every output but one left out
        c.status()
        assert tot.tolist() == [0, 0, 0, 0]
    finally:
        pipe.ctx.close()


@pytest.mark.gpu
def test_resolve_marks_hand_made_words_unresolved(vref):
    """words no rasteriser wrote, and a scene with several LODs and draws without meshlets: records, counters and totals equal the reference"""
    import torch
    import test_visbuffer_cpu as TC
    from niagara_amd import pipeline as P
    s = TC._lod_scene()
    draws, meshes = s["draws"], s["meshes"]
    rng = np.random.default_rng(9)
    slots = int(draws["meshletVisibilityOffset"][-1])
    w, h = 97, 53  # an odd size: a ragged last wave
    mvi = rng.integers(0, slots + 40, w * h)
    mvi = np.repeat(mvi[::7], 7)[:w * h]  # runs of equal clusters, as a frame has them
    tri = rng.integers(0, 100, w * h)
    words = np.array([VB.encode(int(z), int(m), int(t)) for z, m, t in zip(rng.integers(0, 0x3F800001, w * h), mvi, tri)], np.uint64)
    words[rng.random(w * h) < 0.2] = 0
    words[5], words[6], words[7] = 9 << VB.SHIFT, VB.encode(3, VB.MVI_END - 1, 0), VB.encode(0x3F800000, 0, 0)
    ctx = P.Context()
    try:
        for lod in (1, 0):
            cd = s["cull"].copy()
            cd["lodEnabled"] = lod
            want = vref.resolve(cd, words, draws, meshes, TC._mvb_words(draws, meshes))
            dev = ctx.device
            out = dict(records=torch.zeros(w * h * 16, dtype=torch.uint8, device=dev), meshlet_seen=torch.zeros(len(want["seen"]), dtype=torch.int32, device=dev),
                       draw_pixels=torch.zeros(len(draws), dtype=torch.int32, device=dev), totals=torch.zeros(4, dtype=torch.int64, device=dev))
            ctx.visibility_resolve(cd, torch.from_numpy(words.view(np.int64)).to(dev), w, h, P.to_device(draws, dev), len(draws), P.to_device(meshes, dev),
                                   len(meshes), out["records"], out["meshlet_seen"], out["draw_pixels"], out["totals"])
            ctx.status()
            _same_resolve(_resolved(out), want, len(draws))
            assert 0 < want["totals"][1] < want["totals"][0]
    finally:
        ctx.close()


# ---- 8. sharded

@pytest.mark.gpu
@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("name", ["occluder", "interior"])
def test_local_shards_composite_to_the_unsharded_buffer(name, world, vref):
    from niagara_amd import pipeline as P
    s, near_clip, want = _reference_frames(name, vref)
    kw = _kw(s, near_clip)
    shards = P.ShardedVisibilityPipeline.local_shards(s["meshes"], s["meshlets"], s["draws"], s["viewport"], world, **kw)
    try:
        vis = shards.new_visibility()
        for f in range(FRAMES):
            own = []
            shards.frame(s["cull"], post_pass=True, visibility=vis, on_raster=lambda n: own.append([v.cpu().numpy().view(np.uint64).copy() for v in vis]))
            for k, p in enumerate(shards.pipes):
                assert vis[k].cpu().numpy().view(np.uint64).tobytes() == want[f]["visibility"].tobytes(), (f, k)
                if k in (0, world - 1):  # resolve on any rank == the unsharded resolve, with the scene's draw ids
                    _same_resolve(_resolved(p.resolve(s["cull"], vis[k])), want[f]["resolve"], len(s["draws"]))
            if world > 1 and f == 1:  # after frame 2's early raster, before any composite, the shards hold different buffers: the composite has work to do
                assert len({o.tobytes() for o in own[0]}) > 1 and all(o.tobytes() != want[f]["visibility"].tobytes() for o in own[0])
        shards.status()
    finally:
        shards.close()


@pytest.mark.gpu
def test_sharded_pipeline_takes_visibility_only_with_stable_ids():
    from niagara_amd import pipeline as P
    from niagara_amd._lib import NvError
    s, _ = _scene("occluder")
    kw = _kw(s, 0)
    kw["stable_ids"] = False
    shards = P.ShardedVisibilityPipeline.local_shards(s["meshes"], s["meshlets"], s["draws"], s["viewport"], 2, **kw)
    try:
        with pytest.raises(NvError):
            shards.frame(s["cull"], visibility=shards.new_visibility())
    finally:
        shards.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["gloo2", "nccl1"])
def test_process_per_rank_visibility_equals_the_unsharded_buffer(mode, tmp_path, vref):
    """two processes on one device over gloo (shard.composite_visibility's sign-flipped all_reduce(MAX) through the host), and one rank
    with the collective forced over RCCL on device memory.  More than one RCCL rank is not executed here (one device)."""
    s, near_clip, want = _reference_frames("occluder", vref)
    if mode == "gloo2":
        args, ranks = ["--gpus", "2", "--backend", "gloo", "--shared-device"], 2
    else:
        args, ranks = ["--gpus", "1", "--backend", "nccl", "--force-collective"], 1
    rec = TSG._run_tool(args + ["--frames", str(FRAMES), "--post", "--visibility", "--dump", str(tmp_path)], timeout=600)
    assert rec["visibility"] and rec["unresolved_pixels"] == 0 and rec["covered_pixels"] == int((want[-1]["visibility"] != 0).sum())
    for r in range(ranks):
        d = np.load(tmp_path / ("rank_%d.npz" % r))
        for f in range(FRAMES):
            assert d["f%d_visibility" % f].tobytes() == want[f]["visibility"].tobytes(), (r, f)
            assert d["f%d_records" % f].tobytes() == want[f]["resolve"]["records"].tobytes(), (r, f)


# ---- 9. the merge

@pytest.mark.gpu
@pytest.mark.parametrize("sources", [1, 2, 8, 11])
def test_visibility_merge_equals_numpy_maximum(ctx, sources):
    import torch
    rng = np.random.default_rng(sources)
    for w, h, skew in ((64, 48, 0), (61, 47, 0), (61, 47, 1), (1, 1, 0)):  # odd counts: the scalar tail; skew: 8-byte aligned only
        n = w * h
        bufs = rng.integers(0, 1 << 63, (sources + 1, n + 1), dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, (sources + 1, n + 1), dtype=np.uint64)
        bufs[:, ::5] = 0
        bufs[1 % (sources + 1), 3 % n] = np.uint64(VB.encode(0x3F800000, 7, 7))  # bit 63 set
        assert (bufs >> np.uint64(63)).any()
        t = [torch.from_numpy(b.view(np.int64)).to(ctx.device) for b in bufs]
        views = [x[skew:skew + n] for x in t]
        ctx.visibility_merge(views[0], views[1:], w, h)
        ctx.status()
        want = np.maximum.reduce([b[skew:skew + n] for b in bufs])
        assert views[0].cpu().numpy().view(np.uint64).tobytes() == want.tobytes()
        for k in range(1, sources + 1):  # the sources are left alone
            assert t[k].cpu().numpy().view(np.uint64).tobytes() == bufs[k].tobytes()


# ---- 10. capture

@pytest.mark.gpu
def test_frame_with_visibility_and_resolve_replays_from_a_graph(vref):
    import torch
    from niagara_amd import pipeline as P
    s, near_clip, want = _reference_frames("occluder", vref)
    pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], **_kw(s, near_clip))
    try:
        dev = pipe.ctx.device
        vis = pipe.new_visibility()
        w, h = s["viewport"]
        out = dict(records=torch.zeros(w * h * 16, dtype=torch.uint8, device=dev), meshlet_seen=torch.zeros_like(pipe.mvb),
                   draw_pixels=torch.zeros(len(s["draws"]), dtype=torch.int32, device=dev), totals=torch.zeros(4, dtype=torch.int64, device=dev))

        def step():
            pipe.frame(s["cull"], post_pass=True, visibility=vis)
            for t in (out["meshlet_seen"], out["draw_pixels"], out["totals"]):
                t.zero_()
            pipe.ctx.visibility_resolve(s["cull"], vis, w, h, pipe.db, pipe.draw_count, pipe.mb, pipe.mesh_count, out["records"], out["meshlet_seen"],
                                        out["draw_pixels"], out["totals"])
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            step()  # frame 1, eagerly: warm-up of every launch, and the state frame 2 starts from
            torch.cuda.synchronize()
            assert vis.cpu().numpy().view(np.uint64).tobytes() == want[0]["visibility"].tobytes()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=st):
                step()
            torch.cuda.synchronize()
            assert vis.cpu().numpy().view(np.uint64).tobytes() == want[0]["visibility"].tobytes()  # nothing ran during capture
            for _ in range(2):  # frame 2 and its steady-state repeat: the same bits
                out["records"].fill_(0x5A)
                vis.fill_(-1)
                graph.replay()
                torch.cuda.synchronize()
                assert vis.cpu().numpy().view(np.uint64).tobytes() == want[1]["visibility"].tobytes()
                _same_resolve(_resolved(out), want[1]["resolve"], len(s["draws"]))
        pipe.ctx.status()
    finally:
        pipe.ctx.close()
