"""nv_animate_draws on the MI355X.  The device against its host twin (the same text, niagara_amd/csrc/animmath.h): every byte
of the draw and light buffers equal except the orientations of slerp's trigonometric branch, which are held to the counted bound of the fp64
build of tests/animate_ref.c; the fused cull mirror, the rebuilt TLAS, the traced mask and the pipeline's frame against the CPU references run on
the DOWNLOADED records, none with a tolerance; the captured chain; the refusals."""
import numpy as np
import pytest

import animate_ref as AR
import oracle
import raster_ref as RR
import shadow_ref as SH
import test_drawcull_mesh_table as TM
import test_shade_gpu as TS
import test_shadowtrace_gpu as TG
from niagara_amd import host, synth
from niagara_amd import layouts as L
from niagara_amd._lib import NvError

import passes
from scenes import task_capacity

DRAWS = 3000
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1000]  # partial waves, whole workgroups (256 lanes) and one lane more
TIMES = (0.7, 12.5, 1e9)
POISON = TS.POISON
# chosen on the CPU (the oracle's frames of synth.occluder_scene_indexed and tests/shadow_ref.c, host twin's records): with this seed the traced mask
# of the animated scene at ANIM_TIME differs from the unanimated one in 19082 of 320 x 192 texels
ANIM_SEED, ANIM_TIME = 3, 0.6


@pytest.fixture(scope="module")
def aref(tmp_path_factory):
    return AR.load(tmp_path_factory.mktemp("animate_ref_gpu"))


@pytest.fixture(scope="module")
def shref(tmp_path_factory):
    return SH.load(tmp_path_factory.mktemp("shadow_ref_anim_gpu"))


@pytest.fixture(scope="module")
def rref(tmp_path_factory):
    return RR.load(tmp_path_factory.mktemp("raster_ref_anim_gpu"))


@pytest.fixture(scope="module")
def ctx():
    from niagara_amd import pipeline as P
    c = P.Context()
    yield c
    c.close()


def _random_records(n, dtype, seed):
    return np.random.default_rng(seed).integers(0, 256, n * dtype.itemsize, dtype=np.uint8).view(dtype)


def _compare(name, aref, a, k, time, got, want, draws0):
    """the device's draw records against the host twin's: bytes equal outside the trigonometric branch's orientations, those within the bound
    of the fp64 restatement; returns the largest error seen there"""
    n = len(a)
    r32 = aref.eval(a, k, np.arange(n, dtype=np.uint32), np.full(n, time), "f32")
    r64 = aref.eval(a, k, np.arange(n, dtype=np.uint32), np.full(n, time), "f64")
    trig = np.zeros(len(got), bool)
    live = ~r32["skipped"]
    trig[a["drawIndex"][live & ((r32["flags"] & AR.TRIG) != 0)]] = True
    gw, ww = got.view(np.uint32).reshape(-1, 12), want.view(np.uint32).reshape(-1, 12)
    assert (gw[~trig] == ww[~trig]).all(), name
    assert (gw[trig][:, :4] == ww[trig][:, :4]).all() and (gw[trig][:, 8:] == ww[trig][:, 8:]).all(), name
    touched = np.zeros(len(got), bool)
    touched[a["drawIndex"][live]] = True
    assert got[~touched].tobytes() == draws0[~touched].tobytes(), name  # not targeted, or skipped: untouched
    sel = live & ((r32["flags"] & AR.TRIG) != 0)
    err = np.abs(got["orientation"][a["drawIndex"][sel]].astype(np.float64) - r64["out"][sel, 4:]) if sel.any() else np.zeros(1)
    same = int((gw[trig][:, 4:8] == ww[trig][:, 4:8]).sum())
    print("%s: %d animations, %d skipped, %d trigonometric: largest |device - fp64| = %.3g (%.2f x 2^-23, bound %.3g), %d of %d words equal the host twin's"
          % (name, n, int(r32["skipped"].sum()), int(sel.sum()), err.max(), err.max() * 2 ** 23, AR.TRIG_BOUND, same, 4 * int(trig.sum())))
    assert err.max() <= AR.TRIG_BOUND, name
    return err.max()


@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
def test_device_equals_the_host_twin(count, ctx, aref):
    draws0 = _random_records(DRAWS, L.MESHDRAW, 40 + count)
    a, k = AR.fuzz_table(count, DRAWS, seed=50 + count)
    ctx.upload_draws(None, 0)
    ctx.upload_animations(a, k, DRAWS)
    for time in TIMES:
        db = TS._dev(ctx, draws0, 64)
        ctx.animate_draws(time, db, DRAWS)
        ctx.status()
        got = TS._host(db, draws0.nbytes, L.MESHDRAW, (DRAWS,))
        want = draws0.copy()
        host.animate_draws_host(time, a, k, want)
        _compare("count %d time %g" % (count, time), aref, a, k, time, got, want, draws0)
        if count >= 63:
            assert got.tobytes() != draws0.tobytes()


@pytest.mark.gpu
def test_lights(ctx, aref):
    count, nl = 257, 40
    draws0, lights0 = _random_records(DRAWS, L.MESHDRAW, 7), _random_records(nl, L.LIGHT, 8)
    a, k = AR.fuzz_table(count, DRAWS, seed=9, light_count=nl)
    a["drawIndex"][:nl:2] = -1  # lights alone, and lights with a draw
    ctx.upload_draws(None, 0)
    ctx.upload_animations(a, k, DRAWS, nl)
    for time in TIMES:
        db, lb = TS._dev(ctx, draws0, 64), TS._dev(ctx, lights0, 64)
        ctx.animate_draws(time, db, DRAWS, lb, nl)
        ctx.status()
        want_d, want_l = draws0.copy(), lights0.copy()
        host.animate_draws_host(time, a, k, want_d, want_l)
        got_l = TS._host(lb, lights0.nbytes, L.LIGHT, (nl,))
        assert got_l.tobytes() == want_l.tobytes()  # positions bit for bit, range / colour / intensity untouched
        assert all(got_l[f].tobytes() == lights0[f].tobytes() for f in ("range", "color", "intensity"))
        assert (got_l["position"].view(np.uint32) != lights0["position"].view(np.uint32)).any()
        keep = a["drawIndex"] >= 0
        _compare("lights, time %g" % time, aref, a[keep], k, time, TS._host(db, draws0.nbytes, L.MESHDRAW, (DRAWS,)), want_d, draws0)
        # d_lights == NULL: accepted, the draws as before, no light written
        db2 = TS._dev(ctx, draws0, 64)
        ctx.animate_draws(time, db2, DRAWS)
        ctx.status()
        assert TS._host(db2, draws0.nbytes, L.MESHDRAW, (DRAWS,)).tobytes() == TS._host(db, draws0.nbytes, L.MESHDRAW, (DRAWS,)).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("state", ["both", "draws_first", "none"])
def test_drawcull_behind_the_animation_equals_the_oracle_on_the_downloaded_records(state, ctx):
    """the fused mirror (registered draws) and the records in place (nothing registered): early and late drawcull bit-identical to the oracle
    on the device's records, and to the same pass after a full nv_update_draws"""
    from niagara_amd import pipeline as P
    c = TM.case(65)
    scene, meshes = c.scene, c.scene["meshes"]
    which = np.arange(1, c.n, 3)
    a, k = synth.orbit_animations(scene["draws"], which, 5, seed=12, orbit=4.0)
    cd = passes.set_flags(scene["cull"], TM.ALL_ON)
    try:
        d = TM.Device(ctx, scene)
        d.register(state)
        ctx.upload_animations(a, k, c.n)
        ctx.animate_draws(1.3, d.db, c.n)
        ctx.status()
        moved = P.from_device(d.db, L.MESHDRAW, c.n).copy()
        assert (moved[which]["position"] != scene["draws"][which]["position"]).any(axis=1).all()
        rest = np.setdiff1d(np.arange(c.n), which)
        assert moved[rest].tobytes() == scene["draws"][rest].tobytes()
        cap = task_capacity(dict(meshes=meshes, draws=moved))
        for late, dvb0 in TM.early_and_late(c):
            for task in (1, 0):
                want = TM.oracle_pass(meshes, moved, cd, late, task, dvb0, c.pyr)
                stale = TM.oracle_pass(meshes, scene["draws"], cd, late, task, dvb0, c.pyr)
                assert TM.difference(stale, want, moved) is not None  # the animation changes this pass
                got = d.run(cd, late, task, dvb0, cap if task else c.n + 1)
                diff = TM.difference(got, want, moved)
                assert diff is None, ((state, late, task), diff)
        ctx.update_draws(d.db, 0, c.n)  # the unfused pair's second half: the same mirror, the same passes
        for late, dvb0 in TM.early_and_late(c):
            got = d.run(cd, late, 1, dvb0, cap)
            diff = TM.difference(got, TM.oracle_pass(meshes, moved, cd, late, 1, dvb0, c.pyr), moved)
            assert diff is None, ((state, late, "after update_draws"), diff)
        ctx.status()
    finally:
        ctx.upload_animations(None, None, 0)
        TM.drop(ctx)


@pytest.mark.gpu
def test_tlas_and_mask_behind_the_animation(shref):
    """animate -> rt_tlas_build -> shadow_trace: the blob equals the host rebuild on the downloaded draws byte for byte, the mask equals the
    brute-force restatement on them; then the same chain captured once and replayed equals the eager bytes"""
    import torch
    from niagara_amd import pipeline as P
    scene = SH.fuzz_scene(instances=20, seed=11, radius=TG.RADIUS)
    n = len(scene["draws"])
    blob = host.rt_scene_build(scene["meshes"], scene["indices"], scene["vertices"], scene["draws"])
    a, k = synth.orbit_animations(scene["draws"], np.arange(n), 6, seed=5, orbit=1.5)
    w, h = 67, 37
    sd, depth_host = TG._inputs(w, h, 1e-2, 0)
    poison = np.full((h, w), TG.POISON, np.uint8)
    static = shref.shadow_trace(sd, scene, depth_host, poison, 1)
    c = P.Context()
    try:
        c.rt_scene_upload(blob)
        c.rt_scene_reserve_dynamic(n)
        c.upload_animations(a, k, n)
        db = P.to_device(scene["draws"], c.device)
        depth, shadow = TS._dev(c, depth_host), TS._out(c, w * h)
        eager = {}
        for time in (0.4, 2.2):
            c.animate_draws(time, db, n)
            c.rt_tlas_build(db, n)
            shadow.fill_(TG.POISON)
            c.shadow_trace(sd, depth, shadow, w, h, 1)
            c.status()
            moved = P.from_device(db, L.MESHDRAW, n).copy()
            assert c.rt_scene_download().tobytes() == host.rt_tlas_build_host(blob, moved).tobytes()
            want = shref.shadow_trace(sd, dict(scene, draws=moved), depth_host, poison, 1)
            got = TS._host(shadow, w * h, np.uint8, (h, w)).copy()
            TG._report("animated to %g" % time, got, want)
            print("animated and static masks differ in %d texels" % int((want != static).sum()))
            assert (want != static).sum() >= 50
            eager[time] = (moved.tobytes(), got.tobytes())
        # the captured chain: linear (animate -> tlas build -> trace); the time is a launch argument, so a replay repeats it
        db.copy_(P.to_device(scene["draws"], c.device))
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=st):
                c.animate_draws(2.2, db, n)
                c.rt_tlas_build(db, n)
                c.shadow_trace(sd, depth, shadow, w, h, 1)
            torch.cuda.synchronize()
            for _ in range(2):
                db.copy_(P.to_device(scene["draws"], c.device))  # outside the graph
                shadow.fill_(TG.POISON)
                graph.replay()
                torch.cuda.synchronize()
                assert P.from_device(db, L.MESHDRAW, n).tobytes() == eager[2.2][0]
                assert TS._host(shadow, w * h, np.uint8, (h, w)).tobytes() == eager[2.2][1]
        c.status()
    finally:
        c.close()


def _animated_occluder():
    s = synth.occluder_scene_indexed(meshlet_bounds=oracle.meshlet_bounds)
    which = np.arange(len(s["draws"]))
    a, k = synth.orbit_animations(s["draws"], which, 4, seed=ANIM_SEED, orbit=1.0, period=(0.5, 1.5))
    return s, a, k


def _oracle_frame(s, draws, state, rref):
    """one frame of raster_ref.oracle_frames with this frame's draw records; `state` carries dvb, mvb, pyramid and depth between frames"""
    meshes, meshlets, cd = s["meshes"], s["meshlets"], s["cull"]
    w, h = s["viewport"]
    draws = draws.copy()
    slots, _ = oracle.assign_visibility_offsets(draws, meshes)
    if not state:
        state.update(dvb=np.zeros(max(1, len(draws)), np.uint32), mvb=np.zeros(max(1, (slots + 31) // 32 + 2), np.uint32), pyr=oracle.Pyramid(w, h),
                     depth=np.zeros((h, w), np.float32))
    rec = {}
    for name, late in (("early", 0), ("late", 1)):
        if late:
            oracle.depthreduce(state["depth"], state["pyr"])
        pd = cd.copy()
        pd["clusterBackfaceEnabled"], pd["postPass"] = 1, 0
        co, c4 = np.zeros(4096 + 64, dtype=L.TASKCMD), np.zeros(4, np.uint32)
        oracle.drawcull(pd, late, 1, draws, meshes, co, c4, state["dvb"], state["pyr"])
        oracle.tasksubmit(c4, co)
        ncmd = int(c4[1]) * 64
        cib, cc4 = np.zeros(ncmd * 64 + 256, np.uint32), np.zeros(4, np.uint32)
        oracle.clustercull(pd, late, co, c4, draws, meshlets, state["mvb"], state["pyr"], cib, cc4)
        oracle.clustersubmit(cc4, cib)
        state["depth"], _, _ = rref.raster(RR.globals_for(cd, (w, h), 0), co, draws, meshlets, s["data"], s["vertices"], cib, cc4, w, h,
                                           depth=None if name == "early" else state["depth"])
        rec[name] = dict(count4=c4.copy(), commands=co[:ncmd].copy(), cc4=cc4.copy(), cib=cib[:int(cc4[2]) * 256].copy(), dvb=state["dvb"].copy(),
                         mvb=state["mvb"].copy(), depth=state["depth"].copy())
    rec["pyramid"] = state["pyr"].data.copy()
    return rec


@pytest.mark.gpu
def test_pipeline_animate_then_frame_equals_the_oracle_frame(rref):
    """three successive times: animate(t) then frame(), every buffer the frame leaves bit-identical to the oracle chain on the downloaded
    draws, the frame-to-frame state (drawVisibility, meshletVisibility, pyramid) carried on both sides"""
    from niagara_amd import pipeline as P
    s, a, k = _animated_occluder()
    pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], task_capacity=4096, cluster_capacity=4096 * 64, fused=True,
                                meshlet_data=s["data"], vertices=s["vertices"])
    try:
        pipe.set_animations(a, k)
        state, previous = {}, s["draws"]
        for time in (0.3, ANIM_TIME, 1.45):
            pipe.animate(time)
            rec = {}

            def grab(name):
                c4, cc4 = pipe.dccb.cpu().numpy().view(np.uint32).copy(), pipe.ccb.cpu().numpy().view(np.uint32).copy()
                rec[name] = dict(count4=c4, commands=P.from_device(pipe.dcb, L.TASKCMD)[:int(c4[1]) * 64].copy(), cc4=cc4,
                                 cib=pipe.cib.cpu().numpy().view(np.uint32)[:int(cc4[2]) * 256].copy(), dvb=pipe.dvb.cpu().numpy().view(np.uint32).copy(),
                                 mvb=pipe.mvb.cpu().numpy().view(np.uint32).copy(), depth=pipe.depth.cpu().numpy().copy())
            pipe.frame(s["cull"], on_phase=grab)
            pipe.ctx.status()
            moved = pipe.download_draws()
            assert (moved["position"] != previous["position"]).any() and (moved["meshletVisibilityOffset"] == pipe.draws_host["meshletVisibilityOffset"]).all()
            previous = moved
            want = _oracle_frame(s, moved, state, rref)
            assert pipe.pyramid.data.cpu().numpy().tobytes() == want["pyramid"].tobytes(), time
            for ph in ("early", "late"):
                for key in ("count4", "commands", "cc4", "cib", "dvb", "mvb"):
                    assert rec[ph][key].tobytes() == want[ph][key].tobytes(), (time, ph, key)
                assert rec[ph]["depth"].view(np.uint32).tobytes() == want[ph]["depth"].view(np.uint32).tobytes(), (time, ph)
            assert want["late"]["count4"][0] > 0 and (want["late"]["depth"] > 0).any()
    finally:
        pipe.ctx.close()


@pytest.mark.gpu
def test_pipeline_traced_shadows_follow_the_animation(shref):
    """build_rt_scene(dynamic=True): animate(t) rebuilds the TLAS in stream order and shade(shadow="trace")'s 320 x 192 mask is the
    restatement's on the downloaded draws — and not the unanimated mask (ANIM_SEED)"""
    import torch
    s, a, k = _animated_occluder()
    w, h = s["viewport"]
    assert (w, h) == (320, 192)
    pipe = TG._pipeline(s, 0)
    try:
        vis = pipe.new_visibility()
        for _ in range(2):
            pipe.frame(s["cull"], post_pass=True, visibility=vis)
        pipe.build_rt_scene(s["meshes"], s["indices"], s["vertices"], s["draws"], dynamic=True)
        pipe.set_animations(a, k)
        depth = pipe.depth.cpu().numpy().copy()
        sd = host.build_shadow_data(synth.make_globals(s["cull"], (w, h)), TG.SUN, 0.0, 0, w, h)
        zeros = np.zeros((h, w), np.uint8)

        def traced():
            t = torch.zeros((h, w), dtype=torch.int32, device=pipe.ctx.device)
            pipe.shade(s["cull"], t, t.clone(), (0.0, 0.0, 0.0), TG.SUN, shadow="trace", blur=False, checkerboard=False, quality=1)
            pipe.ctx.status()
            return pipe.shadow_image.cpu().numpy().copy()
        before = shref.shadow_trace(sd, s, depth, zeros, 1)
        TG._report("before the animation", traced(), before)
        pipe.animate(ANIM_TIME)
        got = traced()
        moved = pipe.download_draws()
        after = shref.shadow_trace(sd, dict(s, draws=moved), depth, zeros, 1)
        print("the animation changes %d texels of the mask" % int((before != after).sum()))
        assert (before != after).sum() >= 50
        TG._report("after the animation", got, after)
        assert pipe.ctx.rt_scene_download().tobytes() == host.rt_tlas_build_host(pipe.rt_scene, moved).tobytes()
        assert pipe.depth.cpu().numpy().tobytes() == depth.tobytes()
    finally:
        pipe.ctx.close()


@pytest.mark.gpu
def test_refused_calls_launch_nothing():
    from niagara_amd import pipeline as P
    draws0 = _random_records(DRAWS, L.MESHDRAW, 3)
    a, k = AR.fuzz_table(100, DRAWS, seed=4, light_count=10)
    c = P.Context()
    try:
        db, lb = TS._dev(c, draws0, 64), TS._dev(c, _random_records(10, L.LIGHT, 5), 64)
        with pytest.raises(NvError, match="NV_ESTATE"):  # no uploaded table
            c.animate_draws(1.0, db, DRAWS)
        bad = a.copy()
        bad["period"][50] = 0.0
        with pytest.raises(NvError, match="NV_EINVAL"):  # the validator's refusals reach the upload
            c.upload_animations(bad, k, DRAWS, 10)
        with pytest.raises(NvError, match="NV_EINVAL"):
            c.upload_animations(a, k, DRAWS, 9)
        with pytest.raises(NvError, match="NV_ESTATE"):  # a refused upload leaves no table behind
            c.animate_draws(1.0, db, DRAWS)
        c.upload_animations(a, k, DRAWS, 10)
        for time in (float("nan"), float("inf"), -float("inf")):
            with pytest.raises(NvError, match="NV_EINVAL"):
                c.animate_draws(time, db, DRAWS)
        with pytest.raises(NvError, match="NV_EINVAL"):  # drawCount below the uploaded bound
            c.animate_draws(1.0, db, DRAWS - 1)
        with pytest.raises(NvError, match="NV_EINVAL"):  # lightCount below the uploaded bound
            c.animate_draws(1.0, db, DRAWS, lb, 9)
        with pytest.raises(NvError, match="NV_EINVAL"):  # a misaligned d_draws
            c.animate_draws(1.0, db[4:], DRAWS)
        with pytest.raises(NvError, match="NV_EINVAL"):  # NULL draws
            c.animate_draws(1.0, None, DRAWS)
        c.status()
        assert TS._host(db, draws0.nbytes, L.MESHDRAW, (DRAWS,)).tobytes() == draws0.tobytes()  # nothing ran
        c.animate_draws(1.0, db, DRAWS, lb, 10)  # a valid call afterwards works
        c.status()
        want = draws0.copy()
        host.animate_draws_host(1.0, a, k, want, None, light_count=10)
        got = TS._host(db, draws0.nbytes, L.MESHDRAW, (DRAWS,))
        assert (got["position"].view(np.uint32) == want["position"].view(np.uint32)).all() and got.tobytes() != draws0.tobytes()
        c.upload_animations(None, None, 0)  # dropped
        with pytest.raises(NvError, match="NV_ESTATE"):
            c.animate_draws(1.0, db, DRAWS)
    finally:
        c.close()


@pytest.mark.gpu
def test_a_sharded_pipeline_refuses():
    from niagara_amd import pipeline as P
    s = synth.occluder_scene(meshlet_bounds=oracle.meshlet_bounds)
    a, k = synth.orbit_animations(s["draws"], [0, 1], 2, seed=1)
    pipe = P.ShardedVisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], rank=0, world=1, task_capacity=4096,
                                       cluster_capacity=4096 * 64, meshlet_data=s["data"], vertices=s["vertices"])
    try:
        for call in (lambda: pipe.set_animations(a, k), lambda: pipe.animate(0.5)):
            with pytest.raises(NvError, match="is not available on a sharded pipeline"):
                call()
    finally:
        pipe.ctx.close()
