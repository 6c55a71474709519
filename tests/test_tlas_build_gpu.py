"""nv_rt_tlas_build on the MI355X.  Two kinds of check, neither with a tolerance: the device scene read back through
nv_rt_scene_download equals the host twin's blob byte for byte (the tree is unique, the boxes are the same text), and the mask nv_shadow_trace
writes from the rebuilt TLAS equals the brute-force restatement tests/shadow_ref.c on the MOVED draws byte for byte."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle
import shadow_ref as SH
import test_shade_gpu as TS
import test_shadowtrace_gpu as TG
import tlas_ref as TR
from niagara_amd import host, synth
from niagara_amd import layouts as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = TG.POISON
K = 2048            # niagara_amd/csrc/rttlas.hip TL_SORT_KEYS: keys per workgroup of the sort's count and scatter launches
MAX_DRAWS = 100000  # the reservation of the module's context
MOVE_SEED = 2       # chosen on the CPU: the moved and unmoved masks differ in 102 .. 1124 texels over the eight cases below


def test_the_quoted_sort_tile_is_the_kernel_files():
    src = open(os.path.join(ROOT, "niagara_amd", "csrc", "rttlas.hip")).read()
    assert int(re.search(r"TL_SORT_KEYS = (\d+);", src).group(1)) == K


@pytest.fixture(scope="module")
def shref(tmp_path_factory):
    return SH.load(tmp_path_factory.mktemp("shadow_ref_tlas_gpu"))


@pytest.fixture(scope="module")
def scene():
    """test_shadowtrace_gpu.py's fuzz scene around the camera, with a third mesh that has no triangles"""
    return TR.with_empty_mesh(SH.fuzz_scene(instances=20, seed=11, radius=TG.RADIUS))


@pytest.fixture(scope="module")
def blob(scene):
    return host.rt_scene_build(scene["meshes"], scene["indices"], scene["vertices"], scene["draws"])


@pytest.fixture(scope="module")
def ctx(blob):
    from niagara_amd import pipeline as P
    c = P.Context()
    c.rt_scene_upload(blob)
    c.rt_scene_reserve_dynamic(MAX_DRAWS)
    yield c
    c.close()


def _draws_dev(ctx, draws):
    return TS._dev(ctx, draws if len(draws) else np.zeros(1, L.MESHDRAW), 64)


def _rebuild(ctx, draws):
    dev = _draws_dev(ctx, draws)
    ctx.rt_tlas_build(dev, len(draws))
    ctx.status()
    return dev


def _equal_blobs(name, got, want):
    hg, hw = TR.sections(got)[0], TR.sections(want)[0]
    diff = int((got != want).sum()) if got.nbytes == want.nbytes else -1
    print("%s: %d instances (host %d), %d nodes, %d bytes, %d differing bytes" % (name, int(hg["instances"]), int(hw["instances"]), int(hg["tlasNodes"]),
                                                                                  got.nbytes, diff))
    assert got.nbytes == want.nbytes and diff == 0


@pytest.mark.gpu
def test_the_reservation_keeps_the_static_scene(ctx, blob):
    """before the first rebuild the header points at the static TLAS: the download is the uploaded blob"""
    from niagara_amd import pipeline as P
    c = P.Context()
    try:
        c.rt_scene_upload(blob)
        c.rt_scene_reserve_dynamic(64)
        _equal_blobs("reserved, not rebuilt", c.rt_scene_download(), blob)
        c.rt_scene_reserve_dynamic(500)  # a second reservation re-houses the current scene
        _equal_blobs("reserved twice", c.rt_scene_download(), blob)
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2, 3, K - 1, K, K + 1, 3 * K + 5, 100000])
def test_device_bytes_equal_the_host_twin(n, ctx, blob):
    draws = TR.mixed_draws(n, 500 + n, 2, 40.0, empty_mesh=2)
    want = host.rt_tlas_build_host(blob, draws)
    _rebuild(ctx, draws)
    got = ctx.rt_scene_download()
    _equal_blobs("n = %d" % n, got, want)
    assert host.rt_scene_validate(got)
    st = host.rt_scene_stats(got)
    if n >= K - 1:  # the input condition: non-casters, duplicate keys and several sort tiles took part
        keys = TR.check_blob(got)["keys"]
        assert 0 < st["instances"] < n and len(np.unique(keys)) < len(keys)
    elif n:
        assert st["instances"] == n


@pytest.mark.gpu
def test_a_small_build_follows_a_large_one(ctx, blob):
    """the scratch and the dynamic sections hold the large build's data when the small one runs"""
    large, small = TR.mixed_draws(100000, 41, 2, 40.0, empty_mesh=2), TR.mixed_draws(3, 42, 2, 40.0)
    _rebuild(ctx, large)
    _equal_blobs("100000", ctx.rt_scene_download(), host.rt_tlas_build_host(blob, large))
    _rebuild(ctx, small)
    _equal_blobs("3 behind 100000", ctx.rt_scene_download(), host.rt_tlas_build_host(blob, small))
    _rebuild(ctx, small[:0])
    got = ctx.rt_scene_download()
    _equal_blobs("0 behind 3", got, host.rt_tlas_build_host(blob, small[:0]))
    assert host.rt_scene_stats(got)["tlasNodes"] == 0


def _mask(ctx, sd, depth, quality):
    return TG._trace(ctx, sd, depth, quality)


@pytest.mark.gpu
@pytest.mark.parametrize("checkerboard", [0, 1])
@pytest.mark.parametrize("quality", [0, 1])
@pytest.mark.parametrize("size", [(65, 17), (67, 37)])
def test_mask_of_the_moved_draws_equals_the_restatement(size, quality, checkerboard, blob, scene, shref):
    """static upload -> reserve -> every draw moved -> rt_tlas_build -> shadow_trace"""
    from niagara_amd import pipeline as P
    w, h = size
    moved = dict(scene, draws=TR.moved(scene["draws"], MOVE_SEED, TG.RADIUS))
    sd, depth = TG._inputs(w, h, 1e-2, checkerboard)
    poison = np.full((h, w), POISON, np.uint8)
    want, stale = shref.shadow_trace(sd, moved, depth, poison, quality), shref.shadow_trace(sd, scene, depth, poison, quality)
    print("moved and unmoved masks differ in %d texels" % int((want != stale).sum()))
    assert (want != stale).sum() >= 50  # the input condition, on the restatement alone
    c = P.Context()
    try:
        c.rt_scene_upload(blob)
        c.rt_scene_reserve_dynamic(len(scene["draws"]))
        TG._report("reserved, static", _mask(c, sd, depth, quality), stale)
        _rebuild(c, moved["draws"])
        TG._report("%dx%d quality %d checkerboard %d moved" % (w, h, quality, checkerboard), _mask(c, sd, depth, quality), want)
        _rebuild(c, scene["draws"])  # unchanged draws: the static scene's mask from the rebuilt tree
        TG._report("rebuilt from the unmoved draws", _mask(c, sd, depth, quality), stale)
    finally:
        c.close()


@pytest.mark.gpu
def test_one_transform_three_hundred_times(ctx, scene, shref):
    """all keys equal: the tie bits decide every split"""
    w, h = 67, 37
    draws = np.repeat(TR.moved(scene["draws"][1:2], 5, 3.0), 300)
    draws["postPass"], draws["scale"] = 0, 1.5
    sd, depth = TG._inputs(w, h, 1e-2, 0)
    want = shref.shadow_trace(sd, dict(scene, draws=draws[:1]), depth, np.full((h, w), POISON, np.uint8), 1)  # 300 copies occlude what one does
    assert (want == 0).sum() >= 50
    _rebuild(ctx, draws)
    r = TR.check_blob(ctx.rt_scene_download())
    assert len(np.unique(r["keys"])) == 1 and r["depth"] == 9
    TG._report("300 x one transform", _mask(ctx, sd, depth, 1), want)


@pytest.mark.gpu
def test_a_draw_stops_casting_and_casts_again(ctx, scene, shref):
    w, h = 67, 37
    sd, depth = TG._inputs(w, h, 1e-2, 0)
    base = TR.moved(scene["draws"], MOVE_SEED, TG.RADIUS)
    base["postPass"] = 0
    poison = np.full((h, w), POISON, np.uint8)
    full = shref.shadow_trace(sd, dict(scene, draws=base), depth, poison, 1)
    # the draw whose removal changes the most texels
    alone = [int((shref.shadow_trace(sd, dict(scene, draws=np.delete(base, i)), depth, poison, 1) != full).sum()) for i in range(len(base))]
    i = int(np.argmax(alone))
    assert alone[i] >= 20
    for how in ("postPass", "scale", "position"):
        off = base.copy()
        if how == "postPass":
            off["postPass"][i] = 2
        elif how == "scale":
            off["scale"][i] = 0.0
        else:
            off["position"][i, 1] = np.nan
        want = shref.shadow_trace(sd, dict(scene, draws=off), depth, poison, 1)
        assert (want != full).sum() == alone[i]
        _rebuild(ctx, off)
        assert host.rt_scene_stats(ctx.rt_scene_download())["instances"] == len(base) - 1
        TG._report("draw %d off by %s" % (i, how), _mask(ctx, sd, depth, 1), want)
        _rebuild(ctx, base)
        assert host.rt_scene_stats(ctx.rt_scene_download())["instances"] == len(base)
        TG._report("draw %d casts again" % i, _mask(ctx, sd, depth, 1), full)


@pytest.mark.gpu
def test_the_chain_replays_from_a_captured_graph(scene, blob, shref):
    """update_draws -> rt_tlas_build -> shadow_trace captured once; between the replays the device draw buffer is rewritten by a copy outside
    the graph, and each replay's mask is the restatement's of THAT state"""
    import torch
    from niagara_amd import pipeline as P
    w, h = 67, 37
    sd, depth_host = TG._inputs(w, h, 1e-2, 0)
    n = len(scene["draws"])
    states = [TR.moved(scene["draws"], s, TG.RADIUS) for s in (MOVE_SEED, 7)]
    wants = [shref.shadow_trace(sd, dict(scene, draws=s), depth_host, np.full((h, w), POISON, np.uint8), 1) for s in states]
    assert (wants[0] != wants[1]).sum() >= 50
    c = P.Context()
    try:
        c.rt_scene_upload(blob)
        c.rt_scene_reserve_dynamic(n)
        mb, db = P.to_device(scene["meshes"], c.device), P.to_device(scene["draws"], c.device)
        c.upload_meshes(mb, len(scene["meshes"]))
        c.upload_draws(db, n, mb)
        depth, shadow = TS._dev(c, depth_host), TS._out(c, w * h)
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=st):
                c.update_draws(db, 0, n)
                c.rt_tlas_build(db, n)
                c.shadow_trace(sd, depth, shadow, w, h, 1)
            torch.cuda.synchronize()
            assert (shadow == POISON).all()  # nothing ran during capture
            _equal = TR.sections(c.rt_scene_download())[0]
            assert int(_equal["tlasOff"]) == int(TR.sections(blob)[0]["tlasOff"])  # the header still points at the static TLAS
            for state, want in zip(states + states[:1], wants + wants[:1]):
                db.copy_(P.to_device(state, c.device))  # outside the graph
                shadow.fill_(POISON)
                graph.replay()
                torch.cuda.synchronize()
                TG._report("replay", TS._host(shadow, w * h, np.uint8, (h, w)), want)
                assert c.rt_scene_download().tobytes() == host.rt_tlas_build_host(blob, state).tobytes()
        c.status()
    finally:
        c.close()


@pytest.mark.gpu
def test_refused_calls_launch_nothing(scene, blob, shref):
    from niagara_amd import pipeline as P
    from niagara_amd._lib import NvError
    w, h = 21, 3
    sd, depth_host = TG._inputs(w, h, 0.0, 0)
    draws = TR.moved(scene["draws"], MOVE_SEED, TG.RADIUS)
    c = P.Context()
    try:
        with pytest.raises(NvError):  # no scene
            c.rt_scene_reserve_dynamic(8)
        with pytest.raises(NvError):
            c.rt_scene_download()
        c.rt_scene_upload(blob)
        dev = _draws_dev(c, draws)
        depth, out = TS._dev(c, depth_host, 8), TS._out(c, w * h)
        with pytest.raises(NvError):  # no reservation
            c.rt_tlas_build(dev, len(draws))
        for bad in (0, 1 << 29):
            with pytest.raises(NvError):
                c.rt_scene_reserve_dynamic(bad)
        c.rt_scene_reserve_dynamic(len(draws))
        with pytest.raises(NvError):  # drawCount > maxDraws
            c.rt_tlas_build(dev, len(draws) + 1)
        with pytest.raises(NvError):  # NULL draws
            c.rt_tlas_build(None, len(draws))
        c.rt_scene_upload(blob)       # an upload drops the reservation
        with pytest.raises(NvError):
            c.rt_tlas_build(dev, len(draws))
        c.status()
        assert (out == POISON).all()
        assert c.rt_scene_download().tobytes() == blob.tobytes()  # and nothing touched the scene
        c.rt_scene_reserve_dynamic(len(draws))                    # a valid sequence afterwards works
        c.rt_tlas_build(dev, len(draws))
        c.shadow_trace(sd, depth, out, w, h, 1)
        c.status()
        want = shref.shadow_trace(sd, dict(scene, draws=draws), depth_host, np.full((h, w), POISON, np.uint8), 1)
        TG._report("after the refusals", TS._host(out, w * h, np.uint8, (h, w)), want)
    finally:
        c.close()


@pytest.mark.gpu
def test_the_pipeline_moves_its_occluder(shref):
    """occluder_scene with build_rt_scene(dynamic=True): move_draws displaces the wall, shade(shadow="trace")'s mask follows, the depth target
    is untouched by the rebuild"""
    s = synth.occluder_scene_indexed(meshlet_bounds=oracle.meshlet_bounds)
    w, h = s["viewport"]
    pipe = TG._pipeline(s, 0)
    try:
        vis = pipe.new_visibility()
        for _ in range(2):
            pipe.frame(s["cull"], post_pass=True, visibility=vis)
        pipe.build_rt_scene(s["meshes"], s["indices"], s["vertices"], s["draws"], dynamic=True)
        depth = pipe.depth.cpu().numpy().copy()
        sd = host.build_shadow_data(synth.make_globals(s["cull"], (w, h)), TG.SUN, 0.0, 0, w, h)
        zeros = np.zeros((h, w), np.uint8)  # the pipeline's mask starts out as zeros
        before = shref.shadow_trace(sd, s, depth, zeros, 1)
        wall = s["wall"][0]
        rec = s["draws"][wall:wall + 1].copy()
        rec["position"][0] += np.array([-12.0, 0.0, 5.0], np.float32)  # chosen on the CPU reference frame's depth: 2160 texels change
        moved = s["draws"].copy()
        moved[wall] = rec[0]
        after = shref.shadow_trace(sd, dict(s, draws=moved), depth, zeros, 1)
        print("the wall's move changes %d texels of the mask" % int((before != after).sum()))
        assert (before != after).sum() >= 50

        def traced():
            g0 = np.zeros((h, w), np.int32)
            import torch
            t = torch.from_numpy(g0).to(pipe.ctx.device)
            pipe.shade(s["cull"], t, t.clone(), (0.0, 0.0, 0.0), TG.SUN, shadow="trace", blur=False, checkerboard=False, quality=1)
            pipe.ctx.status()
            return pipe.shadow_image.cpu().numpy()
        TG._report("before the move", traced(), before)
        pipe.move_draws(wall, rec)
        TG._report("after the move", traced(), after)
        assert pipe.depth.cpu().numpy().tobytes() == depth.tobytes()
        want_blob = host.rt_tlas_build_host(pipe.rt_scene, pipe.draws_host)
        assert pipe.ctx.rt_scene_download().tobytes() == want_blob.tobytes()
    finally:
        pipe.ctx.close()


@pytest.mark.gpu
def test_poisoned_scratch_and_canaries():
    """the experiments build starts every library-owned block as 0xAB bytes between canary zones: a rebuild that read a word it did not
    write, or stored outside its block, shows there.  A child process, because the library is chosen at import"""
    exp = os.path.join(ROOT, "niagara_amd", "libniagara_vis_exp.so")
    env = dict(os.environ, NV_LIBRARY_PATH=exp)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tlas_runner.py")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    print(out.stdout.decode())
    assert out.returncode == 0 and b"tlas_runner: ok" in out.stdout
