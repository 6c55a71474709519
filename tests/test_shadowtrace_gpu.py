"""nv_shadow_trace on the MI355X against the brute-force restatement tests/shadow_ref.c on the same input bytes: the mask
byte for byte (T and the ray set-up hold no pow or exp2: there is no tolerance).  Outputs are poisoned with a byte that is neither 0 nor
255 before every launch and carry a 64-byte tail that must keep its bytes."""
import numpy as np
import pytest

import oracle
import shade_ref as SR
import shadow_ref as SH
import test_shade_gpu as TS
import visattr_ref as VA
from niagara_amd import host, synth
from niagara_amd import layouts as L

SIZES = [(1, 1), (7, 5), (65, 17), (67, 37)]  # (65, 17): the 8 x 8 tiles of a wave + 1 in both directions
POISON = 0x5A
RADIUS = 8.0           # the fuzz scene of the small images: 20 instances within +-8 of the camera
SMALL = (6, 3, 8.0)    # the second trip's scene: instances, seed, radius
SUN = np.array([2.0, 0.3, 1.0]) / np.linalg.norm([2.0, 0.3, 1.0])  # tests/test_shadowtrace_cpu.py records why


@pytest.fixture(scope="session")
def shref(tmp_path_factory):
    return SH.load(tmp_path_factory.mktemp("shadow_ref_gpu"))


@pytest.fixture(scope="session")
def sref(tmp_path_factory):
    return SR.load(tmp_path_factory.mktemp("shade_ref_shadow_gpu"))


@pytest.fixture(scope="module")
def scene():
    """the small instanced scene of the fuzz, drawn together around the camera so that a good part of the rays hits something"""
    return SH.fuzz_scene(instances=20, seed=11, radius=RADIUS)


@pytest.fixture(scope="module")
def ctx(scene):
    from niagara_amd import pipeline as P
    c = P.Context()
    c.rt_scene_upload(c.rt_scene_build(scene["meshes"], scene["indices"], scene["vertices"], scene["draws"]))
    yield c
    c.close()


def _inputs(w, h, jitter, checkerboard, seed=0):
    """ShadowData of niagara's default camera at a w x h viewport and a random depth image: view-space distances 1 .. 60 (depth = znear /
    distance, in (0, 1]), a tenth of the texels exact zeros (sky)"""
    rng = np.random.default_rng(100 * w + h + seed)
    cd = host.build_cull_data(viewport=(w, h), pyramid=(host.previous_pow2(w), host.previous_pow2(h)))
    sd = host.build_shadow_data(synth.make_globals(cd, (w, h)), SUN, jitter, checkerboard, w, h)
    depth = (0.1 / np.exp(rng.uniform(0.0, np.log(60.0), (h, w)))).astype(np.float32)
    depth[rng.random((h, w)) < 0.1] = 0.0
    if w * h > 4:
        depth.reshape(-1)[0] = 1.0
    return sd, depth


def _trace(ctx, sd, depth, quality):
    """one launch into a poisoned mask with a tail: the mask's bytes on the host"""
    h, w = depth.shape
    d, out = TS._dev(ctx, depth), TS._out(ctx, w * h)
    ctx.shadow_trace(sd, d, out, w, h, quality)
    ctx.status()
    return TS._host(out, w * h, np.uint8, (h, w))


def _report(name, got, want):
    diff = int((got != want).sum())
    print("%s: %d texels, %d occluded, %d lit, %d kept, %d differences" % (name, want.size, int((want == 0).sum()), int((want == 255).sum()),
                                                                          int((want == POISON).sum()), diff))
    assert diff == 0


@pytest.mark.gpu
@pytest.mark.parametrize("checkerboard", [0, 1])
@pytest.mark.parametrize("size", SIZES)
def test_mask_equals_the_restatement(size, checkerboard, ctx, scene, shref):
    w, h = size
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    owned = ((x ^ y ^ checkerboard) & 1) == 0 if checkerboard else np.ones((h, w), bool)  # x = 2 gx + ((y ^ checkerboard) & 1)
    both = set()
    for quality in (0, 1):
        for jitter in (0.0, 1e-2):
            sd, depth = _inputs(w, h, jitter, checkerboard)
            want = shref.shadow_trace(sd, scene, depth, np.full((h, w), POISON, np.uint8), quality)
            got = _trace(ctx, sd, depth, quality)
            assert (want[~owned] == POISON).all() and np.isin(want[owned], (0, 255)).all()
            assert (got[~owned] == POISON).all()  # the other parity keeps the poison exactly
            _report("%dx%d checkerboard %d quality %d jitter %g" % (w, h, checkerboard, quality, jitter), got, want)
            assert (want[owned][depth[owned] == 0] == 255).all()  # sky
            both |= set(np.unique(want[owned]).tolist())
    if w * h >= 1000:
        assert both == {0, 255}


def _pipeline(s, near_clip):
    from niagara_amd import pipeline as P
    return P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], task_capacity=4096, cluster_capacity=4096 * 64, fused=True,
                                vertices=s["vertices"], meshlet_data=s["data"], near_clip=bool(near_clip), stable_ids=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["occluder", "interior"])
def test_frame_scenes_with_the_rasterised_depth(name, shref):
    """320 x 192, the depth target the pipeline's own closed-loop frames leave"""
    s, near_clip = (synth.occluder_scene_indexed(meshlet_bounds=oracle.meshlet_bounds), 0) if name == "occluder" else \
        (synth.interior_scene_indexed(meshlet_bounds=oracle.meshlet_bounds), 1)
    w, h = s["viewport"]
    pipe = _pipeline(s, near_clip)
    try:
        vis = pipe.new_visibility()
        for _ in range(2):
            pipe.frame(s["cull"], post_pass=True, visibility=vis)
        pipe.build_rt_scene(s["meshes"], s["indices"], s["vertices"], s["draws"])
        depth = pipe.depth.cpu().numpy()
        covered = depth > 0
        assert covered.sum() > 1000 and (~covered).sum() > 1000
        for quality, jitter, checkerboard in ((1, 1e-2, 0), (0, 0.0, 1)):
            sd = host.build_shadow_data(synth.make_globals(s["cull"], (w, h)), SUN, jitter, checkerboard, w, h)
            want = shref.shadow_trace(sd, s, depth, np.full((h, w), POISON, np.uint8), quality)
            got = _trace(pipe.ctx, sd, depth, quality)
            _report("%s quality %d jitter %g checkerboard %d" % (name, quality, jitter, checkerboard), got, want)
            if not checkerboard:
                assert (want[covered] == 0).sum() >= 200 and (want[covered] == 255).sum() >= 200 and (want[~covered] == 255).all()
    finally:
        pipe.ctx.close()


@pytest.mark.gpu
def test_the_persistent_grid_takes_its_second_trip(shref):
    """The launch is persistent_grid(ctx, 8) workgroups of four waves, a wave per 8 x 8 tile: one trip covers 32 tiles per compute unit.
    2051 columns are 257 tile columns (the last one 3 wide) and cus + 1 rows are cus / 8 + 1 tile rows (the last one 1 high): more tiles
    than one trip, the later ones ragged.  Four instances keep the brute force within seconds."""
    import torch
    from niagara_amd import pipeline as P
    small = SH.fuzz_scene(instances=SMALL[0], seed=SMALL[1], radius=SMALL[2])
    c = P.Context()
    try:
        cus = torch.cuda.get_device_properties(c.device).multi_processor_count
        w, h = 2051, cus + 1
        tiles_x, tiles_y = (w + 7) // 8, (h + 7) // 8
        trip = cus * 8 * 4  # niagara_amd/csrc/context.hip persistent_grid(ctx, 8) x shadowtrace.hip ST_WAVES
        assert tiles_x * tiles_y > trip and w % 8 != 0
        c.rt_scene_upload(c.rt_scene_build(small["meshes"], small["indices"], small["vertices"], small["draws"]))
        sd, depth = _inputs(w, h, 1e-2, 0)
        want = shref.shadow_trace(sd, small, depth, np.full((h, w), POISON, np.uint8), 1)
        got = _trace(c, sd, depth, 1)
        x, y = np.meshgrid(np.arange(w), np.arange(h))
        later = (y // 8) * tiles_x + x // 8 >= trip  # the tile of the pixel is dealt in a later trip
        assert later.any()
        print("second trip: %d tiles, %d per trip; %d differences in the later trips' rows" % (tiles_x * tiles_y, trip, int((got != want)[later].sum())))
        assert (got[later] != POISON).all(), "the later trips wrote nothing"
        _report("second trip %dx%d" % (w, h), got, want)
        assert set(np.unique(want[later]).tolist()) == {0, 255}
    finally:
        c.close()


@pytest.mark.gpu
def test_refused_calls_launch_nothing(ctx, scene):
    from niagara_amd import pipeline as P
    from niagara_amd._lib import NvError
    w, h = 21, 3
    sd, depth = _inputs(w, h, 0.0, 0)
    d, out = TS._dev(ctx, depth, 8), TS._out(ctx, w * h)
    wrong = sd.copy()
    wrong["imageSize"][0] = (w + 1, h)
    call = lambda c=ctx, **k: c.shadow_trace(**{**dict(shadow_data=sd, depth=d, shadow=out, width=w, height=h, quality=1), **k})
    fresh = P.Context()  # no scene uploaded
    try:
        with pytest.raises(NvError):
            call(c=fresh)
        blob = fresh.rt_scene_build(scene["meshes"], scene["indices"], scene["vertices"], scene["draws"])
        raw = np.zeros(blob.nbytes + 16, np.uint8)
        bad = raw[(-raw.ctypes.data) % 16:][:blob.nbytes]
        bad[:] = blob
        assert host.rt_scene_validate(bad)
        bad[int(bad[36:40].view(np.uint32)[0]) + 12:][:4] = 0  # the TLAS root's skip = 0: a loop
        with pytest.raises(NvError):  # a corrupt blob is refused at load
            fresh.rt_scene_upload(bad)
        fresh.rt_scene_upload(blob)
        fresh.rt_scene_upload(None)  # dropped again
        with pytest.raises(NvError):
            call(c=fresh)
        fresh.status()
    finally:
        fresh.close()
    for kw in (dict(quality=2), dict(quality=-1), dict(shadow_data=wrong), dict(width=w + 1), dict(depth=None), dict(shadow=None), dict(width=0), dict(height=16385),
               dict(depth=d[1:])):
        with pytest.raises(NvError):
            call(**kw)
    ctx.status()
    assert (out == POISON).all()
    call()
    ctx.status()
    assert np.isin(out.cpu().numpy()[:w * h], (0, 255)).all()


@pytest.mark.gpu
def test_the_chain_replays_from_a_captured_graph(ctx, scene, shref):
    """trace -> fill -> blur horizontal -> blur vertical -> final, a linear chain: two replays give the bytes of the direct calls"""
    import torch
    w, h = 67, 37
    i = SR.test_inputs(w, h)
    sh, depth_host = _inputs(w, h, 1e-2, 1)
    shade = SR.test_shade_data(w, h, 1)
    g0, g1, depth = TS._dev(ctx, i["gbuffer0"]), TS._dev(ctx, i["gbuffer1"]), TS._dev(ctx, depth_host)
    shadow, tmp, out = TS._out(ctx, w * h), TS._out(ctx, w * h), TS._out(ctx, w * h * 4)

    def reset():
        tmp.fill_(POISON), out.fill_(POISON), shadow.fill_(POISON)

    def chain():
        ctx.shadow_trace(sh, depth, shadow, w, h, 1)
        ctx.shadow_fill(shadow, depth, w, h, 1)
        ctx.shadow_blur(tmp, shadow, depth, w, h, 1, 0.1)
        ctx.shadow_blur(shadow, tmp, depth, w, h, 0, 0.1)
        ctx.shade_final(shade, g0, g1, depth, shadow, out, w, h)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        reset()
        ctx.shadow_trace(sh, depth, shadow, w, h, 1)
        torch.cuda.synchronize()
        traced = shadow.cpu().numpy().copy()
        want = shref.shadow_trace(sh, scene, depth_host, np.full((h, w), POISON, np.uint8), 1)
        _report("the chain's trace", traced[:w * h].reshape(h, w), want)
        reset()
        chain()
        torch.cuda.synchronize()
        eager = [t.cpu().numpy().copy() for t in (shadow, tmp, out)]
        assert (eager[2][:w * h * 4] != POISON).any()
        reset()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            chain()
        torch.cuda.synchronize()
        assert (out == POISON).all() and (shadow == POISON).all()  # nothing ran during capture
        for _ in range(2):
            reset()
            graph.replay()
            torch.cuda.synchronize()
            for t, e in zip((shadow, tmp, out), eager):
                assert t.cpu().numpy().tobytes() == e.tobytes()
    ctx.status()


@pytest.mark.gpu
def test_the_pipeline_shades_with_traced_shadows(shref, sref):
    """VisibilityPipeline.shade(shadow="trace") against the restatement chain shadow_ref -> shade_ref.shade on the G-buffer words and the depth
    target the GPU passes left.  The traced mask is exact, so where final reads it directly the colour obeys tests/test_shade_gpu.py's one-code
    rule (every channel within one code, at least 90 % equal, alpha 255); with a filter stage between the mask and final (fill, blur) that
    file's rule for its chains applies (two codes: a stage reads its predecessor's quantised output, so one code may carry)."""
    s = VA.with_attributes(synth.occluder_scene(meshlet_bounds=oracle.meshlet_bounds))
    indices, meshes = synth.indexed_geometry(s["meshes"], s["meshlets"], s["data"])
    rt = dict(meshes=meshes, indices=indices, vertices=s["vertices"], draws=s["draws"])
    w, h = s["viewport"]
    pipe = _pipeline(s, 0)
    try:
        from niagara_amd._lib import NvError
        vis = pipe.new_visibility()
        for _ in range(2):
            pipe.frame(s["cull"], post_pass=True, visibility=vis)
        res = pipe.resolve(s["cull"], vis)
        att = pipe.attributes(s["cull"], res["records"], s["materials"], attributes=False)
        camera = (0.0, 0.0, 0.0)
        with pytest.raises(NvError):  # no scene yet
            pipe.shade(s["cull"], att["gbuffer0"], att["gbuffer1"], camera, SUN, shadow="trace")
        blob = pipe.build_rt_scene(meshes, indices, s["vertices"], s["draws"])
        assert host.rt_scene_validate(blob)
        g0, g1 = (att[k].cpu().numpy().view(np.uint32) for k in ("gbuffer0", "gbuffer1"))
        depth = pipe.depth.cpu().numpy()
        znear = float(s["cull"]["znear"][0])
        g = synth.make_globals(s["cull"], (w, h))
        sd = host.build_shade_data(g, camera, SUN, 1, w, h)
        for quality, blur, checkerboard in ((1, False, False), (0, False, False), (0, False, True), (1, True, False), (1, True, True)):
            color = pipe.shade(s["cull"], att["gbuffer0"], att["gbuffer1"], camera, SUN, shadow="trace", blur=blur, checkerboard=checkerboard, quality=quality)
            pipe.ctx.status()
            sh = host.build_shadow_data(g, SUN, 1e-2 if blur else 0.0, 1 if checkerboard else 0, w, h)
            mask = shref.shadow_trace(sh, rt, depth, np.zeros((h, w), np.uint8), quality)  # the pipeline's mask starts out as zeros
            if not blur and not checkerboard and quality == 1:
                _report("the pipeline's mask", pipe.shadow_image.cpu().numpy(), mask)
                assert (mask[depth > 0] == 0).sum() >= 200
            want = sref.shade(sd, g0, g1, depth, mask, blur=blur, checkerboard=checkerboard, znear=znear)
            got = SR.channels(color.cpu().numpy().view(np.uint32))
            name = "traced shadows quality %d blur %d checkerboard %d" % (quality, blur, checkerboard)
            if blur or checkerboard:
                d = np.abs(got - SR.channels(want))
                print("%s: %d channels, %d differ, largest difference %d" % (name, d.size, int((d != 0).sum()), int(d.max())))
                assert d.max() <= 2 and (got[..., 3] == 255).all()
            else:
                TS._close(name, got, SR.channels(want), alpha=True)
        # a caller's mask and no mask behave as before
        import torch
        own = torch.from_numpy(mask.copy()).to(pipe.ctx.device)
        a = pipe.shade(s["cull"], att["gbuffer0"], att["gbuffer1"], camera, SUN, shadow=own, blur=False)
        b = sref.shade(sd, g0, g1, depth, mask, blur=False, znear=znear)
        TS._close("a caller's mask", SR.channels(a.cpu().numpy().view(np.uint32)), SR.channels(b), alpha=True)
        assert (pipe.depth.cpu().numpy() == depth).all()
    finally:
        pipe.ctx.close()
    assert L.SHADOWDATA.itemsize == 96
