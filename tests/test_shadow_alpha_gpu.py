"""nv_shadow_trace_textured on the MI355X against the brute-force restatement tests/shadow_alpha_ref.c on the same input
bytes: the mask byte for byte (T, the barycentrics and the four-tap alpha hold no pow, exp2 or log2: there is no tolerance).  Outputs are
poisoned with a byte that is neither 0 nor 255 before every launch and carry a 64-byte tail that must keep its bytes."""
import numpy as np
import pytest

import shade_ref as SR
import shadow_alpha_ref as SA
import shadow_ref as SH
import test_shade_gpu as TS
import test_shadow_alpha_cpu as AC
import test_shadowtrace_gpu as TG
from niagara_amd import host, synth
from niagara_amd import layouts as L

SIZES = TG.SIZES
POISON = TG.POISON
SUN = TG.SUN
SMALL = (6, 3, 8.0)  # the second trip's scene: instances, seed, radius


@pytest.fixture(scope="session")
def aref(tmp_path_factory):
    return SA.load(tmp_path_factory.mktemp("shadow_alpha_ref_gpu"))


@pytest.fixture(scope="session")
def shref(tmp_path_factory):
    return SH.load(tmp_path_factory.mktemp("shadow_ref_alpha_gpu"))


def aref_rays(sd, depth):
    """the rays of every pixel (tests/shadow_ref.c shr_rays through a throw-away loader: the ray set-up is shadow_ref's)"""
    import tempfile
    return SH.load(tempfile.mkdtemp(prefix="shadow_ref_rays")).rays(sd, depth)


class Device:
    """a context with a textured scene uploaded and the alpha test's tables on the device"""

    def __init__(self, scene, tset):
        from niagara_amd import pipeline as P
        self.scene, self.tset = scene, tset
        self.ctx = c = P.Context()
        self.blob = c.rt_scene_build(scene["meshes"], scene["indices"], scene["vertices"], scene["draws"], texcoords=True)
        c.rt_scene_upload(self.blob)
        self.draws, self.materials = P.to_device(scene["draws"], c.device), P.to_device(scene["materials"], c.device)
        self.descs = P.to_device(np.ascontiguousarray(tset["descs"], L.TEXTUREDESC), c.device)
        self.texels = TS._dev(c, np.ascontiguousarray(tset["texels"], np.uint32))  # exactly the set's words: nothing behind them to read

    def args(self, **k):
        s, t = self.scene, self.tset
        return {**dict(draws=self.draws, draw_count=len(s["draws"]), materials=self.materials, material_count=len(s["materials"]), textures=self.descs,
                       texture_count=len(t["descs"]), texels=self.texels, texel_words=len(t["texels"])), **k}

    def trace(self, sd, depth, quality=1, **k):
        """one launch into a poisoned mask with a tail: the mask's bytes on the host"""
        h, w = depth.shape
        d, out = TS._dev(self.ctx, depth), TS._out(self.ctx, w * h)
        self.ctx.shadow_trace_textured(sd, d, out, w, h, quality, **self.args(**k))
        self.ctx.status()
        return TS._host(out, w * h, np.uint8, (h, w))


@pytest.fixture(scope="module")
def fuzz():
    s, t = SA.textured_fuzz_scene()
    dev = Device(s, t)
    yield dev
    dev.ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("checkerboard", [0, 1])
@pytest.mark.parametrize("size", SIZES)
def test_mask_equals_the_restatement(size, checkerboard, fuzz, aref):
    w, h = size
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    owned = ((x ^ y ^ checkerboard) & 1) == 0 if checkerboard else np.ones((h, w), bool)
    both, rejected_and_dark = set(), 0
    for jitter in (0.0, 1e-2):
        sd, depth = TG._inputs(w, h, jitter, checkerboard)
        want, rejected = aref.shadow_trace(sd, fuzz.scene, fuzz.tset, depth, np.full((h, w), POISON, np.uint8), 1)
        got = fuzz.trace(sd, depth, 1)
        assert (want[~owned] == POISON).all() and np.isin(want[owned], (0, 255)).all()
        assert (got[~owned] == POISON).all()  # the other parity keeps the poison exactly
        TG._report("%dx%d checkerboard %d jitter %g textured" % (w, h, checkerboard, jitter), got, want)
        assert (want[owned][depth[owned] == 0] == 255).all()  # sky
        both |= set(np.unique(want[owned]).tolist())
        rejected_and_dark += int(((rejected > 0) & (want == 0)).sum())
        # quality 0 is nv_shadow_trace's kernel and bytes
        d, a, b = TS._dev(fuzz.ctx, depth), TS._out(fuzz.ctx, w * h), TS._out(fuzz.ctx, w * h)
        fuzz.ctx.shadow_trace_textured(sd, d, a, w, h, 0, **fuzz.args())
        fuzz.ctx.shadow_trace(sd, d, b, w, h, 0)
        fuzz.ctx.status()
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() and (a[:w * h][owned.reshape(-1)].cpu().numpy() != POISON).all()
    if w * h >= 1000:
        assert both == {0, 255} and rejected_and_dark >= 20


@pytest.mark.gpu
def test_the_layered_scene_splits_the_lanes_of_a_wave(aref):
    """a cut-out wall above a half-covering opaque wall over a flat receiver: neighbouring lanes of a wave disagree at the alpha test.  The sun
    stands at the zenith (+z in this scene's frame), the camera looks down on the receiver"""
    s, t = SA.layered_scene(box=True)
    dev = Device(s, t)
    try:
        w, h = 64, 64
        sd = np.zeros(1, L.SHADOWDATA)
        sd["sunDirection"], sd["imageSize"] = (0.02, 0.03, 1.0), (w, h)
        # an orthographic "inverse view projection": clip x, y in [-1, 1] -> world x, y in [-3.9, 3.9], z = 0; depth is not used
        m = np.zeros((4, 4), np.float32)
        m[0, 0], m[1, 1], m[3, 3] = 3.9, 3.9, 1.0
        sd["inverseViewProjection"] = m.T.reshape(-1)  # column-major
        depth = np.full((h, w), 0.5, np.float32)
        want, rejected = aref.shadow_trace(sd, s, t, depth, np.full((h, w), POISON, np.uint8), 1)
        got = dev.trace(sd, depth, 1)
        TG._report("layered scene", got, want)
        passes = rejected > 0           # the cut-out wall let the ray through at least once
        x = (np.arange(w) + 0.5) / w * 2 - 1
        under_wall = np.broadcast_to(x[None, :] * 3.9 < -0.2, (h, w))  # the opaque wall covers x < 0
        counts = dict(passes_hits=int((passes & under_wall & (want == 0)).sum()), passes_misses=int((passes & ~under_wall & (want == 255)).sum()),
                      stopped_over_wall=int((~passes & under_wall & (want == 0)).sum()), stopped_beside=int((~passes & ~under_wall & (want == 0)).sum()))
        print("layered scene:", counts)
        assert all(v >= 20 for v in counts.values())
        # neighbouring lanes disagree: the mask changes along rows inside 8 x 8 tiles
        assert int((want[:, 1:] != want[:, :-1]).sum()) >= 50
        # a BLAS leaf that holds a rejected and a confirmed triangle for the same ray: the restatement over one leaf of the box at a time
        o, d = aref_rays(sd, depth)
        mixed = 0
        for leaf in SA.leaf_subscenes(dev.blob, s, 2):
            m, r = aref.trace(leaf, t, o, d, 1)
            mixed += int(((m == 0) & (r > 0)).sum())
        print("layered scene: %d (ray, leaf) pairs with a rejected and a confirmed triangle" % mixed)
        assert mixed >= 1
    finally:
        dev.ctx.close()


@pytest.mark.gpu
def test_the_persistent_grid_takes_its_second_trip(aref):
    import torch
    s, t = SA.textured_fuzz_scene(instances=SMALL[0], seed=SMALL[1], radius=SMALL[2])
    dev = Device(s, t)
    try:
        cus = torch.cuda.get_device_properties(dev.ctx.device).multi_processor_count
        w, h = 2051, cus + 1
        tiles_x, tiles_y = (w + 7) // 8, (h + 7) // 8
        trip = cus * 8 * 4  # persistent_grid(ctx, 8) workgroups of four waves
        assert tiles_x * tiles_y > trip and w % 8 != 0
        sd, depth = TG._inputs(w, h, 1e-2, 0)
        want, rejected = aref.shadow_trace(sd, s, t, depth, np.full((h, w), POISON, np.uint8), 1)
        got = dev.trace(sd, depth, 1)
        x, y = np.meshgrid(np.arange(w), np.arange(h))
        later = (y // 8) * tiles_x + x // 8 >= trip
        assert later.any() and (got[later] != POISON).all(), "the later trips wrote nothing"
        TG._report("second trip %dx%d textured" % (w, h), got, want)
        assert set(np.unique(want[later]).tolist()) == {0, 255} and (rejected[later] > 0).any()
    finally:
        dev.ctx.close()


@pytest.mark.gpu
def test_a_rebuilt_tlas_keeps_the_texcoords(aref):
    from niagara_amd import pipeline as P
    s, t = SA.textured_fuzz_scene()
    dev = Device(s, t)
    try:
        c = dev.ctx
        c.rt_scene_reserve_dynamic(len(s["draws"]) + 3)
        kept = c.rt_scene_download()
        assert AC._header(kept)["flags"] == 1 and AC._triangles(kept).tobytes() == AC._triangles(dev.blob).tobytes()
        moved = s["draws"].copy()
        rng = np.random.default_rng(31)
        moved["position"] += rng.uniform(-3, 3, moved["position"].shape).astype(np.float32)
        moved["postPass"] = np.roll(moved["postPass"], 1)
        db = P.to_device(moved, c.device)
        c.rt_tlas_build(db, len(moved))
        w, h = 67, 37
        sd, depth = TG._inputs(w, h, 1e-2, 0)
        ms = dict(s, draws=moved)
        want, rejected = aref.shadow_trace(sd, ms, t, depth, np.full((h, w), POISON, np.uint8), 1)
        still, _ = aref.shadow_trace(sd, s, t, depth, np.full((h, w), POISON, np.uint8), 1)
        got = dev.trace(sd, depth, 1, draws=db)
        TG._report("moved draws, rebuilt TLAS", got, want)
        assert (want != still).sum() >= 50 and ((rejected > 0) & (want == 0)).sum() >= 20
        blob = c.rt_scene_download()
        assert AC._header(blob)["flags"] == 1 and AC._triangles(blob).tobytes() == AC._triangles(dev.blob).tobytes()
        assert blob.tobytes() == host.rt_tlas_build_host(dev.blob, moved).tobytes()
    finally:
        dev.ctx.close()


@pytest.mark.gpu
def test_refused_calls_launch_nothing(fuzz):
    from niagara_amd import pipeline as P
    from niagara_amd._lib import NvError
    w, h = 21, 3
    sd, depth = TG._inputs(w, h, 0.0, 0)
    d, out = TS._dev(fuzz.ctx, depth, 8), TS._out(fuzz.ctx, w * h)
    wrong = sd.copy()
    wrong["imageSize"][0] = (w + 1, h)

    def call(c=fuzz.ctx, **k):
        a = {**dict(shadow_data=sd, depth=d, shadow=out, width=w, height=h, quality=1), **fuzz.args(), **k}
        c.shadow_trace_textured(**a)
    fresh = P.Context()
    try:
        with pytest.raises(NvError):  # no scene uploaded
            call(c=fresh)
        s = fuzz.scene
        fresh.rt_scene_upload(fresh.rt_scene_build(s["meshes"], s["indices"], s["vertices"], s["draws"]))
        with pytest.raises(NvError):  # a scene without the texcoord flag, also at quality 0
            call(c=fresh)
        with pytest.raises(NvError):
            call(c=fresh, quality=0)
        fresh.status()
    finally:
        fresh.close()
    byte = lambda t: t[4:]  # a flat uint8 tensor four bytes on: 4-byte aligned, not 16
    table = [dict(quality=2), dict(quality=-1), dict(shadow_data=wrong), dict(shadow_data=None), dict(width=w + 1), dict(depth=None), dict(shadow=None), dict(width=0),
             dict(height=16385), dict(depth=d[1:]), dict(draws=None), dict(materials=None), dict(textures=None), dict(texels=None),
             dict(draws=byte(fuzz.draws)), dict(materials=byte(fuzz.materials)), dict(textures=byte(fuzz.descs)), dict(texels=fuzz.texels[1:])]
    for kw in table:
        with pytest.raises(NvError):
            call(**kw)
    fuzz.ctx.status()
    assert (out == POISON).all()
    call(draw_count=0, draws=None)  # a NULL array with a zero count is "no draws": every instance is opaque
    call()
    fuzz.ctx.status()
    assert np.isin(out.cpu().numpy()[:w * h], (0, 255)).all()


@pytest.mark.gpu
def test_the_chain_replays_from_a_captured_graph(fuzz, aref):
    """trace -> fill -> blur horizontal -> blur vertical -> final, a linear chain: two replays give the bytes of the direct calls"""
    import torch
    ctx = fuzz.ctx
    w, h = 67, 37
    i = SR.test_inputs(w, h)
    sh, depth_host = TG._inputs(w, h, 1e-2, 1)
    shade = SR.test_shade_data(w, h, 1)
    g0, g1, depth = TS._dev(ctx, i["gbuffer0"]), TS._dev(ctx, i["gbuffer1"]), TS._dev(ctx, depth_host)
    shadow, tmp, out = TS._out(ctx, w * h), TS._out(ctx, w * h), TS._out(ctx, w * h * 4)
    args = fuzz.args()

    def reset():
        tmp.fill_(POISON), out.fill_(POISON), shadow.fill_(POISON)

    def chain():
        ctx.shadow_trace_textured(sh, depth, shadow, w, h, 1, **args)
        ctx.shadow_fill(shadow, depth, w, h, 1)
        ctx.shadow_blur(tmp, shadow, depth, w, h, 1, 0.1)
        ctx.shadow_blur(shadow, tmp, depth, w, h, 0, 0.1)
        ctx.shade_final(shade, g0, g1, depth, shadow, out, w, h)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        reset()
        ctx.shadow_trace_textured(sh, depth, shadow, w, h, 1, **args)
        torch.cuda.synchronize()
        traced = shadow.cpu().numpy().copy()
        want, _ = aref.shadow_trace(sh, fuzz.scene, fuzz.tset, depth_host, np.full((h, w), POISON, np.uint8), 1)
        TG._report("the chain's trace", traced[:w * h].reshape(h, w), want)
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
def test_the_pipeline_shades_with_alpha_tested_shadows(aref, shref):
    """VisibilityPipeline.shade(shadow="trace", textures=True) on the occluder scene with its wall in the post pass and with_textures' cut-out
    albedo, 320 x 192: the mask equals the restatement on the depth target the GPU passes left and differs from textures=False's"""
    from niagara_amd._lib import NvError
    s, _ = AC.cutout_occluder()
    w, h = s["viewport"]
    pipe = TG._pipeline(s, 0)
    try:
        vis = pipe.new_visibility()
        for _ in range(2):
            pipe.frame(s["cull"], post_pass=True, visibility=vis)
        res = pipe.resolve(s["cull"], vis)
        att = pipe.attributes(s["cull"], res["records"], s["materials"], attributes=False)
        camera = (0.0, 0.0, 0.0)
        shade = lambda **k: pipe.shade(s["cull"], att["gbuffer0"], att["gbuffer1"], camera, SUN, shadow="trace", blur=False, **k)
        pipe.build_rt_scene(s["meshes"], s["indices"], s["vertices"], s["draws"])
        for missing in ("set_textures", "materials=", "texcoords=True"):  # each of the three is named while it is missing
            with pytest.raises(NvError) as e:
                shade(textures=True)
            assert missing in str(e.value)
            if missing == "set_textures":
                pipe.set_textures(s["textures"])
            elif missing == "materials=":
                shade_m = shade
                shade = lambda **k: shade_m(materials=s["materials"], **k)
            else:
                pipe.build_rt_scene(s["meshes"], s["indices"], s["vertices"], s["draws"], texcoords=True)
        shade(textures=True)
        pipe.ctx.status()
        got = pipe.shadow_image.cpu().numpy().copy()
        shade()
        pipe.ctx.status()
        opaque = pipe.shadow_image.cpu().numpy().copy()
        depth = pipe.depth.cpu().numpy()
        descs, texels = host.texture_decode_host(s["textures"])
        assert descs.tobytes() == pipe.texture_descs.tobytes() and texels.tobytes() == pipe.texels.cpu().numpy().tobytes()
        sh = host.build_shadow_data(synth.make_globals(s["cull"], (w, h)), SUN, 0.0, 0, w, h)
        want, rejected = aref.shadow_trace(sh, s, dict(descs=descs, texels=texels), depth, np.zeros((h, w), np.uint8), 1)
        TG._report("the pipeline's alpha-tested mask", got, want)
        TG._report("the pipeline's opaque mask", opaque, shref.shadow_trace(sh, s, depth, np.zeros((h, w), np.uint8), 1))
        covered = depth > 0
        differ = int((got != opaque)[covered].sum())
        print("alpha-tested against opaque: %d covered texels differ" % differ)
        assert differ >= 200
    finally:
        pipe.ctx.close()
