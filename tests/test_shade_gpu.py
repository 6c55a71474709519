"""The shading end of the frame on the MI355X: nv_shadow_fill, nv_shadow_blur and nv_shade_final against the fp32 build of
tests/shade_ref.c on the same input bytes — every 8-bit channel within one code, alpha exactly 255, at least 90 % of the channels equal (the
device's and glibc's powf / exp2f each err by a few ULP; through tonemap's steepest slope, about 8.3, times 255 that is under 0.01 code, so
the two sides differ only where a value sits on a rounding boundary: tests/test_shade_cpu.py moves the restatement's results by 2 ULP and
stays inside both conditions).  Outputs are poisoned before every launch and carry a tail that must keep its bytes."""
import numpy as np
import pytest

import oracle
import shade_cases as SC
import shade_ref as SR
import visattr_ref as VA
from niagara_amd import layouts as L
from niagara_amd import synth

SIZES = [(1, 1), (7, 5), (21, 3), (3, 21), (67, 37), (65, 5), (65, 17)]  # (65, 5) / (65, 17): the blur kernels' tiles (64 x 4, 64 x 16) + 1
POISON = 0x5A
TAIL = 64  # bytes behind every output


@pytest.fixture(scope="session")
def sref(tmp_path_factory):
    return SR.load(tmp_path_factory.mktemp("shade_ref_gpu"))


@pytest.fixture(scope="module")
def ctx():
    from niagara_amd import pipeline as P
    c = P.Context()
    yield c
    c.close()


def _dev(ctx, arr, tail=0):
    """the bytes of `arr` on the device, followed by `tail` poison bytes"""
    import torch
    a = np.ascontiguousarray(arr)
    t = torch.full((a.nbytes + tail,), POISON, dtype=torch.uint8, device=ctx.device)
    t[:a.nbytes] = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(ctx.device)
    return t


def _out(ctx, nbytes):
    import torch
    return torch.full((nbytes + TAIL,), POISON, dtype=torch.uint8, device=ctx.device)


def _host(t, nbytes, dtype, shape):
    a = t.cpu().numpy()
    assert (a[nbytes:] == POISON).all(), "bytes behind the image were written"
    return a[:nbytes].view(dtype).reshape(shape)


def _close(name, got, want, alpha=False):
    """the issue's comparison of 8-bit channels; prints the counts before it asserts"""
    g, r = got.astype(np.int64), want.astype(np.int64)
    d = np.abs(g - r)
    print("%s: %d channels, %d differ, largest difference %d" % (name, d.size, int((d != 0).sum()), int(d.max())))
    assert d.max() <= 1
    assert (d == 0).mean() >= 0.9
    if alpha:
        assert (g[..., 3] == 255).all()


@pytest.mark.gpu
@pytest.mark.parametrize("checkerboard", [0, 1])
@pytest.mark.parametrize("size", SIZES)
def test_shadow_fill_equals_the_restatement(size, checkerboard, ctx, sref):
    w, h = size
    i = SR.test_inputs(w, h)
    want = sref.shadow_fill(i["shadow"], i["depth"], checkerboard)
    shadow, depth = _dev(ctx, i["shadow"], TAIL), _dev(ctx, i["depth"])
    ctx.shadow_fill(shadow, depth, w, h, checkerboard)
    ctx.status()
    got = _host(shadow, w * h, np.uint8, (h, w))
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    owned = (~(y ^ checkerboard) & 1) == (x & 1)
    assert (got[~owned] == i["shadow"][~owned]).all()  # the other parity keeps its bytes exactly
    assert (want[~owned] == i["shadow"][~owned]).all()
    if owned.any():
        _close("fill %dx%d cb %d" % (w, h, checkerboard), got[owned], want[owned])


@pytest.mark.gpu
@pytest.mark.parametrize("direction", [1, 0])
@pytest.mark.parametrize("size", SIZES)
def test_shadow_blur_equals_the_restatement(size, direction, ctx, sref):
    w, h = size
    i = SR.test_inputs(w, h)
    want = sref.shadow_blur(i["shadow"], i["depth"], direction, i["znear"])
    shadow, depth, out = _dev(ctx, i["shadow"]), _dev(ctx, i["depth"]), _out(ctx, w * h)
    ctx.shadow_blur(out, shadow, depth, w, h, direction, i["znear"])
    ctx.status()
    _close("blur %dx%d direction %d" % (w, h, direction), _host(out, w * h, np.uint8, (h, w)), want)
    assert shadow.cpu().numpy().tobytes() == i["shadow"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("shadows", [0, 1])
@pytest.mark.parametrize("size", SIZES)
def test_shade_final_equals_the_restatement(size, shadows, ctx, sref):
    w, h = size
    i = SR.test_inputs(w, h)
    sd = SR.test_shade_data(w, h, shadows)
    want = sref.shade_final(sd, i["gbuffer0"], i["gbuffer1"], i["depth"], i["shadow"] if shadows else None)
    g0, g1, depth, out = _dev(ctx, i["gbuffer0"]), _dev(ctx, i["gbuffer1"]), _dev(ctx, i["depth"]), _out(ctx, w * h * 4)
    shadow = _dev(ctx, i["shadow"]) if shadows else None  # shadows off: the image is never read, so none is given
    ctx.shade_final(sd, g0, g1, depth, shadow, out, w, h)
    ctx.status()
    _close("final %dx%d shadows %d" % (w, h, shadows), SR.channels(_host(out, w * h * 4, np.uint32, (h, w))), SR.channels(want), alpha=True)


@pytest.mark.gpu
@pytest.mark.parametrize("path", SC.FIXTURES, ids=SC.FIXTURE_IDS)
def test_fixtures_of_the_reference_shaders_replay(path, ctx):
    """tests/golden/shade: the inputs and what the reference's own shadowfill / shadowblur / final, run on the CPU, stored for them (DESIGN.md
    §2).  tests/test_shade_fixtures_cpu.py holds the restatement to these words bit for bit, so the comparison and its bounds are the ones
    above, unchanged."""
    f = np.load(path)
    w, h = SC.fixture_size(f)
    name = "fixture %dx%d" % (w, h)
    depth = _dev(ctx, f["depth"])
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    for cb in (0, 1):
        shadow = _dev(ctx, f["shadow"], TAIL)
        ctx.shadow_fill(shadow, depth, w, h, cb)
        ctx.status()
        got, owned = _host(shadow, w * h, np.uint8, (h, w)), (~(y ^ cb) & 1) == (x & 1)
        assert (got[~owned] == f["shadow"][~owned]).all()
        _close("%s, fill cb %d" % (name, cb), got[owned], f["fill%d_words" % cb][owned])
    for direction in (1, 0):
        shadow, out = _dev(ctx, f["shadow"]), _out(ctx, w * h)
        ctx.shadow_blur(out, shadow, depth, w, h, direction, float(f["znear"]))
        ctx.status()
        _close("%s, blur direction %d" % (name, direction), _host(out, w * h, np.uint8, (h, w)), f["blur%d_words" % direction])
    g0, g1 = _dev(ctx, f["gbuffer0"]), _dev(ctx, f["gbuffer1"])
    for shadows in (0, 1):
        out, shadow = _out(ctx, w * h * 4), _dev(ctx, f["shadow"]) if shadows else None
        ctx.shade_final(SC.fixture_shade_data(f, shadows), g0, g1, depth, shadow, out, w, h)
        ctx.status()
        _close("%s, final shadows %d" % (name, shadows), SR.channels(_host(out, w * h * 4, np.uint32, (h, w))), SR.channels(f["final%d_words" % shadows]), alpha=True)


@pytest.mark.gpu
def test_bad_arguments_are_refused_and_write_nothing(ctx, sref):
    import torch
    from niagara_amd._lib import NvError
    w, h = 21, 3
    i = SR.test_inputs(w, h)
    sd = SR.test_shade_data(w, h, 1)
    g0, g1, depth, shadow = _dev(ctx, i["gbuffer0"], 8), _dev(ctx, i["gbuffer1"], 8), _dev(ctx, i["depth"], 8), _dev(ctx, i["shadow"], TAIL)
    out8, out32 = _out(ctx, w * h), _out(ctx, w * h * 4 + 8)
    fill = lambda **k: ctx.shadow_fill(**{**dict(shadow=shadow, depth=depth, width=w, height=h, checkerboard=1), **k})
    blur = lambda **k: ctx.shadow_blur(**{**dict(out=out8, shadow=shadow, depth=depth, width=w, height=h, direction=1, znear=0.1), **k})
    final = lambda **k: ctx.shade_final(**{**dict(shade_data=sd, gbuffer0=g0, gbuffer1=g1, depth=depth, shadow=shadow, color=out32, width=w, height=h), **k})
    wrong = sd.copy()
    wrong["imageSize"][0] = (w + 1, h)
    bad = [(fill, dict(shadow=None)), (fill, dict(depth=None)), (fill, dict(width=0)), (fill, dict(height=0)), (fill, dict(width=16385)),
           (fill, dict(height=16385)), (fill, dict(depth=depth[1:])),
           (blur, dict(out=None)), (blur, dict(shadow=None)), (blur, dict(depth=None)), (blur, dict(out=shadow)), (blur, dict(width=0)),
           (blur, dict(height=16385)), (blur, dict(depth=depth[2:])), (blur, dict(direction=2)),
           (final, dict(gbuffer0=None)), (final, dict(gbuffer1=None)), (final, dict(depth=None)), (final, dict(color=None)), (final, dict(shadow=None)),
           (final, dict(width=0)), (final, dict(height=0)), (final, dict(width=16385)), (final, dict(shade_data=wrong)), (final, dict(width=w + 1)),
           (final, dict(gbuffer0=g0[1:])), (final, dict(gbuffer1=g1[2:])), (final, dict(depth=depth[3:])), (final, dict(color=out32[1:]))]
    for fn, kw in bad:
        with pytest.raises(NvError):
            fn(**kw)
    ctx.status()
    assert (out8 == POISON).all() and (out32 == POISON).all()
    assert shadow.cpu().numpy()[:w * h].tobytes() == i["shadow"].tobytes()
    # a NULL context
    from niagara_amd import _lib
    assert _lib.lib.nv_shadow_fill(None, None, shadow.data_ptr(), depth.data_ptr(), w, h, 0) == -1
    # shadows off: no shadow image needed
    off = sd.copy()
    off["shadowsEnabled"] = 0
    final(shade_data=off, shadow=None)
    ctx.status()
    want = sref.shade_final(off, i["gbuffer0"], i["gbuffer1"], i["depth"])
    _close("final without a shadow image", SR.channels(out32.cpu().numpy()[:w * h * 4].view(np.uint32).reshape(h, w)), SR.channels(want), alpha=True)
    del torch


@pytest.mark.gpu
def test_the_chain_replays_from_a_captured_graph(ctx, sref):
    """fill -> blur horizontal -> blur vertical -> final, a linear chain: two replays give the bytes of the eager run"""
    import torch
    w, h = 67, 37
    i = SR.test_inputs(w, h)
    sd = SR.test_shade_data(w, h, 1)
    g0, g1, depth = _dev(ctx, i["gbuffer0"]), _dev(ctx, i["gbuffer1"]), _dev(ctx, i["depth"])
    source = _dev(ctx, i["shadow"])
    shadow, tmp, out = _out(ctx, w * h), _out(ctx, w * h), _out(ctx, w * h * 4)

    def reset():
        tmp.fill_(POISON), out.fill_(POISON), shadow.fill_(POISON)
        shadow[:w * h] = source

    def chain():
        ctx.shadow_fill(shadow, depth, w, h, 1)
        ctx.shadow_blur(tmp, shadow, depth, w, h, 1, i["znear"])
        ctx.shadow_blur(shadow, tmp, depth, w, h, 0, i["znear"])
        ctx.shade_final(sd, g0, g1, depth, shadow, out, w, h)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        reset()
        chain()
        torch.cuda.synchronize()
        eager = [t.cpu().numpy().copy() for t in (shadow, tmp, out)]
        want = sref.shade(sd, i["gbuffer0"], i["gbuffer1"], i["depth"], i["shadow"], blur=True, checkerboard=True, znear=i["znear"])
        d = np.abs(SR.channels(eager[2][:w * h * 4].view(np.uint32).reshape(h, w)) - SR.channels(want))
        print("chain: %d channels, %d differ, largest difference %d" % (d.size, int((d != 0).sum()), int(d.max())))
        assert d.max() <= 2  # the second blur reads the first's quantised output: one code may carry
        reset()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            chain()
        torch.cuda.synchronize()
        assert (out == POISON).all()  # nothing ran during capture
        for _ in range(2):
            reset()
            graph.replay()
            torch.cuda.synchronize()
            for t, e in zip((shadow, tmp, out), eager):
                assert t.cpu().numpy().tobytes() == e.tobytes()
    ctx.status()


@pytest.mark.gpu
def test_the_occluder_frame_shades_end_to_end(sref):
    """frame(visibility=) -> resolve -> attributes -> shade with a synthetic shadow mask, against the restatement chained the same way on the
    G-buffer words and the depth target the GPU passes left: within two codes (the second blur reads the first's quantised output, so one
    code may carry), alpha 255; and shadows off; sky and geometry both present"""
    import torch
    from niagara_amd import pipeline as P
    s = VA.with_attributes(synth.occluder_scene(meshlet_bounds=oracle.meshlet_bounds))
    w, h = s["viewport"]
    pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], task_capacity=4096, cluster_capacity=4096 * 64, fused=True,
                                vertices=s["vertices"], meshlet_data=s["data"], stable_ids=True)
    try:
        vis = pipe.new_visibility()
        for _ in range(2):
            pipe.frame(s["cull"], post_pass=True, visibility=vis)
        res = pipe.resolve(s["cull"], vis)
        att = pipe.attributes(s["cull"], res["records"], s["materials"], attributes=False)
        x, y = np.meshgrid(np.arange(w), np.arange(h))
        r = np.hypot(x - 0.45 * w, y - 0.5 * h) / (0.3 * h)
        mask = np.clip(np.rint(255.0 * np.clip((r - 0.8) / 0.4, 0.0, 1.0)), 0, 255).astype(np.uint8)
        camera, sun = (0.0, 0.0, 0.0), np.array([0.35, 0.6, 0.72]) / np.linalg.norm([0.35, 0.6, 0.72])
        g0, g1 = (att[k].cpu().numpy().view(np.uint32) for k in ("gbuffer0", "gbuffer1"))
        depth = pipe.depth.cpu().numpy()
        sky, geometry = int((depth == 0).sum()), int((depth > 0).sum())
        print("frame: %d sky pixels, %d geometry pixels" % (sky, geometry))
        assert sky > 1000 and geometry > 1000 and (g0[depth > 0] != 0).any()
        from niagara_amd import host
        znear = float(s["cull"]["znear"][0])
        for name, kw in (("shadows, blur", dict(shadow=mask, blur=True, checkerboard=False)), ("shadows, fill and blur", dict(shadow=mask, blur=True, checkerboard=True)),
                         ("no shadows", dict(shadow=None))):
            dev_mask = None if kw["shadow"] is None else torch.from_numpy(mask.copy()).to(pipe.ctx.device)
            color = pipe.shade(s["cull"], att["gbuffer0"], att["gbuffer1"], camera, sun, **{**kw, "shadow": dev_mask})
            pipe.ctx.status()
            sd = host.build_shade_data(synth.make_globals(s["cull"], (w, h)), camera, sun, 0 if kw["shadow"] is None else 1, w, h)
            want = sref.shade(sd, g0, g1, depth, znear=znear, **kw)
            got = SR.channels(color.cpu().numpy().view(np.uint32))
            d = np.abs(got - SR.channels(want))
            print("%s: %d channels, %d differ, largest difference %d" % (name, d.size, int((d != 0).sum()), int(d.max())))
            assert d.max() <= 2 and (got[..., 3] == 255).all()
            assert (got[..., :3][depth == 0] == 0).all() and (got[..., :3][depth > 0] > 0).any()
        assert (pipe.depth.cpu().numpy() == depth).all()
    finally:
        pipe.ctx.close()
    assert L.SHADEDATA.itemsize == 112
