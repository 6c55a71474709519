"""Bloom on the MI355X against the fp32 build of tests/bloom_ref.c on the same input bytes.

Passes 1 and 2 are additions and multiplications only: bit-identical words, level by level, on given words with denormal codes, sums past
the format's maximum and inf / NaN codes.  Pass 0 goes through pow and exp2: every channel the same code or the adjacent one and at least 99 %
equal (a condition: tests/test_bloom_cpu.py moves the restatement's pow / exp2 by 2 ULP on these inputs and stays inside).  nv_bloom: level 0
as pass 0, every other level bit-identical to the restatement's passes run from the device's own level 0.  nv_shade_final_bloom: §4.14's
comparison.  Inputs and outputs are poisoned; every output carries a 64-byte tail that must keep its bytes."""
import numpy as np
import pytest

import bloom_ref as BR
import oracle
import shade_cases as SC
import shade_ref as SR
import visattr_ref as VA
from niagara_amd import host, synth

# (67, 37): level 1 is 17 x 9, one more than the 16-texel tile of passes 1 and 2 along x; (67, 67): 17 x 17, along both
SIZES = [(1, 1), (2, 2), (7, 5), (33, 3), (67, 37), (511, 9), (67, 67)]
POISON = 0x5A
TAIL = 64


@pytest.fixture(scope="session")
def bref(tmp_path_factory):
    return BR.load(tmp_path_factory.mktemp("bloom_ref_gpu"))


@pytest.fixture(scope="session")
def sref(tmp_path_factory):
    return SR.load(tmp_path_factory.mktemp("shade_ref_bloom_gpu"))


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


def _host(t, nbytes, dtype=np.uint32):
    a = t.cpu().numpy()
    assert (a[nbytes:] == POISON).all(), "bytes behind the buffer were written"
    return a[:nbytes].view(dtype)


def _adjacent(name, got, want):
    """pass 0's comparison of UFLOAT codes; prints the counts before it asserts"""
    d = np.abs(BR.codes(got) - BR.codes(want))
    print("%s: %d channels, %d differ, largest difference %d" % (name, d.size, int((d != 0).sum()), int(d.max())))
    assert d.max() <= 1
    assert (d == 0).mean() >= 0.99


def _close8(name, got, want):
    """§4.14's comparison of 8-bit channels"""
    g, r = SR.channels(got), SR.channels(want)
    d = np.abs(g - r)
    print("%s: %d channels, %d differ, largest difference %d" % (name, d.size, int((d != 0).sum()), int(d.max())))
    assert d.max() <= 1
    assert (d == 0).mean() >= 0.9
    assert (g[..., 3] == 255).all()


def _poison_words(d):
    return np.full(d["total"], POISON * 0x01010101, np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_extract_equals_the_restatement(size, ctx, bref):
    w, h = size
    d, desc = BR.desc(w, h), host.bloom_desc(w, h)
    g0 = BR.test_gbuffer0(w, h)
    want = bref.extract(g0)
    src, out = _dev(ctx, g0), _out(ctx, d["total"] * 4)
    ctx.bloom_extract(src, w, h, out, desc)
    ctx.status()
    got = _host(out, d["total"] * 4)
    n0 = d["sizes"][0][0] * d["sizes"][0][1]
    assert (got[n0:] == POISON * 0x01010101).all()  # the other levels keep their bytes
    _adjacent("extract %dx%d" % (w, h), got[:n0].reshape(want.shape), want)
    assert src.cpu().numpy().tobytes() == g0.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_downsample_is_bit_identical_level_by_level(size, ctx, bref):
    w, h = size
    d, desc = BR.desc(w, h), host.bloom_desc(w, h)
    given = BR.test_levels(w, h)
    for level in range(1, d["levels"]):
        buf = _dev(ctx, BR.pack(given), TAIL)
        ctx.bloom_downsample(buf, desc, level)
        ctx.status()
        got = BR.unpack(_host(buf, d["total"] * 4), d)
        want = bref.downsample(given[level - 1])
        assert got[level].tobytes() == want.tobytes(), (size, level, int((got[level] != want).sum()))
        for i in range(d["levels"]):
            assert i == level or got[i].tobytes() == given[i].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("radius", [2.0, 0.0, 1.25, 5.5])  # 5.5: past the staged form's radius, the direct form
@pytest.mark.parametrize("size", SIZES)
def test_upsample_is_bit_identical_level_by_level(size, radius, ctx, bref):
    w, h = size
    d, desc = BR.desc(w, h), host.bloom_desc(w, h)
    given = BR.test_levels(w, h, seed=2)
    for level in range(d["levels"] - 1):
        buf = _dev(ctx, BR.pack(given), TAIL)
        ctx.bloom_upsample(buf, desc, level, radius)
        ctx.status()
        got = BR.unpack(_host(buf, d["total"] * 4), d)
        want = bref.upsample(given[level + 1], given[level], radius)
        assert got[level].tobytes() == want.tobytes(), (size, level, int((got[level] != want).sum()))
        for i in range(d["levels"]):
            assert i == level or got[i].tobytes() == given[i].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_the_chain_equals_the_single_passes_and_the_restatement(size, ctx, bref):
    """nv_bloom against (a) the single-pass entry points called in the reference's order on another buffer: the same words; (b) the
    restatement: the device's level 0 after pass 0 alone compared as pass 0 is, every level of the finished chain bit-identical to the
    restatement's passes 1 and 2 run from that level 0"""
    w, h = size
    d, desc = BR.desc(w, h), host.bloom_desc(w, h)
    g0 = BR.test_gbuffer0(w, h)
    src, chain, single = _dev(ctx, g0), _out(ctx, d["total"] * 4), _out(ctx, d["total"] * 4)
    ctx.bloom(src, w, h, chain, desc)
    ctx.bloom_extract(src, w, h, single, desc)
    ctx.status()
    n0 = d["sizes"][0][0] * d["sizes"][0][1]
    level0 = _host(single, d["total"] * 4)[:n0].reshape(d["sizes"][0][1], d["sizes"][0][0]).copy()
    _adjacent("chain %dx%d, level 0 after pass 0" % (w, h), level0, bref.extract(g0))
    for i in range(1, d["levels"]):
        ctx.bloom_downsample(single, desc, i)
    for i in range(d["levels"] - 2, -1, -1):
        ctx.bloom_upsample(single, desc, i, 2.0)
    ctx.status()
    got = _host(chain, d["total"] * 4)
    assert got.tobytes() == _host(single, d["total"] * 4).tobytes()
    want = bref.chain_from(level0, d["levels"])
    for i, (a, b) in enumerate(zip(BR.unpack(got, d), want)):
        assert a.tobytes() == b.tobytes(), (size, i, int((a != b).sum()))


# (67, 37): the fused tail holds the whole chain (first level 0); (300, 200): level 0 has 15000 texels, levels 1-7 have 4960 together (first
# level 1: seven levels in one launch); (511, 9): 1280 texels at level 0, all eight levels; (1, 1) and (2, 2): one level, nothing to fuse
@pytest.mark.gpu
@pytest.mark.parametrize("size", [(67, 37), (300, 200), (511, 9), (7, 5), (2, 2)])
def test_the_fused_tail_writes_the_per_level_words(size, ctx, bref):
    """nv_bloom with NV_OPT_BLOOM_FUSED_TAIL 1 against the per-level entry points on the same input: the same words at every level, and the
    levels behind level 0 bit-identical to the restatement run from the device's level 0"""
    from niagara_amd import pipeline as P
    w, h = size
    d, desc = BR.desc(w, h), host.bloom_desc(w, h)
    g0 = BR.test_gbuffer0(w, h)
    src, fused, single = _dev(ctx, g0), _out(ctx, d["total"] * 4), _out(ctx, d["total"] * 4)
    ctx.set_option(P.NV_OPT_BLOOM_FUSED_TAIL, 1)
    try:
        ctx.bloom(src, w, h, fused, desc)
    finally:
        ctx.set_option(P.NV_OPT_BLOOM_FUSED_TAIL, 0)
    ctx.bloom_extract(src, w, h, single, desc)
    ctx.status()
    n0 = d["sizes"][0][0] * d["sizes"][0][1]
    level0 = _host(single, d["total"] * 4)[:n0].reshape(d["sizes"][0][1], d["sizes"][0][0]).copy()
    for i in range(1, d["levels"]):
        ctx.bloom_downsample(single, desc, i)
    for i in range(d["levels"] - 2, -1, -1):
        ctx.bloom_upsample(single, desc, i, 2.0)
    ctx.status()
    got = _host(fused, d["total"] * 4)
    want = _host(single, d["total"] * 4)
    for i, (a, b) in enumerate(zip(BR.unpack(got, d), BR.unpack(want, d))):
        assert a.tobytes() == b.tobytes(), (size, i, int((a != b).sum()))
    for i, (a, b) in enumerate(zip(BR.unpack(got, d), bref.chain_from(level0, d["levels"]))):
        assert a.tobytes() == b.tobytes(), (size, i, int((a != b).sum()))
    from niagara_amd._lib import NvError
    for bad in (2, -1):
        with pytest.raises(NvError):
            ctx.set_option(P.NV_OPT_BLOOM_FUSED_TAIL, bad)


@pytest.mark.gpu
def test_bloom_changes_final_only_within_the_reach_of_the_chain(ctx):
    """An emitter in the leftmost 16 columns of an 8192 x 16 image (bloom target 4096 x 8, eight levels, the last 32 x 1): final with bloom
    differs from final without it only within the chain's reach.  The reach in pixels: pass 0 and final's own bilinear fetch 4 each; pass 1
    into level i reads within two texels of level i (one for the tap, one for the footprint), 2 * 2^(i + 1) pixels, i = 1 .. 7: 1016; pass 2
    into level i reads within two texels of level i + 1 (radius 2 is one texel of the source, one for the footprint), i = 0 .. 6: 1016"""
    w, h, lit = 8192, 16, 16
    reach = 4 + 1016 + 1016 + 4
    desc = host.bloom_desc(w, h)
    assert desc.levels == 8 and (desc.width >> 7, max(1, desc.height >> 7)) == (32, 1)
    rng = np.random.default_rng(4)
    g0 = (rng.integers(0, 1 << 24, (h, w), dtype=np.uint64).astype(np.uint32) | np.uint32(0x00404040))  # albedo, no emission
    g0[:, :lit] |= np.uint32(0xFF000000)
    g1 = rng.integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)
    depth = np.full((h, w), 0.02, np.float32)
    sd = SR.test_shade_data(w, h, 0)
    dg0, dg1, dd = _dev(ctx, g0), _dev(ctx, g1), _dev(ctx, depth)
    bloom, plain, lit_out = _out(ctx, desc.totalTexels * 4), _out(ctx, w * h * 4), _out(ctx, w * h * 4)
    ctx.bloom(dg0, w, h, bloom, desc)
    ctx.shade_final(sd, dg0, dg1, dd, None, plain, w, h)
    ctx.shade_final_bloom(sd, dg0, dg1, dd, None, lit_out, w, h, bloom, desc)
    ctx.status()
    a, b = _host(plain, w * h * 4).reshape(h, w), _host(lit_out, w * h * 4).reshape(h, w)
    changed = a != b
    cols = np.nonzero(changed.any(axis=0))[0]
    print("reach: columns %d .. %d changed, bound %d" % (int(cols.min()), int(cols.max()), lit + reach))
    assert changed[:, lit:lit + 64].any()  # light reaches pixels that emit nothing
    assert cols.max() < lit + reach
    assert not changed[:, lit + reach:].any()


@pytest.mark.gpu
def test_the_chain_replays_from_a_captured_graph(ctx, bref):
    import torch
    w, h = 67, 37
    d, desc = BR.desc(w, h), host.bloom_desc(w, h)
    src, out = _dev(ctx, BR.test_gbuffer0(w, h)), _out(ctx, d["total"] * 4)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx.bloom(src, w, h, out, desc)
        torch.cuda.synchronize()
        eager = out.cpu().numpy().copy()
        assert (eager[:d["total"] * 4] != POISON).any()
        out.fill_(POISON)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            ctx.bloom(src, w, h, out, desc)
        torch.cuda.synchronize()
        assert (out == POISON).all()  # nothing ran during capture
        for _ in range(2):
            out.fill_(POISON)
            graph.replay()
            torch.cuda.synchronize()
            assert out.cpu().numpy().tobytes() == eager.tobytes()
    ctx.status()


def bloom0_input(w, h):
    """tests/test_bloom_cpu.py's: level 0 of the bloom target given to final (moderate values, zeros, denormals, two inf and two NaN codes)"""
    return BR.test_levels(w, h, seed=1, top=17)[0]


bloom0_input.__test__ = False


@pytest.mark.gpu
@pytest.mark.parametrize("shadows", [0, 1])
@pytest.mark.parametrize("size", SIZES)
def test_shade_final_bloom_equals_the_restatement(size, shadows, ctx, bref):
    w, h = size
    d, desc = BR.desc(w, h), host.bloom_desc(w, h)
    i = SR.test_inputs(w, h)
    sd = SR.test_shade_data(w, h, shadows)
    words = _poison_words(d)
    b0 = bloom0_input(w, h)
    words[:b0.size] = b0.reshape(-1)
    want = bref.shade_final_bloom(sd, i["gbuffer0"], i["gbuffer1"], i["depth"], i["shadow"] if shadows else None, b0)
    g0, g1, depth, out, bloom = _dev(ctx, i["gbuffer0"]), _dev(ctx, i["gbuffer1"]), _dev(ctx, i["depth"]), _out(ctx, w * h * 4), _dev(ctx, words)
    shadow = _dev(ctx, i["shadow"]) if shadows else None
    ctx.shade_final_bloom(sd, g0, g1, depth, shadow, out, w, h, bloom, desc)
    ctx.status()
    _close8("final with bloom %dx%d shadows %d" % (w, h, shadows), _host(out, w * h * 4).reshape(h, w), want)
    assert bloom.cpu().numpy().tobytes() == words.tobytes()
    # an all-zero bloom image: nv_shade_final's colour, byte for byte
    zero, plain, with_zero = _dev(ctx, np.zeros(d["total"], np.uint32)), _out(ctx, w * h * 4), _out(ctx, w * h * 4)
    ctx.shade_final(sd, g0, g1, depth, shadow, plain, w, h)
    ctx.shade_final_bloom(sd, g0, g1, depth, shadow, with_zero, w, h, zero, desc)
    ctx.status()
    assert _host(plain, w * h * 4).tobytes() == _host(with_zero, w * h * 4).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("path", SC.FIXTURES, ids=SC.FIXTURE_IDS)
def test_fixtures_of_the_reference_shader_replay(path, ctx, bref):
    """tests/golden/shade: the inputs and what the reference's own bloom.comp.glsl and final.comp.glsl, run on the CPU, stored for them (DESIGN.md
    §2; tests/test_shade_fixtures_cpu.py holds the restatement to these words bit for bit).  The rules are this file's, unchanged: pass 0
    adjacent codes, passes 1 and 2 bit-identical, nv_bloom as pass 0 at level 0 and bit-identical from there, final as §4.14."""
    f = np.load(path)
    w, h = SC.fixture_size(f)
    d, desc = BR.desc(w, h), host.bloom_desc(w, h)
    name = "fixture %dx%d" % (w, h)
    n0 = d["sizes"][0][0] * d["sizes"][0][1]
    src, out = _dev(ctx, f["bloom_g0"]), _out(ctx, d["total"] * 4)
    ctx.bloom_extract(src, w, h, out, desc)
    ctx.status()
    got = _host(out, d["total"] * 4)
    assert (got[n0:] == POISON * 0x01010101).all()
    level0 = got[:n0].reshape(f["extract_words"].shape).copy()
    _adjacent(name + ", extract", level0, f["extract_words"])
    for level in range(1, d["levels"]):  # pass 1, each level from the given words
        buf = _dev(ctx, f["levels"], TAIL)
        ctx.bloom_downsample(buf, desc, level)
        ctx.status()
        got, want = BR.unpack(_host(buf, d["total"] * 4), d), BR.unpack(f["down_words"], d)
        assert got[level].tobytes() == want[level].tobytes(), (name, "downsample", level, int((got[level] != want[level]).sum()))
    for k, radius in enumerate(SC.RADII):  # pass 2, the staged form and the direct one
        for level in range(d["levels"] - 1):
            buf = _dev(ctx, f["levels2"], TAIL)
            ctx.bloom_upsample(buf, desc, level, radius)
            ctx.status()
            got, want = BR.unpack(_host(buf, d["total"] * 4), d), BR.unpack(f["up%d_words" % k], d)
            assert got[level].tobytes() == want[level].tobytes(), (name, "upsample", radius, level, int((got[level] != want[level]).sum()))
    # the loop: from the reference's level 0 the single passes give the reference's words; nv_bloom gives what they give from its own level 0
    words = _poison_words(d)
    words[:n0] = f["extract_words"].reshape(-1)
    single, chain = _dev(ctx, words, TAIL), _out(ctx, d["total"] * 4)
    for i in range(1, d["levels"]):
        ctx.bloom_downsample(single, desc, i)
    for i in range(d["levels"] - 2, -1, -1):
        ctx.bloom_upsample(single, desc, i, 2.0)
    ctx.bloom(src, w, h, chain, desc)
    ctx.status()
    assert _host(single, d["total"] * 4).tobytes() == f["loop_words"].tobytes()
    assert _host(chain, d["total"] * 4).tobytes() == BR.pack(bref.chain_from(level0, d["levels"])).tobytes()
    # final with the fixture's bloom image
    g0, g1, depth = _dev(ctx, f["gbuffer0"]), _dev(ctx, f["gbuffer1"]), _dev(ctx, f["depth"])
    words = _poison_words(d)
    words[:n0] = f["bloom0"].reshape(-1)
    bloom = _dev(ctx, words)
    for shadows in (0, 1):
        out, shadow = _out(ctx, w * h * 4), _dev(ctx, f["shadow"]) if shadows else None
        ctx.shade_final_bloom(SC.fixture_shade_data(f, shadows), g0, g1, depth, shadow, out, w, h, bloom, desc)
        ctx.status()
        _close8("%s, final with bloom, shadows %d" % (name, shadows), _host(out, w * h * 4).reshape(h, w), f["finalbloom%d_words" % shadows])


@pytest.mark.gpu
def test_bad_arguments_are_refused_and_write_nothing(ctx):
    import ctypes as C

    from niagara_amd import _lib
    from niagara_amd._lib import NvError
    w, h = 21, 7
    d, desc = BR.desc(w, h), host.bloom_desc(w, h)
    i = SR.test_inputs(w, h)
    sd = SR.test_shade_data(w, h, 1)
    g0, g1, depth, shadow = _dev(ctx, i["gbuffer0"], 8), _dev(ctx, i["gbuffer1"], 8), _dev(ctx, i["depth"], 8), _dev(ctx, i["shadow"])
    bloom, color = _out(ctx, d["total"] * 4 + 8), _out(ctx, w * h * 4 + 8)
    other = host.bloom_desc(w + 2, h)  # a valid desc of another image
    broken = host.bloom_desc(w, h)
    broken.levelOffset[1] += 1
    capped = host.bloom_desc(w, h)
    capped.levels -= 1
    wrong_sd = sd.copy()
    wrong_sd["imageSize"][0] = (w + 1, h)
    extract = lambda **k: ctx.bloom_extract(**{**dict(gbuffer0=g0, width=w, height=h, bloom=bloom, desc=desc), **k})
    chain = lambda **k: ctx.bloom(**{**dict(gbuffer0=g0, width=w, height=h, bloom=bloom, desc=desc), **k})
    down = lambda **k: ctx.bloom_downsample(**{**dict(bloom=bloom, desc=desc, level=1), **k})
    up = lambda **k: ctx.bloom_upsample(**{**dict(bloom=bloom, desc=desc, level=0, radius=2.0), **k})
    final = lambda **k: ctx.shade_final_bloom(**{**dict(shade_data=sd, gbuffer0=g0, gbuffer1=g1, depth=depth, shadow=shadow, color=color, width=w, height=h,
                                                        bloom=bloom, desc=desc), **k})
    bad = []
    for fn in (extract, chain):
        bad += [(fn, dict(gbuffer0=None)), (fn, dict(bloom=None)), (fn, dict(desc=None)), (fn, dict(width=0)), (fn, dict(height=0)), (fn, dict(width=16385)),
                (fn, dict(height=16385)), (fn, dict(gbuffer0=g0[1:])), (fn, dict(bloom=bloom[2:])), (fn, dict(desc=other)), (fn, dict(desc=broken)),
                (fn, dict(desc=capped)), (fn, dict(width=w + 2))]
    bad += [(down, dict(bloom=None)), (down, dict(desc=None)), (down, dict(level=0)), (down, dict(level=desc.levels)), (down, dict(level=0xFFFFFFFF)),
            (down, dict(bloom=bloom[1:])), (down, dict(desc=broken)), (down, dict(desc=capped)),
            (up, dict(bloom=None)), (up, dict(desc=None)), (up, dict(level=desc.levels - 1)), (up, dict(level=0xFFFFFFFF)), (up, dict(bloom=bloom[3:])),
            (up, dict(desc=broken)), (up, dict(radius=-1.0)), (up, dict(radius=-0.5)), (up, dict(radius=float("inf"))), (up, dict(radius=float("nan"))),
            (final, dict(gbuffer0=None)), (final, dict(gbuffer1=None)), (final, dict(depth=None)), (final, dict(color=None)), (final, dict(shadow=None)),
            (final, dict(bloom=None)), (final, dict(desc=None)), (final, dict(desc=other)), (final, dict(desc=broken)), (final, dict(width=0)),
            (final, dict(height=16385)), (final, dict(shade_data=wrong_sd)), (final, dict(width=w + 1)), (final, dict(gbuffer0=g0[1:])),
            (final, dict(color=color[1:])), (final, dict(bloom=bloom[1:]))]
    for fn, kw in bad:
        with pytest.raises(NvError):
            fn(**kw)
    ctx.status()
    assert (bloom == POISON).all() and (color == POISON).all()
    assert _lib.lib.nv_bloom(None, None, g0.data_ptr(), w, h, bloom.data_ptr(), C.byref(desc)) == -1  # a NULL context
    single = host.bloom_desc(1, 1)  # one level: neither per-level pass has a level to run
    assert single.levels == 1
    for fn, kw in ((down, dict(desc=single, level=1)), (down, dict(desc=single, level=0)), (up, dict(desc=single, level=0))):
        with pytest.raises(NvError):
            fn(**kw)
    ctx.status()
    assert (bloom == POISON).all()


@pytest.mark.gpu
def test_the_pipeline_shades_with_and_without_bloom():
    """synth.occluder_scene with one emissive material through VisibilityPipeline.shade: bloom=False is the existing result (nv_shade_final on
    the same inputs, byte for byte); bloom=True differs from it, also at pixels that emit nothing, and only adds light"""
    import torch
    from niagara_amd import pipeline as P
    s = VA.with_attributes(synth.occluder_scene(meshlet_bounds=oracle.meshlet_bounds))
    s["materials"] = s["materials"].copy()
    s["materials"]["emissiveFactor"] = 0.0
    s["materials"]["emissiveFactor"][1] = (4.0, 1.5, 0.25)
    w, h = s["viewport"]
    pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], task_capacity=4096, cluster_capacity=4096 * 64, fused=True,
                                vertices=s["vertices"], meshlet_data=s["data"], stable_ids=True)
    try:
        vis = pipe.new_visibility()
        for _ in range(2):
            pipe.frame(s["cull"], post_pass=True, visibility=vis)
        res = pipe.resolve(s["cull"], vis)
        att = pipe.attributes(s["cull"], res["records"], s["materials"], attributes=False)
        camera, sun = (0.0, 0.0, 0.0), np.array([0.35, 0.6, 0.72]) / np.linalg.norm([0.35, 0.6, 0.72])
        off = pipe.shade(s["cull"], att["gbuffer0"], att["gbuffer1"], camera, sun).cpu().numpy().view(np.uint32)
        default = pipe.shade(s["cull"], att["gbuffer0"], att["gbuffer1"], camera, sun, bloom=False).cpu().numpy().view(np.uint32)
        on = pipe.shade(s["cull"], att["gbuffer0"], att["gbuffer1"], camera, sun, bloom=True).cpu().numpy().view(np.uint32)
        pipe.ctx.status()
        sd = host.build_shade_data(synth.make_globals(s["cull"], (w, h)), camera, sun, 0, w, h)
        direct = torch.zeros((h, w), dtype=torch.int32, device=pipe.ctx.device)
        pipe.ctx.shade_final(sd, att["gbuffer0"], att["gbuffer1"], pipe.depth, None, direct, w, h)
        pipe.ctx.status()
        assert off.tobytes() == default.tobytes() == direct.cpu().numpy().tobytes()
        emissive = (att["gbuffer0"].cpu().numpy().view(np.uint32) >> 24) != 0
        changed = on != off
        print("pipeline: %d emissive pixels, %d pixels changed by bloom" % (int(emissive.sum()), int(changed.sum())))
        assert emissive.sum() > 100 and (~emissive).sum() > 100
        assert changed.any() and changed[~emissive].any()  # light reaches pixels that emit nothing themselves
        # (this viewport's last level is 1 x 1, so light reaches every pixel: the reach is test_bloom_changes_final_only_within_the_reach_of_the_chain's)
        assert (SR.channels(on) >= SR.channels(off)).all()  # bloom only adds light: tonemap and the UNORM store are monotone
        bloom = pipe.bloom_image.cpu().numpy().view(np.uint32)
        assert (bloom[:pipe.bloom_desc.levelOffset[1]] != 0).any()
    finally:
        pipe.ctx.close()
