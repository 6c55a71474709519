"""Block-resident texture sets on the MI355X: nv_visibility_attributes_blocks, nv_shadow_trace_blocks and nv_rasterdepth_blocks
against the DECODED entry point run on the same device with the same inputs — every output bit-identical, gbuffer0 included: the two kernels
run the same operations on the same RGBA8 codes — and, for the attribute pass, against tests/texture_ref.c under test_textures_gpu._same's
rule.  Outputs are poisoned before every launch; the block buffer sits between canary units that must survive."""
import numpy as np
import pytest

import pixel_cases as PC
import raster_alpha_ref as RA
import shadow_alpha_ref as SA
import test_raster_alpha_cpu as RC
import test_raster_alpha_gpu as RG
import test_shade_gpu as TS
import test_shadow_alpha_cpu as AC
import test_shadow_alpha_gpu as AG
import test_shadowtrace_gpu as STG
import test_textures_gpu as TG
import texture_ref as TR
import visattr_ref as VA
from niagara_amd import host
from niagara_amd import layouts as L

POISON, POISON32, CANARY = TG.POISON, TG.POISON32, 0xC5
GUARD = 64  # canary bytes on both sides of a block buffer (a multiple of 16: the buffer stays aligned)

tref, aref, vref, rref, ctx = TG.tref, TG.aref, TG.vref, TG.rref, TG.ctx  # the fixtures of the decoded pass's tests


class BlockSet:
    """files -> the decoded set (device) and the block set between canaries (device), both with their host forms"""

    def __init__(self, ctx, files):
        import torch
        from niagara_amd import pipeline as P
        self.files = files
        self.descs, self.texels = ctx.texture_decode(files)
        self.hdescs, self.htexels = host.texture_decode_host(files)
        self.table = P.to_device(self.descs, ctx.device)
        self.bdescs, self.hblocks = host.texture_blocks_host(files)
        self.btable = P.to_device(self.bdescs, ctx.device)
        self.units = len(self.hblocks) // 16
        self.guarded = torch.full((len(self.hblocks) + 2 * GUARD,), CANARY, dtype=torch.uint8, device=ctx.device)
        self.guarded[GUARD:GUARD + len(self.hblocks)] = torch.from_numpy(self.hblocks.copy()).to(ctx.device)
        self.blocks = self.guarded[GUARD:GUARD + len(self.hblocks)]
        assert self.blocks.data_ptr() % 16 == 0
        ctx.status()

    def check_canaries(self):
        g = self.guarded.cpu().numpy()
        assert (g[:GUARD] == CANARY).all() and (g[-GUARD:] == CANARY).all(), "a canary of the block buffer was written"
        assert g[GUARD:-GUARD].tobytes() == self.hblocks.tobytes()


_SETS = {}


def _five(ctx):
    """the five-texture set of the decoded pass's tests: BC7 64^2, BC3 20 x 12 x 5, BC1 1 x 1, BC2 8 x 8, BC1 64^2"""
    if "five" not in _SETS:
        _SETS["five"] = BlockSet(ctx, TG._texture_files(np.random.default_rng(23)))
        fmts = [int(d["levelsFormat"]) >> 8 for d in _SETS["five"].bdescs[1:]]
        assert fmts == [7, 3, 1, 2, 1]
    return _SETS["five"]


def _blocks(ctx, s, records, w, h, btable, count, blocks, units, out=None, dev=None):
    """one launch of nv_visibility_attributes_blocks over exactly-sized device buffers into poisoned outputs (TG._textured's twin)"""
    from niagara_amd import pipeline as P
    out = out or TG._poisoned(ctx, w * h)
    t = dev or [P.to_device(s[k], ctx.device) for k in ("draws", "meshlets", "data", "vertices", "materials")] + [P.to_device(records, ctx.device)]
    ctx.visibility_attributes_blocks(s["g"], t[5], w, h, t[0], len(s["draws"]), t[1], len(s["meshlets"]), t[2], len(s["data"]), t[3], len(s["vertices"]),
                                     t[4], len(s["materials"]), out["attributes"], out["gbuffer0"], out["gbuffer1"], out["totals"], btable, count, blocks, units)
    return out, t


def _both(ctx, ts, s, rec, w, h, texel_words=None, units=None, count=None):
    """the decoded and the block entry point on the same device buffers: (decoded, blocks) host outputs, asserted bit-identical"""
    count = len(ts.descs) if count is None else count
    dec, dev = TG._textured(ctx, s, rec, w, h, ts.table, count, ts.texels, len(ts.htexels) if texel_words is None else texel_words)
    blk, _ = _blocks(ctx, s, rec, w, h, ts.btable, count, ts.blocks, ts.units if units is None else units, dev=dev)
    ctx.status()
    a, b = TG._host(dec), TG._host(blk)
    for k in ("totals", "attributes", "gbuffer1", "gbuffer0"):
        assert a[k].tobytes() == b[k].tobytes(), "%s differs from the decoded entry point's (%d words)" % (k, int((a[k].view(np.uint32) != b[k].view(np.uint32)).sum()))
    ts.check_canaries()
    return a, b


# ---------------------------------------------------------------------------------------------------------------- the attribute pass

@pytest.mark.gpu
def test_plane_equals_the_decoded_pass_over_every_level_and_the_wrap(ctx, tref, rref):
    ts = _five(ctx)
    s, rec = TG._plane_scene(rref)
    tref.hits()
    want = TG._reference(tref, s, rec, 160, 96, ts.hdescs, ts.htexels)
    hits = tref.hits()
    uv = want["attributes"]["uv"][(want["flags"] & VA.SHADED) != 0]
    assert uv[:, 0].max() - uv[:, 0].min() > 1 and uv[:, 1].max() - uv[:, 1].min() > 1, "uv does not span more than one period on both axes"
    assert int((hits[:7] > 0).sum()) >= 2, "fewer than two mip levels are reached"
    dec, blk = _both(ctx, ts, s, rec, 160, 96)
    TG._same("plane, blocks", blk, want, ts.hdescs, s["materials"])


@pytest.mark.gpu
def test_occluder_scene_equals_the_decoded_pass_and_untextured_without_a_table(ctx, tref, vref, aref):
    """320 x 192; the scene's five materials name the five-texture set in five orders, so every format is sampled"""
    from niagara_amd import pipeline as P
    ts = _five(ctx)
    s0, frame = TG._occluder_scene(vref, aref)
    s = dict(s0)
    m = s0["materials"].copy()
    for k in range(len(m)):
        ids = [1 + (k + j) % 5 for j in range(4)]
        m[k]["albedoTexture"], m[k]["normalTexture"], m[k]["specularTexture"], m[k]["emissiveTexture"] = ids
    s["materials"] = m
    rec = frame["resolve"]["records"]
    w, h = s["viewport"]
    assert (w, h) == (320, 192)
    tref.hits()
    want = TG._reference(tref, s, rec, w, h, ts.hdescs, ts.htexels)
    hits = tref.hits()
    shaded = (want["flags"] & VA.SHADED) != 0
    uv = want["attributes"]["uv"][shaded]
    assert want["totals"][0] > 20000 and want["totals"][3] == 0
    assert uv[:, 0].max() - uv[:, 0].min() > 1 and uv[:, 1].max() - uv[:, 1].min() > 1
    assert int((hits[:7] > 0).sum()) >= 2
    assert len(set(m["albedoTexture"][want["attributes"]["materialIndex"][shaded]].tolist())) >= 3  # lanes meet several formats
    dec, blk = _both(ctx, ts, s, rec, w, h)
    TG._same("occluder, blocks", blk, want, ts.hdescs, m)
    # a NULL table: nv_visibility_attributes' bytes, every output
    dev = [P.to_device(s[k], ctx.device) for k in ("draws", "meshlets", "data", "vertices", "materials")] + [P.to_device(rec, ctx.device)]
    bare, _ = _blocks(ctx, s, rec, w, h, None, 0, None, 0, dev=dev)
    plain = TG._poisoned(ctx, w * h)
    ctx.visibility_attributes(s["g"], dev[5], w, h, dev[0], len(s["draws"]), dev[1], len(s["meshlets"]), dev[2], len(s["data"]), dev[3], len(s["vertices"]),
                              dev[4], len(m), plain["attributes"], plain["gbuffer0"], plain["gbuffer1"], plain["totals"])
    ctx.status()
    a, b = TG._host(bare), TG._host(plain)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a) and a["totals"][3] > 0
    assert (a["gbuffer0"] != blk["gbuffer0"]).any()  # the textured output differs from the untextured one


@pytest.mark.gpu
def test_second_trip_with_textures_past_the_table(ctx, tref):
    """test_textures_gpu's second-trip case (2051 x (CUs + 1)): material 2 names a texture past the table, material 3 index == textureCount and
    0xFFFFFFFF — counted into totals[3], shaded from the factors, equal to the decoded path"""
    ts = _five(ctx)
    cus = TG._cus(ctx)
    w, h, n = PC.second_trip_sizes(cus)["pixel"]
    g = PC.check_second_trip(n, w, h, cus)
    s = PC.attr_scene((w, h))
    m = s["materials"].copy()
    m[3]["albedoTexture"], m[3]["specularTexture"], m[3]["normalTexture"] = len(ts.descs), 0xFFFFFFFF, 2
    m[0]["albedoTexture"], m[0]["emissiveTexture"] = 5, 1
    s["materials"] = m
    rec = PC.random_records(s, n, 11)
    want = TG._reference(tref, s, rec, w, h, ts.hdescs, ts.htexels)
    assert 0 < want["totals"][3] < want["totals"][0] and tref.bad_indices() == 0
    dec, blk = _both(ctx, ts, s, rec, w, h)
    raw = blk["attributes"].view(np.uint32).reshape(n, 16)
    assert (raw[g:] != POISON32).any(), "nothing of the second trip was written"
    assert blk["totals"][3] == want["totals"][3]
    TG._same("second trip, blocks", blk, want, ts.hdescs, m)


@pytest.mark.gpu
def test_runs_of_one_triangle_across_materials_of_different_formats(ctx, tref):
    """pixel_cases.run_edge_cases, groups b and c: adjacent runs of one triangle under draws whose materials name textures of different formats
    (BC7, BC1, BC2, BC3), so neighbouring lanes of a wave disagree on the format.  Asserted on the host before anything is launched."""
    ts = _five(ctx)
    fmt = lambda t: int(ts.bdescs[t]["levelsFormat"]) >> 8
    s = PC.attr_scene((64, 48))
    assert s["draws"]["materialIndex"].tolist() == [3, 0, 2]
    m = s["materials"].copy()
    for index, tex in ((0, (1, 5, 4, 2)), (2, (5, 0, 1, 3)), (3, (2, 1, 0, 0))):
        m[index]["albedoTexture"], m[index]["normalTexture"], m[index]["specularTexture"], m[index]["emissiveTexture"] = tex
    assert len({fmt(int(m[i]["albedoTexture"])) for i in (0, 2, 3)}) == 3  # BC7, BC1, BC3 as albedo
    s["materials"] = m
    cases = PC.run_edge_cases(s)
    images = cases["b"] + cases["c"]
    crossings = 0
    for image in images:
        lane, start, diff, named, key = PC.run_starts(image)
        valid = named & (key[:, 0] < len(s["draws"]))
        mat = np.where(valid, s["draws"]["materialIndex"][np.minimum(key[:, 0], len(s["draws"]) - 1)], -1)
        cross = np.zeros(len(key), bool)
        cross[1:] = (diff[1:] == 1) & valid[1:] & valid[:-1] & (mat[1:] != mat[:-1])
        assert all(fmt(int(m[mat[i]]["albedoTexture"])) != fmt(int(m[mat[i - 1]]["albedoTexture"])) for i in np.nonzero(cross)[0])
        crossings += int(cross.sum())
    assert crossings >= 12 * 3, crossings
    for image in images:
        w, h, rec = image["width"], image["height"], image["records"]
        si = PC.attr_scene((w, h))
        si["materials"] = m
        dec, blk = _both(ctx, ts, si, rec, w, h)
        TG._same(image["name"] + ", blocks", blk, TG._reference(tref, si, rec, w, h, ts.hdescs, ts.htexels), ts.hdescs, m)
    assert tref.bad_indices() == 0


@pytest.mark.gpu
def test_chain_one_unit_short_of_its_descriptor_is_not_sampled(ctx, tref):
    """units16 one short of the set: the last texture's chain ends one unit past it — treated as absent, counted into totals[3], shaded from the
    factors, as the decoded path treats the same texture with texelWords one short; the tail canary keeps its bytes"""
    ts = _five(ctx)
    s = PC.attr_scene((64, 48))
    m = s["materials"].copy()
    last = len(ts.descs) - 1
    m[0]["albedoTexture"], m[3]["normalTexture"], m[2]["albedoTexture"], m[2]["normalTexture"], m[2]["emissiveTexture"] = last, last, 1, 0, 0
    s["materials"] = m
    rec = PC.random_records(s, 64 * 48, 12)
    want = TG._reference(tref, s, rec, 64, 48, ts.hdescs, ts.htexels, texel_words=len(ts.htexels) - 1)
    full, _ = _both(ctx, ts, s, rec, 64, 48)
    dec, blk = _both(ctx, ts, s, rec, 64, 48, texel_words=len(ts.htexels) - 1, units=ts.units - 1)
    assert full["totals"][3] == 0 and blk["totals"][3] == want["totals"][3] > 0
    TG._same("one unit short, blocks", blk, want, ts.hdescs, m)


@pytest.mark.gpu
def test_the_launch_replays_from_a_captured_graph(ctx):
    import torch
    from niagara_amd import pipeline as P
    ts = _five(ctx)
    s = PC.attr_scene((96, 64))
    m = s["materials"].copy()
    m[0]["albedoTexture"], m[3]["normalTexture"], m[2]["emissiveTexture"] = 5, 1, 2
    s["materials"] = m
    rec = PC.random_records(s, 96 * 64, 13)
    want, _ = _both(ctx, ts, s, rec, 96, 64)
    out = TG._poisoned(ctx, 96 * 64)
    dev = [P.to_device(s[k], ctx.device) for k in ("draws", "meshlets", "data", "vertices", "materials")] + [P.to_device(rec, ctx.device)]

    def reset():
        for k in ("attributes", "gbuffer0", "gbuffer1"):
            out[k].fill_(POISON if k == "attributes" else POISON32)
        out["totals"].zero_()

    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        reset()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            _blocks(ctx, s, rec, 96, 64, ts.btable, len(ts.bdescs), ts.blocks, ts.units, out=out, dev=dev)
        torch.cuda.synchronize()
        assert (out["gbuffer0"] == POISON32).all()  # nothing ran during capture
        for _ in range(2):
            reset()
            graph.replay()
            torch.cuda.synchronize()
            got = TG._host(out)
            assert all(got[k].tobytes() == want[k].tobytes() for k in want)
    ctx.status()
    ts.check_canaries()


@pytest.mark.gpu
def test_misaligned_block_buffer_is_refused(ctx):
    from niagara_amd._lib import NvError
    ts = _five(ctx)
    s = PC.attr_scene((64, 48))
    rec = PC.random_records(s, 64 * 48, 12)
    out = TG._poisoned(ctx, 64 * 48)
    for bad in (ts.guarded[GUARD + 4:], ts.guarded[GUARD + 8:]):
        with pytest.raises(NvError):
            _blocks(ctx, s, rec, 64, 48, ts.btable, len(ts.bdescs), bad, ts.units - 1, out=out)
    with pytest.raises(NvError):
        _blocks(ctx, s, rec, 64, 48, ts.btable, len(ts.bdescs), None, ts.units, out=out)
    ctx.status()
    assert (out["gbuffer0"] == POISON32).all()


# ---------------------------------------------------------------------------------------------------------------- the shadow trace

def _bc_fuzz_files(rng):
    """six textures of shadow_alpha_ref.random_textures' shapes as DDS files of the four formats, random blocks (BC7: a valid mode each)"""
    shapes = [(8, 8, 1), (5, 3, 2), (1, 1, 1), (16, 4, 3), (7, 1, 1), (2, 9, 2)]
    files = []
    for (w, h, levels), fmt in zip(shapes, (7, 3, 1, 2, 7, 1)):
        b = rng.integers(0, 256, TR.image_size_bc(w, h, levels, TR.BLOCK_BYTES[fmt])[0], dtype=np.uint8)
        if fmt == 7:
            b[0::16] |= 1 << 6
        files.append(TG._dds(fmt, w, h, levels, b))
    return files


def _checker_bc2():
    """shadow_alpha_ref.layered_scene's 8 x 8 alpha checker as one BC2 level: explicit 4-bit alpha 0 / 15, a constant colour"""
    y, x = np.mgrid[0:8, 0:8]
    alpha = np.where((x + y) % 2 == 1, 0, 15)
    blocks = np.zeros((2, 2, 16), np.uint8)
    for by in range(2):
        for bx in range(2):
            a = alpha[by * 4:by * 4 + 4, bx * 4:bx * 4 + 4].reshape(-1)
            blocks[by, bx, :8] = a[0::2] | a[1::2] << 4
            blocks[by, bx, 8:12] = 0xFF
    return TG._dds(2, 8, 8, 1, blocks)


class TraceDevice(AG.Device):
    """test_shadow_alpha_gpu.Device over the decoded form of `files`, plus the block form between canaries on the same context"""

    def __init__(self, scene, files):
        from niagara_amd import pipeline as P
        descs, texels = host.texture_decode_host(files)
        AG.Device.__init__(self, scene, dict(descs=descs, texels=texels))
        import torch
        self.bdescs, hblocks = host.texture_blocks_host(files)
        self.hblocks = hblocks
        self.btable = P.to_device(self.bdescs, self.ctx.device)
        self.guarded = torch.full((len(hblocks) + 2 * GUARD,), CANARY, dtype=torch.uint8, device=self.ctx.device)
        self.guarded[GUARD:GUARD + len(hblocks)] = torch.from_numpy(hblocks.copy()).to(self.ctx.device)
        self.blocks = self.guarded[GUARD:GUARD + len(hblocks)]

    def block_args(self, **k):
        s = self.scene
        return {**dict(draws=self.draws, draw_count=len(s["draws"]), materials=self.materials, material_count=len(s["materials"]), textures=self.btable,
                       texture_count=len(self.bdescs), blocks=self.blocks, units16=len(self.hblocks) // 16), **k}

    def trace_blocks(self, sd, depth, quality=1, **k):
        h, w = depth.shape
        d, out = TS._dev(self.ctx, depth), TS._out(self.ctx, w * h)
        self.ctx.shadow_trace_blocks(sd, d, out, w, h, quality, **self.block_args(**k))
        self.ctx.status()
        g = self.guarded.cpu().numpy()
        assert (g[:GUARD] == CANARY).all() and (g[-GUARD:] == CANARY).all(), "a canary of the block buffer was written"
        return TS._host(out, w * h, np.uint8, (h, w))


@pytest.fixture(scope="module")
def cutout():
    s, _ = AC.cutout_occluder()
    dev = TraceDevice(s, s["textures"])
    yield dev
    dev.ctx.close()


@pytest.fixture(scope="module")
def bcfuzz():
    s, _ = SA.textured_fuzz_scene()
    dev = TraceDevice(s, _bc_fuzz_files(np.random.default_rng(77)))
    yield dev
    dev.ctx.close()


def _masks_equal(name, dev, sd, depth, **k):
    want = dev.trace(sd, depth, 1, **{a: b for a, b in k.items() if a == "draws"})
    got = dev.trace_blocks(sd, depth, 1, **k)
    print("%s: %d texels, %d occluded, %d lit, %d differ from the decoded trace" % (name, want.size, int((want == 0).sum()), int((want == 255).sum()),
                                                                               int((want != got).sum())))
    assert got.tobytes() == want.tobytes()
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("checkerboard", [0, 1])
@pytest.mark.parametrize("size", [(65, 17), (67, 37)])
@pytest.mark.parametrize("which", ["cutout", "bcfuzz"])
def test_mask_equals_the_decoded_trace(which, size, checkerboard, cutout, bcfuzz):
    """the cut-out occluder scene (its BC1 set) and the fuzz scene over six textures of all four formats, two sizes of
    test_shadow_alpha_gpu.SIZES, with and without jitter and checkerboard; quality 0 is nv_shadow_trace's launch"""
    dev = cutout if which == "cutout" else bcfuzz
    w, h = size
    assert size in AG.SIZES
    seen = set()
    for jitter in (0.0, 1e-2):
        sd, depth = STG._inputs(w, h, jitter, checkerboard)
        want = _masks_equal("%s %dx%d checkerboard %d jitter %g" % (which, w, h, checkerboard, jitter), dev, sd, depth)
        seen |= set(np.unique(want).tolist())
        d, a, b = TS._dev(dev.ctx, depth), TS._out(dev.ctx, w * h), TS._out(dev.ctx, w * h)
        dev.ctx.shadow_trace_blocks(sd, d, a, w, h, 0, **dev.block_args())
        dev.ctx.shadow_trace(sd, d, b, w, h, 0)
        dev.ctx.status()
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert which == "cutout" or {0, 255} <= seen  # (the fuzz scene surrounds the camera: both outcomes at every size)


@pytest.mark.gpu
def test_the_layered_scene_splits_the_lanes_of_a_wave():
    """test_shadow_alpha_gpu's layered scene with its checker as a BC2 texture: neighbouring lanes of a wave disagree at the alpha test"""
    s, t = SA.layered_scene(box=True)
    files = [_checker_bc2()]
    descs, texels = host.texture_decode_host(files)
    assert texels.tobytes() != b"" and ((texels >> 24).reshape(8, 8) == (t["texels"] >> 24).reshape(8, 8)).all()  # the same alpha checker
    dev = TraceDevice(s, files)
    try:
        w, h = 64, 64
        sd = np.zeros(1, L.SHADOWDATA)
        sd["sunDirection"], sd["imageSize"] = (0.02, 0.03, 1.0), (w, h)
        m = np.zeros((4, 4), np.float32)
        m[0, 0], m[1, 1], m[3, 3] = 3.9, 3.9, 1.0
        sd["inverseViewProjection"] = m.T.reshape(-1)
        depth = np.full((h, w), 0.5, np.float32)
        want = _masks_equal("layered scene", dev, sd, depth)
        assert int((want[:, 1:] != want[:, :-1]).sum()) >= 50  # the mask changes along rows inside 8 x 8 tiles
    finally:
        dev.ctx.close()


@pytest.mark.gpu
def test_a_rebuilt_tlas_in_between():
    from niagara_amd import pipeline as P
    s, _ = SA.textured_fuzz_scene()
    dev = TraceDevice(s, _bc_fuzz_files(np.random.default_rng(78)))
    try:
        c = dev.ctx
        c.rt_scene_reserve_dynamic(len(s["draws"]) + 3)
        w, h = 67, 37
        sd, depth = STG._inputs(w, h, 1e-2, 0)
        before = _masks_equal("before the rebuild", dev, sd, depth)
        moved = s["draws"].copy()
        rng = np.random.default_rng(31)
        moved["position"] += rng.uniform(-3, 3, moved["position"].shape).astype(np.float32)
        moved["postPass"] = np.roll(moved["postPass"], 1)
        db = P.to_device(moved, c.device)
        c.rt_tlas_build(db, len(moved))
        after = _masks_equal("after the rebuild", dev, sd, depth, draws=db)
        assert (before != after).sum() >= 50
    finally:
        dev.ctx.close()


@pytest.mark.gpu
def test_refused_trace_calls_launch_nothing(bcfuzz):
    from niagara_amd import pipeline as P
    from niagara_amd._lib import NvError
    w, h = 21, 3
    sd, depth = STG._inputs(w, h, 0.0, 0)
    d, out = TS._dev(bcfuzz.ctx, depth, 8), TS._out(bcfuzz.ctx, w * h)

    def call(c=bcfuzz.ctx, **k):
        a = {**dict(shadow_data=sd, depth=d, shadow=out, width=w, height=h, quality=1), **bcfuzz.block_args(), **k}
        c.shadow_trace_blocks(**a)
    fresh = P.Context()
    try:
        s = bcfuzz.scene
        with pytest.raises(NvError):  # no scene uploaded
            call(c=fresh)
        fresh.rt_scene_upload(fresh.rt_scene_build(s["meshes"], s["indices"], s["vertices"], s["draws"]))
        with pytest.raises(NvError):  # a scene without texcoords
            call(c=fresh)
        with pytest.raises(NvError):  # ... at quality 0 too
            call(c=fresh, quality=0)
        fresh.status()
    finally:
        fresh.close()
    byte = lambda t: t[4:]
    for kw in (dict(quality=2), dict(quality=-1), dict(blocks=byte(bcfuzz.blocks)), dict(blocks=bcfuzz.blocks[8:]), dict(blocks=None), dict(textures=None),
               dict(textures=byte(bcfuzz.btable)), dict(materials=byte(bcfuzz.materials)), dict(draws=byte(bcfuzz.draws)), dict(width=w + 1), dict(shadow=None)):
        with pytest.raises(NvError):
            call(**kw)
    bcfuzz.ctx.status()
    assert (out == POISON).all()
    call()
    bcfuzz.ctx.status()
    assert np.isin(out.cpu().numpy()[:w * h], (0, 255)).all()


# ---------------------------------------------------------------------------------------------------------------- the raster

def _raster_blocks(ctx, args, w, h, mats, files, near_clip=0, stable=0, limit=None):
    """nv_rasterdepth_blocks through Context.rasterdepth_blocks into the targets test_raster_alpha_gpu._gpu uses: the same dict"""
    import torch
    from niagara_amd import pipeline as P
    dev = ctx.device
    ctx.set_option(P.NV_OPT_RASTER_NEAR_CLIP, near_clip)
    ctx.set_option(P.NV_OPT_RASTER_VISIBILITY_ID, stable)
    if limit is not None:
        ctx.set_option(P.NV_OPT_RASTER_SMALL_LIMIT, limit)
    try:
        t = [P.to_device(a, dev) for a in args[1:]]
        bdescs, hblocks = host.texture_blocks_host(files)
        guarded = torch.full((len(hblocks) + 2 * GUARD,), CANARY, dtype=torch.uint8, device=dev)
        guarded[GUARD:GUARD + len(hblocks)] = torch.from_numpy(hblocks.copy()).to(dev)
        d = torch.zeros((h, w), dtype=torch.float32, device=dev)
        v = torch.zeros((h, w), dtype=torch.int64, device=dev)
        tot = torch.zeros(4, dtype=torch.int64, device=dev)
        alpha = torch.zeros(2, dtype=torch.int64, device=dev)
        ctx.rasterdepth_blocks(args[0], *t, d, w, h, v, tot, materials=P.to_device(np.ascontiguousarray(mats, L.MATERIAL), dev), material_count=len(mats),
                               textures=P.to_device(bdescs, dev), texture_count=len(bdescs), blocks=guarded[GUARD:GUARD + len(hblocks)],
                               units16=len(hblocks) // 16, alpha_totals2=alpha)
        ctx.status()
        g = guarded.cpu().numpy()
        assert (g[:GUARD] == CANARY).all() and (g[-GUARD:] == CANARY).all(), "a canary of the block buffer was written"
        return dict(depth=d.cpu().numpy(), visibility=v.cpu().numpy().view(np.uint64), totals=tot.cpu().numpy().view(np.uint64),
                    alpha=alpha.cpu().numpy().view(np.uint64))
    finally:
        ctx.set_option(P.NV_OPT_RASTER_SMALL_LIMIT, 16)
        ctx.set_option(P.NV_OPT_RASTER_NEAR_CLIP, 0)
        ctx.set_option(P.NV_OPT_RASTER_VISIBILITY_ID, 0)


def _raster_both(name, ctx, s, **k):
    w, h = s["viewport"]
    tex = RC._tex(s)
    host_descs, host_texels = host.texture_decode_host(s["textures"])
    assert host_descs.tobytes() == np.ascontiguousarray(tex["descs"], L.TEXTUREDESC).tobytes() and host_texels.tobytes() == np.ascontiguousarray(tex["texels"], np.uint32).tobytes()
    dec = RG._gpu(ctx, RA.args(s), w, h, tex, k.get("near_clip", 0), k.get("stable", 0), k.get("limit"))
    blk = _raster_blocks(ctx, RA.args(s), w, h, tex["materials"], s["textures"], **k)
    print("%s: kept %d dropped %d unevaluated %d; depth / visibility words that differ from the decoded raster %d / %d" %
          (name, int(dec["totals"][3]), int(dec["alpha"][0]), int(dec["alpha"][1]), int((dec["depth"].view(np.uint32) != blk["depth"].view(np.uint32)).sum()),
           int((dec["visibility"] != blk["visibility"]).sum())))
    for key in ("totals", "alpha", "depth", "visibility"):
        assert dec[key].tobytes() == blk[key].tobytes(), key
    return dec


@pytest.mark.gpu
@pytest.mark.parametrize("stable", [0, 1])
@pytest.mark.parametrize("viewport", [(67, 37), (320, 192)])
def test_the_cutout_wall_equals_the_decoded_raster_on_both_paths(viewport, stable, ctx, tref):
    """67 x 37: every triangle of the wall is small (a lane walks it alone); 320 x 192: every triangle takes the wave path; mip-mapped sets"""
    s = RA.occluder(tref, viewport, True, size=256 if viewport[0] == 320 else 64)
    dec = _raster_both("occluder %dx%d stable %d" % (viewport + (stable,)), ctx, s, stable=stable)
    assert dec["alpha"][0] > 200 and dec["totals"][3] > 200
    if viewport[0] == 320:  # and with the limit that sends every triangle down the wave path
        _raster_both("occluder 320x192 stable %d, limit 0" % stable, ctx, s, stable=stable, limit=0)


@pytest.mark.gpu
@pytest.mark.parametrize("stable", [0, 1])
def test_the_clipped_floor_equals_the_decoded_raster(stable, ctx, tref):
    s = RA.floor(tref, (320, 192), True)
    dec = _raster_both("floor 320x192 near clip, stable %d" % stable, ctx, s, near_clip=1, stable=stable)
    assert dec["alpha"][0] > 500 and dec["totals"][3] > 500


@pytest.mark.gpu
def test_a_wave_takes_slot_after_slot_of_different_materials(ctx, tref):
    import torch
    waves = torch.cuda.get_device_properties(ctx.device).multi_processor_count * 6 * 4
    slots = 4 * waves
    s = RA.sequence(tref, True, slots)
    dec = _raster_both("slot sequence, %d slots" % slots, ctx, s)
    assert dec["alpha"][0] > slots and dec["totals"][3] > slots


# ---------------------------------------------------------------------------------------------------------------- the pipeline

def _pipeline_image(s, resident):
    from niagara_amd import pipeline as P
    pipe = STG._pipeline(s, 0)
    try:
        pipe.set_textures(s["textures"], resident=resident)
        pipe.build_rt_scene(s["meshes"], s["indices"], s["vertices"], s["draws"], texcoords=True)
        vis = pipe.new_visibility()
        for _ in range(2):
            pipe.frame(s["cull"], post_pass=True, visibility=vis, textures=True, materials=s["materials"])
        res = pipe.resolve(s["cull"], vis)
        att = pipe.attributes(s["cull"], res["records"], s["materials"], textures=True)
        color = pipe.shade(s["cull"], att["gbuffer0"], att["gbuffer1"], (0.0, 0.0, 0.0), STG.SUN, shadow="trace", blur=False, textures=True, materials=s["materials"])
        pipe.ctx.status()
        out = dict(color=color.cpu().numpy().copy(), shadow=pipe.shadow_image.cpu().numpy().copy(), depth=pipe.depth.cpu().numpy().copy(),
                   gbuffer0=att["gbuffer0"].cpu().numpy().copy(), records=P.from_device(res["records"], L.VISRECORD).copy(), bytes=pipe.texture_resident_bytes)
        return out
    finally:
        pipe.ctx.close()


@pytest.mark.gpu
def test_the_pipeline_gives_the_decoded_runs_image_from_a_block_set():
    """set_textures(resident="blocks") -> frame(textures=True) -> resolve -> attributes -> shade(shadow="trace", textures=True) at 320 x 192 on the
    cut-out occluder scene: the final image of the decoded run byte for byte; the resident bytes are the payloads', each rounded up to 16"""
    s, _ = AC.cutout_occluder()
    assert tuple(s["viewport"]) == (320, 192)
    dec, blk = _pipeline_image(s, "decoded"), _pipeline_image(s, "blocks")
    for k in ("records", "depth", "gbuffer0", "shadow", "color"):
        assert dec[k].tobytes() == blk[k].tobytes(), k
    assert (dec["shadow"] == 0).any() and (dec["shadow"] == 255).any()
    payloads = [host.dds_parse(f)["payloadBytes"] for f in s["textures"]]
    assert blk["bytes"] == sum((p + 15) // 16 * 16 for p in payloads)
    assert dec["bytes"] == 4 * host.texture_set_layout(s["textures"])[1] and dec["bytes"] > 7 * blk["bytes"]  # BC1: 8 x, less the tail's partial blocks


# ---------------------------------------------------------------------------------------------------------------- the code objects

@pytest.mark.parametrize("source,kernel", [("visattr_blocks", "visibility_attributes_kernel"), ("shadowtrace_blocks", "shadow_trace_kernel"),
                                           ("rasterdepth_blocks", "rasterdepth_kernel")])
def test_block_kernels_use_no_scratch_memory(source, kernel, tmp_path):
    """every kernel of the three new code objects, compiled with the Makefile's flags: 0 bytes of private segment, no spilled vector register"""
    import os
    import subprocess
    csrc = os.path.join(os.path.dirname(TG.HERE), "niagara_amd", "csrc")
    asm = str(tmp_path / (source + ".s"))
    subprocess.check_call(["hipcc", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize", "--offload-arch=gfx950", "--cuda-device-only",
                           "-S", os.path.join(csrc, source + ".hip"), "-o", asm], stderr=subprocess.DEVNULL)
    text = open(asm).read()
    entries = [e for e in text[text.index("amdhsa.kernels:"):].split("\n  - .")[1:] if kernel in e.split(".name:")[1].split()[0]]
    assert len(entries) == (4 if source == "rasterdepth_blocks" else 1)
    for e in entries:
        field = lambda name: int(e.split("." + name + ":")[1].split()[0])
        print("%s: %d VGPRs, %d SGPRs, %d bytes LDS, %d bytes scratch" % (e.split(".name:")[1].split()[0], field("vgpr_count"), field("sgpr_count"),
                                                                         field("group_segment_fixed_size"), field("private_segment_fixed_size")))
        assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0
