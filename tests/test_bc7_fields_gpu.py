"""The BC7 decode on every partition and header field, on the MI355X: the blocks of tests/golden/textures/bc7_fields.npz
(tests/test_bc7_fields_cpu.py says what they walk) packed into single-level textures and sent through every device consumer of a block —
nv_texture_decode against the fixture's bytes, the attribute pass of both residencies against each other and against tests/texture_ref.c,
the alpha-tested raster and shadow trace of both residencies against each other and against their restatements (there with a BC2 and a BC3
texture of bc_blocks.npz's blocks beside the BC7 one).  Whether a launch reads the blocks it is meant to read is a property of its inputs:
each is asserted on the CPU restatement before anything is launched.  One context serves the module."""
import os

import numpy as np
import pytest

import raster_alpha_ref as RA
import raster_ref as RR
import shadow_alpha_ref as SA
import test_bc7_fields_cpu as BF
import test_raster_alpha_gpu as RG
import test_shadowtrace_gpu as STG
import test_texture_blocks_cpu as BC
import test_texture_blocks_gpu as BG
import test_textures_gpu as TG
import texture_ref as TR
import visattr_ref as VA
from niagara_amd import host
from niagara_amd import layouts as L

tref, rref = TG.tref, TG.rref
FIELD_SHAPES = [(64, 64), (64, 64), (64, 40)]  # 256 + 256 + 160 blocks: the fixture's 672 exactly
ALPHA_SHAPES = [(7, 64, 56), (2, 64, 32), (3, 64, 64)]  # the fixture's 224 alpha-carrying BC7 blocks, bc_blocks.npz's 128 BC2 and 256 BC3 blocks
EDGE = 1.0 / 64  # the quads' texcoords run from -EDGE to 1 + EDGE (exact in fp16): the wrap is crossed on all four sides


@pytest.fixture(scope="module")
def fields():
    f = np.load(os.path.join(BF.TEXTURES, "bc7_fields.npz"))
    return f["bc7"], f["bc7_rgba"]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(BF.TEXTURES, "bc_blocks.npz"))


@pytest.fixture(scope="module")
def araster(tmp_path_factory):
    return RA.load(tmp_path_factory.mktemp("raster_alpha_ref_bc7_fields"))


@pytest.fixture(scope="module")
def ashadow(tmp_path_factory):
    return SA.load(tmp_path_factory.mktemp("shadow_alpha_ref_bc7_fields"))


def _field_files(blocks):
    assert sum(w * h // 16 for w, h in FIELD_SHAPES) == len(blocks)
    files, at = [], 0
    for w, h in FIELD_SHAPES:
        files.append(TG._dds(7, w, h, 1, blocks[at:at + w * h // 16]))
        at += w * h // 16
    return files


def _alpha_blocks(fields, golden):
    """per texture of ALPHA_SHAPES its blocks; the BC7 ones are the fixture's blocks of modes 4 to 7, in the fixture's order"""
    modes = np.array([BF.header(b)["mode"] for b in fields[0]])
    out = [fields[0][modes >= 4], golden["bc2"], golden["bc3"]]
    assert [len(b) for b in out] == [w * h // 16 for _, w, h in ALPHA_SHAPES]
    return out


def _alpha_files(fields, golden):
    return [TG._dds(fmt, w, h, 1, b) for (fmt, w, h), b in zip(ALPHA_SHAPES, _alpha_blocks(fields, golden))]


def _by_block(texels, w, h):
    """the words of one w x h level -> (blocks, 64) bytes, blocks in the payload's order"""
    return np.ascontiguousarray(np.asarray(texels, np.uint32).reshape(h // 4, 4, w // 4, 4).transpose(0, 2, 1, 3)).reshape(-1, 16).view(np.uint8).reshape(-1, 64)


def _rotation_classes(blocks):
    """(mode, rotation) -> the indices of the blocks of modes 4 and 5 that carry it"""
    out = {}
    for i, b in enumerate(blocks):
        h = BF.header(b)
        if h["mode"] in (4, 5):
            out.setdefault((h["mode"], h["rotation"]), []).append(i)
    assert sorted(out) == [(m, r) for m in (4, 5) for r in range(4)]
    return out


def _inverted_alpha(descs, texels, tex_id, blocks):
    """a copy of the decoded set in which the texels of `blocks` of texture tex_id carry the complement of their alpha code: a restatement run
    over it differs from the run over the set itself exactly where a sample reads one of these blocks"""
    out = np.array(texels, np.uint32, copy=True)
    d = descs[tex_id]
    level = out[int(d["offset"]):int(d["offset"]) + int(d["width"]) * int(d["height"])].reshape(int(d["height"]), int(d["width"]))
    for b in blocks:
        by, bx = divmod(int(b), int(d["width"]) // 4)
        level[by * 4:by * 4 + 4, bx * 4:bx * 4 + 4] ^= np.uint32(0xFF000000)
    return out


# ---------------------------------------------------------------------------------------------------------------- the context

def _shadow_scene():
    """three cut-out walls (shadow_ref.geometry's 4 x 4 grid of quads, texcoords (x, y) / 2 + 1 / 2, postPass 1, one material and one texture of
    ALPHA_SHAPES each) side by side at z = 6 over a receiver at z = 0, seen by an orthographic camera of 288 x 96 texels: a wall is 88 texels
    of the image across, so a texel of its 64-wide texture spans 1.4 of them and every ray meets one wall at most once"""
    s, _ = SA.layered_scene()
    draws = np.zeros(3, L.MESHDRAW)
    draws["orientation"], draws["scale"], draws["meshIndex"], draws["postPass"] = (0.0, 0.0, 0.0, 1.0), 1.2, 0, 1
    draws["position"] = [(-2.6, 0.0, 6.0), (0.0, 0.0, 6.0), (2.6, 0.0, 6.0)]
    draws["materialIndex"] = (0, 1, 2)
    m = np.zeros(3, L.MATERIAL)
    m["albedoTexture"], m["diffuseFactor"] = (1, 2, 3), (1, 1, 1, 1)
    w, h = 288, 96
    sd = np.zeros(1, L.SHADOWDATA)
    sd["sunDirection"], sd["imageSize"] = (0.004, 0.006, 1.0), (w, h)
    inv = np.zeros((4, 4), np.float32)
    inv[0, 0], inv[1, 1], inv[3, 3] = 3.9, 1.3, 1.0  # clip x, y in [-1, 1] -> world x in [-3.9, 3.9], y in [-1.3, 1.3], z = 0
    sd["inverseViewProjection"] = inv.T.reshape(-1)
    return dict(s, draws=draws, materials=m), sd, np.full((h, w), 0.5, np.float32)


@pytest.fixture(scope="module")
def shadow(fields, golden):
    """the module's one context: test_texture_blocks_gpu.TraceDevice over the shadow scene and the alpha set"""
    dev = BG.TraceDevice(_shadow_scene()[0], _alpha_files(fields, golden))
    yield dev
    dev.ctx.close()


@pytest.fixture(scope="module")
def ctx(shadow):
    return shadow.ctx


# ---------------------------------------------------------------------------------------------------------------- the decode kernel

@pytest.mark.gpu
def test_device_decode_equals_the_fixture_and_the_host(ctx, fields):
    blocks, want = fields
    n = len(blocks)
    files = [TG._dds(7, 4 * n, 4, 1, blocks)] + _field_files(blocks)
    descs, got = TG._decode_with_canaries(ctx, files)
    at = lambda i: got[int(descs[i]["offset"]):int(descs[i]["offset"]) + int(descs[i]["width"]) * int(descs[i]["height"])]
    strip = np.ascontiguousarray(at(1).reshape(4, n, 4).transpose(1, 0, 2)).reshape(n, 16).view(np.uint8).reshape(n, 64)
    bad = np.nonzero((strip != want).any(axis=1))[0]
    assert len(bad) == 0, "blocks %s of the strip differ; first: %s" % (bad[:8], BF.header(blocks[bad[0]]))
    packed = np.concatenate([_by_block(at(2 + k), w, h) for k, (w, h) in enumerate(FIELD_SHAPES)])
    bad = np.nonzero((packed != want).any(axis=1))[0]
    assert len(bad) == 0, "blocks %s of the packed textures differ; first: %s" % (bad[:8], BF.header(blocks[bad[0]]))
    hdescs, htexels = host.texture_decode_host(files)
    for i in range(1, len(files) + 1):
        words = int(hdescs[i]["width"]) * int(hdescs[i]["height"])
        assert at(i).tobytes() == htexels[int(hdescs[i]["offset"]):int(hdescs[i]["offset"]) + words].tobytes(), i


# ---------------------------------------------------------------------------------------------------------------- the attribute pass

ATTR_VIEWPORT = (96, 96)
SLOTS = ("albedoTexture", "normalTexture", "specularTexture", "emissiveTexture")


def _quad_scene(rref, material):
    """one screen-facing quad of two triangles under one draw at 96 x 96, some 88 pixels across (a texel of a 64-wide texture spans 1.3 pixels),
    texcoords -EDGE .. 1 + EDGE over it; material k names the three packed textures in the slots' order rotated by k, so over the three
    materials every texture stands in every slot.  Returns (scene, records of the reference rasteriser's visibility words)"""
    w, h = ATTR_VIEWPORT
    pos = np.array([(-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0)], np.float32)
    draws = np.zeros(1, L.MESHDRAW)
    draws["position"], draws["scale"], draws["orientation"], draws["materialIndex"] = (0.013, -0.021, -6.0), 3.85, (0.0, 0.0, 0.0, 1.0), material
    s = RR.mesh_scene(pos, [(0, 1, 2), (0, 2, 3)], (w, h), draws=draws, flags=dict(postPass=1))
    v = VA.fill_attributes(s["vertices"], s["meshlets"], s["data"])
    uv = np.where(pos[:, :2] > 0, 1.0 + EDGE, -EDGE).astype(np.float16)
    v["tu"], v["tv"] = uv[:, 0].view(np.uint16), uv[:, 1].view(np.uint16)
    s["vertices"] = v
    m = VA.make_materials()
    m["diffuseFactor"], m["specularFactor"], m["emissiveFactor"] = (1, 1, 1, 1), (1, 1, 1, 1), (1, 1, 1)  # the taps reach the G-buffer unscaled
    for k in range(3):
        for j, slot in enumerate(SLOTS):
            m[k][slot] = 1 + (k + j) % 3
    s["materials"] = m
    _, vis, _ = rref.raster(*RR.raster_args(s), w, h, visibility=True)
    vis = vis.reshape(-1)
    slot, tri = (vis >> np.uint64(7)).astype(np.uint32) & np.uint32((1 << 25) - 1), (vis & np.uint64(127)).astype(np.uint32)
    cmd = s["cib"][slot]
    rec = np.zeros(len(vis), L.VISRECORD)
    rec["drawId"] = np.where(vis != 0, s["commands"]["drawId"][cmd & 0xFFFFFF], 0xFFFFFFFF)
    rec["meshletIndex"] = np.where(vis != 0, s["commands"]["taskOffset"][cmd & 0xFFFFFF] + (cmd >> 24), 0)
    rec["triangle"] = np.where(vis != 0, tri, 0)
    rec["depthBits"] = (vis >> np.uint64(32)).astype(np.uint32)
    return s, rec


def _blocks_tapped(uv, width, height):
    """the level-0 blocks the four taps of each sample at `uv` read, by the sampler's own index rule (test_texture_blocks_cpu._axis)"""
    seen = np.zeros((height // 4, width // 4), bool)
    for u, v in uv:
        for y in BC._axis(v, height):
            for x in BC._axis(u, width):
                seen[y >> 2, x >> 2] = True
    return seen


def attr_case(tref, rref, material, hdescs, htexels):
    """the scene, its records and the restatement's output for one material; asserts that the shaded pixels' taps read every block of level 0 of
    the texture in every slot"""
    s, rec = _quad_scene(rref, material)
    w, h = ATTR_VIEWPORT
    want = TG._reference(tref, s, rec, w, h, hdescs, htexels)
    shaded = (want["flags"] & VA.SHADED) != 0
    assert want["totals"][3] == 0 and tref.bad_indices() == 0 and ((want["flags"] & TR.NORMAL_MAPPED) != 0).sum() == shaded.sum() > 6000
    uv = want["attributes"]["uv"][shaded]
    assert uv.min() < 0 and uv.max() > 1
    coverage = {}
    for shape in sorted(set(FIELD_SHAPES)):
        coverage[shape] = _blocks_tapped(uv, *shape)
    for slot in SLOTS:
        tex = int(s["materials"][material][slot])
        seen = coverage[FIELD_SHAPES[tex - 1]]
        assert seen.all(), "material %d, %s: %d blocks of texture %d are never tapped" % (material, slot, int((~seen).sum()), tex)
    print("material %d: %d shaded pixels, textures %s in the four slots, taps read %s blocks" %
          (material, int(shaded.sum()), [int(s["materials"][material][k]) for k in SLOTS], {k: "%d of %d" % (int(v.sum()), v.size) for k, v in coverage.items()}))
    return s, rec, want


@pytest.fixture(scope="module")
def field_set(ctx, fields):
    return BG.BlockSet(ctx, _field_files(fields[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("material", [0, 1, 2])
def test_both_attribute_passes_read_every_block_in_every_slot(material, ctx, field_set, tref, rref):
    ts = field_set
    assert [int(d["levelsFormat"]) for d in ts.bdescs[1:]] == [1 | 7 << 8] * 3
    s, rec, want = attr_case(tref, rref, material, ts.hdescs, ts.htexels)
    w, h = ATTR_VIEWPORT
    dec, blk = BG._both(ctx, ts, s, rec, w, h)
    TG._same("fixture quad, material %d" % material, dec, want, ts.hdescs, s["materials"])


# ---------------------------------------------------------------------------------------------------------------- the alpha-tested raster

def raster_scene(tref, files, tess):
    """three screen-facing quads side by side at 320 x 192, each a tess x tess grid of cells of two triangles, each some 96 pixels across under its
    own draw and material (albedo textures 1, 2, 3 of the alpha set, texcoords -EDGE .. 1 + EDGE), in the post pass.  tess 1: two triangles of
    thousands of pixels each (the wave path); tess 32: triangles whose box holds 16 centres at most (a lane walks it alone)"""
    k = np.arange(tess + 1)
    x, y = np.meshgrid(k, k)
    x, y = x.reshape(-1) / tess, y.reshape(-1) / tess
    pos = np.stack([2 * x - 1, 2 * y - 1, np.zeros_like(x)], -1)
    tris = []
    for j in range(tess):
        for i in range(tess):
            a = j * (tess + 1) + i
            tris += [(a, a + 1, a + tess + 2), (a, a + tess + 2, a + tess + 1)]
    draws = np.zeros(3, L.MESHDRAW)
    draws["orientation"], draws["scale"], draws["postPass"] = (0.0, 0.0, 0.0, 1.0), 2.1, 1
    draws["position"] = [(-4.537, 0.021, -6.0), (0.013, -0.017, -6.0), (4.563, 0.009, -6.0)]
    draws["materialIndex"] = (0, 1, 2)
    s = RR.mesh_scene(pos, tris, (320, 192), draws=draws)
    v = s["vertices"].copy()
    uv = np.stack([x * (1 + 2 * EDGE) - EDGE, y * (1 + 2 * EDGE) - EDGE], -1).astype(np.float16)
    v["tu"], v["tv"] = uv[:, 0].view(np.uint16), uv[:, 1].view(np.uint16)
    s["vertices"] = v
    m = np.zeros(3, L.MATERIAL)
    m["albedoTexture"], m["diffuseFactor"] = (1, 2, 3), (1, 1, 1, 1)
    s["materials"], s["textures"] = m, files
    s["descs"], s["texels"] = tref.decode_set(files)
    s["g"]["cullData"]["postPass"] = 1
    return s


def raster_conditions(araster, s, blocks):
    """on the restatement: every texture has evaluated samples of which 20 % to 80 % fail the test, and samples read BC7 blocks of every rotation
    of modes 4 and 5.  Returns the shares"""
    w, h = s["viewport"]
    tex = dict(materials=s["materials"], descs=s["descs"], texels=s["texels"])
    base = araster.raster(*RA.args(s), w, h, log=2 * w * h, **tex)
    smp = base["samples"]
    assert (smp["status"] == RA.SAMPLED).all() and base["alpha"][1] == 0
    shares = []
    for draw in range(3):
        mine = smp[smp["drawId"] == draw]
        assert len(mine) > 5000, (draw, len(mine))
        shares.append(float((mine["keep"] == 0).mean()))
        assert 0.2 <= shares[-1] <= 0.8, (draw, shares)
    for key, members in _rotation_classes(blocks[0]).items():
        other = araster.raster(*RA.args(s), w, h, log=2 * w * h, **dict(tex, texels=_inverted_alpha(s["descs"], s["texels"], 1, members)))["samples"]
        assert len(other) == len(smp) and (other["alpha"] != smp["alpha"]).sum() >= 16, "no sample reads a block of mode %d, rotation %d" % key
    return base, shares


@pytest.mark.gpu
@pytest.mark.parametrize("tess", [1, 32])
def test_both_rasters_alpha_test_the_fixture_blocks(tess, ctx, fields, golden, tref, araster):
    blocks = _alpha_blocks(fields, golden)
    s = raster_scene(tref, _alpha_files(fields, golden), tess)
    base, shares = raster_conditions(araster, s, blocks)
    c = base["counters"]
    assert (c["tested_large"] == 6 and c["tested_small"] == 0) if tess == 1 else (c["tested_small"] == 3 * 2 * 32 * 32 and c["tested_large"] == 0)
    print("raster, tess %d: %d samples evaluated, discard shares BC7 %.3f BC2 %.3f BC3 %.3f" % ((tess, c["tested_samples"]) + tuple(shares)))
    dec = BG._raster_both("fixture quads, tess %d" % tess, ctx, s)
    w, h = s["viewport"]
    tex = dict(materials=s["materials"], descs=s["descs"], texels=s["texels"])
    RG._compare("fixture quads, tess %d" % tess, dec, lambda policy: araster.raster(*RA.args(s), w, h, band=False, policy=policy, **tex), False)


# ---------------------------------------------------------------------------------------------------------------- the alpha-tested shadow trace

def shadow_conditions(ashadow, s, sd, depth, tset, blocks):
    """on the restatement: per wall the rays that meet it (each evaluates one sample) and the share the alpha test rejects, 20 % to 80 %; rays
    read BC7 blocks of every rotation of modes 4 and 5.  Returns (the restatement's mask, the shares)"""
    h, w = depth.shape
    poison = np.full((h, w), STG.POISON, np.uint8)
    want, rejected = ashadow.shadow_trace(sd, s, tset, depth, poison, 1)
    assert rejected.max() == 1 and not ((rejected > 0) & (want == 0)).any()  # one wall per ray: a ray is stopped or let through once
    shares = []
    for draw in range(3):
        mask, rej = ashadow.shadow_trace(sd, dict(s, draws=s["draws"][draw:draw + 1]), tset, depth, poison, 1)
        evaluated = (mask == 0) | (rej > 0)
        assert evaluated.sum() > 5000, (draw, int(evaluated.sum()))
        shares.append(float((rej > 0).sum() / evaluated.sum()))
        assert 0.2 <= shares[-1] <= 0.8, (draw, shares)
    for key, members in _rotation_classes(blocks[0]).items():
        other, _ = ashadow.shadow_trace(sd, s, dict(descs=tset["descs"], texels=_inverted_alpha(tset["descs"], tset["texels"], 1, members)), depth, poison, 1)
        assert (other != want).sum() >= 16, "no ray reads a block of mode %d, rotation %d" % key
    return want, shares


@pytest.mark.gpu
def test_both_shadow_traces_alpha_test_the_fixture_blocks(shadow, fields, golden, ashadow):
    s, sd, depth = _shadow_scene()
    want, shares = shadow_conditions(ashadow, s, sd, depth, shadow.tset, _alpha_blocks(fields, golden))
    print("shadow trace: %d rays stopped, %d let through or past; rejected shares BC7 %.3f BC2 %.3f BC3 %.3f" %
          ((int((want == 0).sum()), int((want == 255).sum())) + tuple(shares)))
    got = BG._masks_equal("fixture walls", shadow, sd, depth)
    STG._report("fixture walls against the restatement", got, want)
