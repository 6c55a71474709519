"""The material textures on the MI355X: nv_texture_decode against the bytes of niagara's decoder (tests/golden/textures/bc_blocks.npz)
and against nv_texture_decode_host, nv_visibility_attributes_textured against tests/texture_ref.c — attribute records and totals bit for bit,
gbuffer1 bit for bit where no level of detail enters and within one code otherwise, gbuffer0 within one code per channel with at least 90 %
of the channels equal (pow and log2 are correctly rounded on neither side) — the second grid trip, missing and out-of-range textures,
non-finite texcoords, a captured graph and the pipeline's entry.  Outputs are poisoned before every launch; texel buffers carry canaries."""
import os

import numpy as np
import pytest

import oracle
import pixel_cases as PC
import raster_ref as RR
import shade_cases as SC
import texture_ref as TR
import visattr_ref as VA
import visbuffer_ref as VB
from niagara_amd import host, synth
from niagara_amd import layouts as L

HERE = os.path.dirname(os.path.abspath(__file__))
POISON, POISON32 = 0x5A, 0x5A5A5A5A
CANARY = 0x7E57C0DE
DXGI = {1: 71, 2: 74, 3: 77, 7: 98}
FRAMES = 2


@pytest.fixture(scope="module")
def tref(tmp_path_factory):
    return TR.load(tmp_path_factory.mktemp("texture_ref_gpu"))


@pytest.fixture(scope="module")
def aref(tmp_path_factory):
    return VA.load(tmp_path_factory.mktemp("visattr_ref_tex_gpu"))


@pytest.fixture(scope="module")
def vref(tmp_path_factory):
    return VB.load(tmp_path_factory.mktemp("visbuffer_ref_tex_gpu"))


@pytest.fixture(scope="module")
def rref(tmp_path_factory):
    return RR.load(tmp_path_factory.mktemp("raster_ref_tex_gpu"))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "textures", "bc_blocks.npz"))


@pytest.fixture(scope="module")
def ctx():
    from niagara_amd import pipeline as P
    c = P.Context()
    yield c
    c.close()


# ---- decode

def _dds(fmt, width, height, levels, blocks):
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1)
    assert len(blocks) == TR.image_size_bc(width, height, levels, TR.BLOCK_BYTES[fmt])[0]
    return TR.dds_header(DXGI[fmt], width, height, levels, dx10=True) + blocks.tobytes()


def _decode_with_canaries(ctx, files, gap=5):
    """nv_texture_decode of every file into ONE poisoned buffer whose textures are `gap` canary words apart (and `gap` from both ends):
    (descs, texels as uint32 host array); asserts the canaries"""
    import ctypes as C
    import torch
    from niagara_amd import pipeline as P
    from niagara_amd._lib import TextureDesc, check, lib
    descs, words, infos = host.texture_set_layout(files)
    descs = descs.copy()
    for i in range(1, len(descs)):
        descs[i]["offset"] += gap * i
    total = words + gap * (len(files) + 1)
    start = np.full(total, CANARY, np.uint32)
    texels = torch.from_numpy(start.view(np.int32).copy()).to(ctx.device)
    keep = []
    for i, data in enumerate(files):
        info = infos[i]
        blocks = P.to_device(np.frombuffer(data, np.uint8)[info.payloadOffset:].copy(), ctx.device)
        keep.append(blocks)
        d = TextureDesc(*[int(descs[i + 1][k]) for k in ("offset", "width", "height", "levels")])
        check(lib.nv_texture_decode(ctx.h, P._stream(), P._ptr(blocks), info.format, info.width, info.height, info.levels, P._ptr(texels), C.byref(d)),
              "nv_texture_decode")
    ctx.status()
    got = texels.cpu().numpy().view(np.uint32).copy()
    inside = np.zeros(total, bool)
    for d in descs[1:]:
        inside[int(d["offset"]):int(d["offset"]) + TR.chain_words(int(d["width"]), int(d["height"]), int(d["levels"]))] = True
    assert (got[~inside] == CANARY).all(), "a word outside every chain was written"
    return descs, got


@pytest.mark.gpu
@pytest.mark.parametrize("name,fmt", [("bc1", 1), ("bc2", 2), ("bc3", 3), ("bc7", 7)])
def test_device_decode_equals_the_fixture_and_the_host(name, fmt, ctx, golden):
    blocks, want = golden[name], golden[name + "_rgba"]
    n = len(blocks)
    rng = np.random.default_rng(fmt)
    chain20 = blocks[rng.integers(0, n, 25)]  # 20 x 12 with its full chain: 15 + 6 + 2 + 1 + 1 blocks
    files = [_dds(fmt, 4 * n, 4, 1, blocks),       # the whole fixture, one block per column of blocks
             _dds(fmt, 4, 4, 1, blocks[:1]),       # one block
             _dds(fmt, 20, 12, 5, chain20),        # partial blocks, the 2 x 1 and 1 x 1 tail
             _dds(fmt, 4, 4 * 40, 1, blocks[:40])]  # one block per row of blocks
    descs, got = _decode_with_canaries(ctx, files)
    at = lambda i: got[int(descs[i]["offset"]):int(descs[i]["offset"]) + TR.chain_words(*[int(descs[i][k]) for k in ("width", "height", "levels")])]
    strip = np.ascontiguousarray(at(1).reshape(4, n, 4).transpose(1, 0, 2)).reshape(n, 16).view(np.uint8).reshape(n, 64)
    assert strip.tobytes() == want.tobytes()
    assert at(2).view(np.uint8).tobytes() == want[0].tobytes()
    assert at(4).view(np.uint8).reshape(40, 64).tobytes() == want[:40].tobytes()
    hdescs, htexels = host.texture_decode_host(files)
    for i in range(1, 5):
        words = TR.chain_words(*[int(hdescs[i][k]) for k in ("width", "height", "levels")])
        assert at(i).tobytes() == htexels[int(hdescs[i]["offset"]):int(hdescs[i]["offset"]) + words].tobytes(), i
    assert len(at(3)) == 240 + 60 + 15 + 2 + 1


# ---- scenes of the textured pass

def _texture_files(rng):
    """textures 1..5: 64 x 64 with 7 levels (BC7), 20 x 12 with 5 (BC3), 1 x 1 (BC1), 8 x 8 single level (BC2), 64 x 64 with 7 (BC1, a smooth image)"""
    def rand(fmt, w, h, levels):
        b = rng.integers(0, 256, TR.image_size_bc(w, h, levels, TR.BLOCK_BYTES[fmt])[0], dtype=np.uint8)
        if fmt == 7:
            b[0::16] |= 1 << 6
        return _dds(fmt, w, h, levels, b)
    return [rand(7, 64, 64, 7), rand(3, 20, 12, 5), rand(1, 1, 1, 1), rand(2, 8, 8, 1), synth.dds_bytes(synth.texture_images(64)[1])]


_SETS = {}


def _texture_set(ctx):
    """(files, descs host, table device, texels device, texels host): decoded once on the device; equal to the host decode"""
    if "set" not in _SETS:
        from niagara_amd import pipeline as P
        files = _texture_files(np.random.default_rng(23))
        descs, texels = ctx.texture_decode(files)
        ctx.status()
        hdescs, htexels = host.texture_decode_host(files)
        got = texels.cpu().numpy().view(np.uint32)
        assert descs.tobytes() == hdescs.tobytes() and got[:len(htexels)].tobytes() == htexels.tobytes()
        _SETS["set"] = (files, descs, P.to_device(descs, ctx.device), texels, htexels)
    return _SETS["set"]


def _poisoned(ctx, n):
    import torch
    dev = ctx.device
    return dict(attributes=torch.full((n * 64,), POISON, dtype=torch.uint8, device=dev), gbuffer0=torch.full((n,), POISON32, dtype=torch.int32, device=dev),
                gbuffer1=torch.full((n,), POISON32, dtype=torch.int32, device=dev), totals=torch.zeros(4, dtype=torch.int64, device=dev))


def _host(out):
    from niagara_amd import pipeline as P
    g = lambda t: t.cpu().numpy().view(np.uint32).reshape(-1).copy()
    return dict(attributes=P.from_device(out["attributes"], L.PIXELATTR).copy(), gbuffer0=g(out["gbuffer0"]), gbuffer1=g(out["gbuffer1"]),
                totals=out["totals"].cpu().numpy().view(np.uint64).copy())


def _textured(ctx, s, records, w, h, table, count, texels, texel_words, out=None, dev=None):
    """one launch of nv_visibility_attributes_textured over exactly-sized device buffers into poisoned outputs"""
    from niagara_amd import pipeline as P
    out = out or _poisoned(ctx, w * h)
    t = dev or [P.to_device(s[k], ctx.device) for k in ("draws", "meshlets", "data", "vertices", "materials")] + [P.to_device(records, ctx.device)]
    ctx.visibility_attributes_textured(s["g"], t[5], w, h, t[0], len(s["draws"]), t[1], len(s["meshlets"]), t[2], len(s["data"]), t[3], len(s["vertices"]),
                                       t[4], len(s["materials"]), out["attributes"], out["gbuffer0"], out["gbuffer1"], out["totals"], table, count, texels,
                                       texel_words)
    return out, t


def _channels(words, bits):
    out, at = [], 0
    for b in bits:
        out.append((words >> np.uint32(at)) & np.uint32((1 << b) - 1))
        at += b
    return np.stack(out, -1).astype(np.int64)


def _same(name, got, want, descs, materials):
    """the issue's comparison"""
    assert got["totals"].tolist() == want["totals"].tolist(), (got["totals"], want["totals"])
    a, b = got["attributes"].view(np.uint32).reshape(-1, 16), want["attributes"].view(np.uint32).reshape(-1, 16)
    bad = np.nonzero((a != b).any(axis=1))[0]
    assert len(bad) == 0, "attribute records differ at %d pixels; first %s" % (len(bad), bad[:8])
    _same_gbuffers(name, got, want, descs, materials)


def _same_gbuffers(name, got, want, descs, materials):
    shaded = (want["flags"] & VA.SHADED) != 0
    assert (got["gbuffer0"][~shaded] == 0).all() and (got["gbuffer1"][~shaded] == 0).all()
    # gbuffer1: bit for bit for single-level textures (no level of detail: no log2) and for pixels without a normal map, within one code otherwise
    single = np.array([all(t == 0 or t >= len(descs) or descs[t]["levels"] == 1 for t in (m["albedoTexture"], m["normalTexture"], m["specularTexture"],
                                                                                          m["emissiveTexture"])) for m in materials])
    no_nmap = shaded & ((want["flags"] & TR.NORMAL_MAPPED) == 0)
    exact = shaded & (single[want["attributes"]["materialIndex"]] | no_nmap)
    c1, r1 = _channels(got["gbuffer1"], (10, 10, 10, 2)), _channels(want["gbuffer1"], (10, 10, 10, 2))
    assert (got["gbuffer1"][exact] == want["gbuffer1"][exact]).all()
    assert np.abs(c1 - r1).max() <= 1
    c0, r0 = _channels(got["gbuffer0"][shaded], (8, 8, 8, 8)), _channels(want["gbuffer0"][shaded], (8, 8, 8, 8))
    print("%s: gbuffer0 %d channels, %.2f %% equal, largest difference %d; gbuffer1 %.2f %% of the words equal, largest difference %d; %d pixels exact by rule" %
          (name, c0.size, 100 * (c0 == r0).mean(), int(np.abs(c0 - r0).max()), 100 * (got["gbuffer1"][shaded] == want["gbuffer1"][shaded]).mean(),
           int(np.abs(c1 - r1).max()), int(exact.sum())))
    assert np.abs(c0 - r0).max() <= 1
    assert (c0 == r0).mean() >= 0.9


def _plane_scene(rref):
    """a tilted tessellated plane at 160 x 96 under one draw: u runs 1.5 repeats across it (crossing 0 and 1), v 40 t^3 along it — from a
    magnified near edge to more than a repeat per pixel at the far edge; every draw pixel names material 1, whose four textures are 64 x 64 with 7 levels"""
    k = np.arange(17)
    x, y = np.meshgrid(k, k)
    x, y = x.reshape(-1) / 16.0, y.reshape(-1) / 16.0
    pos = np.stack([x - 0.5, y - 0.5, np.zeros_like(x)], -1)
    tris = []
    for j in range(16):
        for i in range(16):
            a = j * 17 + i
            tris += [(a, a + 1, a + 18), (a, a + 18, a + 17)]
    draws = np.zeros(1, L.MESHDRAW)
    ang = np.deg2rad(-78.0) / 2
    draws["position"], draws["scale"], draws["orientation"] = (0.0, -1.2, -9.0), 16.0, (np.sin(ang), 0.0, 0.0, np.cos(ang))
    draws["materialIndex"] = 1
    s = RR.mesh_scene(pos, tris, (160, 96), draws=draws, flags=dict(postPass=1))
    v = VA.fill_attributes(s["vertices"], s["meshlets"], s["data"])
    uv = np.stack([1.5 * x - 0.25, 40.0 * y ** 3], -1).astype(np.float16)
    v["tu"], v["tv"] = uv[:, 0].view(np.uint16), uv[:, 1].view(np.uint16)
    s["vertices"] = v
    m = VA.make_materials()
    m[1]["albedoTexture"], m[1]["normalTexture"], m[1]["specularTexture"], m[1]["emissiveTexture"] = 1, 5, 1, 5
    s["materials"] = m
    # the records: the reference rasteriser's visibility words, decoded (slot -> command, meshlet; one draw)
    _, vis, _ = rref.raster(*RR.raster_args(s), 160, 96, visibility=True)
    vis = vis.reshape(-1)
    slot, tri = (vis >> np.uint64(7)).astype(np.uint32) & np.uint32((1 << 25) - 1), (vis & np.uint64(127)).astype(np.uint32)
    cmd = s["cib"][slot]
    rec = np.zeros(len(vis), L.VISRECORD)
    rec["drawId"] = np.where(vis != 0, s["commands"]["drawId"][cmd & 0xFFFFFF], PC.NONE)
    rec["meshletIndex"] = np.where(vis != 0, s["commands"]["taskOffset"][cmd & 0xFFFFFF] + (cmd >> 24), 0)
    rec["triangle"] = np.where(vis != 0, tri, 0)
    rec["depthBits"] = (vis >> np.uint64(32)).astype(np.uint32)
    assert (vis != 0).sum() > 3000
    return s, rec


def _occluder_scene(vref, aref):
    if "occluder" in _SETS:
        return _SETS["occluder"]
    s = synth.with_textures(VA.with_attributes(synth.occluder_scene(meshlet_bounds=oracle.meshlet_bounds)))
    rec, _ = VA.reference_frame(s, 0, vref, aref, frames=FRAMES)
    s["g"] = RR.globals_for(s["cull"], s["viewport"])
    _SETS["occluder"] = (s, rec)
    return s, rec


def _reference(tref, s, records, w, h, descs, texels, **kw):
    return tref.attributes(s["g"], records, w, h, s["draws"], s["meshlets"], s["data"], s["vertices"], s["materials"], descs, texels, **kw)


@pytest.mark.gpu
def test_textured_plane_equals_the_restatement_over_every_level_and_the_wrap(ctx, tref, rref):
    files, descs, table, texels, htexels = _texture_set(ctx)
    s, rec = _plane_scene(rref)
    tref.hits()
    want = _reference(tref, s, rec, 160, 96, descs, htexels)
    hits = tref.hits()
    uv = want["attributes"]["uv"][(want["flags"] & VA.SHADED) != 0]
    print("plane: samples per level %s, with a fraction %d; u in [%.2f, %.2f], v in [%.2f, %.2f]" %
          (hits[:7].tolist(), int(hits[15]), uv[:, 0].min(), uv[:, 0].max(), uv[:, 1].min(), uv[:, 1].max()))
    assert (hits[:7] > 0).all() and hits[15] > 0, "a level of the 64 x 64 textures is never selected"
    assert uv[:, 0].min() < 0 and uv[:, 0].max() > 1 and uv[:, 1].max() > 5, "the wrap is not crossed"
    assert want["totals"][3] == 0 and tref.bad_indices() == 0
    out, _ = _textured(ctx, s, rec, 160, 96, table, len(descs), texels, len(htexels))
    ctx.status()
    _same("plane", _host(out), want, descs, s["materials"])


@pytest.mark.gpu
def test_textured_occluder_scene_equals_the_restatement_and_untextured_without_a_table(ctx, tref, vref, aref):
    from niagara_amd import pipeline as P
    s, frame = _occluder_scene(vref, aref)
    rec = frame["resolve"]["records"]
    w, h = s["viewport"]
    assert (w, h) == (320, 192)
    sdescs, stexels = host.texture_decode_host(s["textures"])
    ddescs, dtexels = ctx.texture_decode(s["textures"])
    assert dtexels.cpu().numpy().view(np.uint32)[:len(stexels)].tobytes() == stexels.tobytes()
    want = _reference(tref, s, rec, w, h, sdescs, stexels)
    # every material of with_textures names the four maps: every shaded pixel samples them, the normal map included
    assert want["totals"][0] > 20000 and want["totals"][3] == 0
    assert ((want["flags"] & TR.NORMAL_MAPPED) != 0).sum() == want["totals"][0]
    out, dev = _textured(ctx, s, rec, w, h, P.to_device(ddescs, ctx.device), len(ddescs), dtexels, len(stexels))
    ctx.status()
    _same("occluder", _host(out), want, sdescs, s["materials"])
    # no table: nv_visibility_attributes' bytes, every output
    bare, _ = _textured(ctx, s, rec, w, h, None, 0, None, 0, dev=dev)
    plain = _poisoned(ctx, w * h)
    ctx.visibility_attributes(s["g"], dev[5], w, h, dev[0], len(s["draws"]), dev[1], len(s["meshlets"]), dev[2], len(s["data"]), dev[3], len(s["vertices"]),
                              dev[4], len(s["materials"]), plain["attributes"], plain["gbuffer0"], plain["gbuffer1"], plain["totals"])
    ctx.status()
    a, b = _host(bare), _host(plain)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a) and a["totals"][3] > 0
    assert (a["gbuffer0"] != _host(out)["gbuffer0"]).any()  # and the textures do change the picture


@pytest.mark.gpu
@pytest.mark.parametrize("path", SC.FIXTURES, ids=SC.FIXTURE_IDS)
def test_fixture_of_the_reference_fragment_shader_replays_textured(path, ctx, tref):
    """tests/golden/shade: records of one scene and the attachments the reference's own mesh.frag.glsl, run on the CPU, writes for them with
    the restatement's taps (tests/test_shade_fixtures_cpu.py holds the restatement to them bit for bit).  _same's rule, unchanged."""
    from niagara_amd import pipeline as P
    f = np.load(path)
    w, h = SC.fixture_size(f)
    s, rec = SC.fixture_frag_scene(path, f)
    files, hdescs, htexels = SC.frag_textures()
    want = _reference(tref, s, rec, w, h, hdescs, htexels)
    assert want["totals"][3] == 0 and tref.bad_indices() == 0
    want["gbuffer0"], want["gbuffer1"] = f["fragtex_gbuffer0"], f["fragtex_gbuffer1"]  # the expectation is the reference's
    descs, texels = ctx.texture_decode(files)
    assert texels.cpu().numpy().view(np.uint32)[:len(htexels)].tobytes() == htexels.tobytes()
    out, _ = _textured(ctx, s, rec, w, h, P.to_device(descs, ctx.device), len(descs), texels, len(htexels))
    ctx.status()
    _same("fixture %dx%d" % (w, h), _host(out), want, hdescs, s["materials"])


# ---- edges

def _cus(ctx):
    import torch
    return torch.cuda.get_device_properties(ctx.device).multi_processor_count


@pytest.mark.gpu
def test_textured_pass_takes_its_second_trip_with_missing_textures(ctx, tref):
    """2051 x (CUs + 1) pixels of random runs over pixel_cases.attr_scene: material 2 names textures 3, 4 and 7 — 7 is past the table of six, so
    its pixels are shaded from the factors where the texture is missing and counted; material 3 is given index == textureCount and 0xFFFFFFFF"""
    files, descs, table, texels, htexels = _texture_set(ctx)
    cus = _cus(ctx)
    w, h, n = PC.second_trip_sizes(cus)["pixel"]
    g = PC.check_second_trip(n, w, h, cus)
    s = PC.attr_scene((w, h))
    m = s["materials"].copy()
    m[3]["albedoTexture"], m[3]["specularTexture"], m[3]["normalTexture"] = len(descs), 0xFFFFFFFF, 2
    m[0]["albedoTexture"], m[0]["emissiveTexture"] = 5, 1
    s["materials"] = m
    rec = PC.random_records(s, n, 11)
    want = _reference(tref, s, rec, w, h, descs, htexels)
    assert 0 < want["totals"][3] < want["totals"][0] and tref.bad_indices() == 0
    out, _ = _textured(ctx, s, rec, w, h, table, len(descs), texels, len(htexels))
    ctx.status()
    got = _host(out)
    raw = got["attributes"].view(np.uint32).reshape(n, 16)
    assert (raw[g:] != POISON32).any(), "nothing of the second trip was written"
    _same("second trip", got, want, descs, m)


@pytest.mark.gpu
def test_runs_of_one_triangle_across_materials_through_the_textured_pass(ctx, tref):
    """pixel_cases.run_edge_cases, groups b (consecutive runs one word apart) and c (a boundary at every listed lane), through the TEXTURED
    kernel: the pair ((1, 0, 5), (2, 0, 5)) is one meshlet and triangle under two draws — adjacent runs that share the triangle and differ
    in the material, whose textures differ.  Asserted on the host before anything is launched."""
    files, descs, table, texels, htexels = _texture_set(ctx)
    s = PC.attr_scene((64, 48))
    assert s["draws"]["materialIndex"].tolist() == [3, 0, 2]
    m = s["materials"].copy()
    for index, tex in ((0, (1, 5, 4, 2)), (2, (5, 0, 1, 3)), (3, (2, 1, 0, 0))):  # draws 1, 2 and 0
        m[index]["albedoTexture"], m[index]["normalTexture"], m[index]["specularTexture"], m[index]["emissiveTexture"] = tex
    s["materials"] = m
    cases = PC.run_edge_cases(s)
    images = cases["b"] + cases["c"]
    crossings = 0
    for image in images:
        lane, start, diff, named, key = PC.run_starts(image)
        valid = named & (key[:, 0] < len(s["draws"]))
        mat = np.where(valid, s["draws"]["materialIndex"][np.minimum(key[:, 0], len(s["draws"]) - 1)], -1)
        cross = np.zeros(len(key), bool)
        cross[1:] = (diff[1:] == 1) & valid[1:] & valid[:-1] & (mat[1:] != mat[:-1])  # only the drawId differs: same meshlet, same triangle
        names = lambda i: tuple(int(m[mat[i]][k]) for k in ("albedoTexture", "normalTexture", "specularTexture", "emissiveTexture"))
        assert all(names(i) != names(i - 1) for i in np.nonzero(cross)[0])
        crossings += int(cross.sum())
        image["crossings"] = np.nonzero(cross)[0]
    assert crossings >= 12 * 3, crossings  # group c alone: the pair at each of the 12 listed lanes, and group b's runs of 1, 2, 3
    on_lanes = {int(i % 64) for image in images for i in image["crossings"]}
    assert set(PC.BOUNDARIES) <= on_lanes
    for image in images:
        w, h, rec = image["width"], image["height"], image["records"]
        si = PC.attr_scene((w, h))  # (the scene under the image's own viewport)
        si["materials"] = m
        want = _reference(tref, si, rec, w, h, descs, htexels)
        out, _ = _textured(ctx, si, rec, w, h, table, len(descs), texels, len(htexels))
        ctx.status()
        got = _host(out)
        _same(image["name"], got, want, descs, m)
        at = image["crossings"]
        if len(at):  # the two sides of a crossing are the same triangle at neighbouring pixels and do not carry the same words
            assert (want["gbuffer0"][at] != want["gbuffer0"][at - 1]).any()
    assert tref.bad_indices() == 0


@pytest.mark.gpu
def test_descriptor_one_word_past_the_buffer_is_not_sampled(ctx, tref):
    """texelWords one short of the set: the last texture's chain ends one word past it — treated as absent, counted, shaded from the factors;
    the texel buffer's tail canary keeps its bytes (nothing writes it) and the restatement forms no index outside the shortened buffer"""
    import torch
    files, descs, table, texels, htexels = _texture_set(ctx)
    s = PC.attr_scene((64, 48))
    m = s["materials"].copy()
    last = len(descs) - 1
    m[0]["albedoTexture"], m[3]["normalTexture"], m[2]["albedoTexture"], m[2]["normalTexture"], m[2]["emissiveTexture"] = last, last, 1, 0, 0
    s["materials"] = m
    rec = PC.random_records(s, 64 * 48, 12)
    words = len(htexels) - 1
    guarded = torch.cat([texels[:len(htexels)], torch.full((64,), CANARY, dtype=torch.int32, device=ctx.device)])
    want = _reference(tref, s, rec, 64, 48, descs, htexels, texel_words=words)
    full = _reference(tref, s, rec, 64, 48, descs, htexels)
    assert want["totals"][3] > 0 and full["totals"][3] == 0 and tref.bad_indices() == 0
    out, _ = _textured(ctx, s, rec, 64, 48, table, len(descs), guarded, words)
    ctx.status()
    got = _host(out)
    _same("one word past", got, want, descs, m)
    assert (guarded[len(htexels):].cpu().numpy().view(np.uint32) == CANARY).all()
    # the pixels of the refused texture carry the factors' shading: equal to the pass without any table
    none = _host(_textured(ctx, s, rec, 64, 48, None, 0, None, 0)[0])
    refused = (want["flags"] & TR.NOT_SAMPLED) != 0
    only = refused & np.isin(want["attributes"]["materialIndex"], (0,))
    assert only.any() and (got["gbuffer0"][only] == none["gbuffer0"][only]).all() and (got["gbuffer1"][only] == none["gbuffer1"][only]).all()


@pytest.mark.gpu
def test_non_finite_texcoords_and_small_textures_equal_the_restatement(ctx, tref):
    """pixel_cases.special_scene: uv halves NaN, +-inf, denormal, -0 and 65504-scale positions; material 6 names textures 2 (20 x 12), 5 and 1,
    material 0 the 1 x 1 texture: no index out of range on the restatement's side, the device equals it under §4.13's NaN rule"""
    files, descs, table, texels, htexels = _texture_set(ctx)
    s = PC.special_scene()
    w, h = s["viewport"]
    m = s["materials"].copy()
    m[0]["albedoTexture"], m[0]["specularTexture"], m[1]["emissiveTexture"], m[1]["normalTexture"] = 3, 4, 2, 3
    s["materials"] = m
    with np.errstate(all="ignore"):
        want = _reference(tref, s, s["records"], w, h, descs, htexels)
    assert tref.bad_indices() == 0 and want["totals"][2] > 0 and want["totals"][3] == 0
    out, _ = _textured(ctx, s, s["records"], w, h, table, len(descs), texels, len(htexels))
    ctx.status()
    got = _host(out)
    assert got["totals"].tolist() == want["totals"].tolist()
    n = w * h
    a, b = got["attributes"].view(np.uint32).reshape(n, 16).copy(), want["attributes"].view(np.uint32).reshape(n, 16).copy()
    is_float = np.ones(16, bool)
    is_float[[L.PIXELATTR.fields["drawId"][1] // 4, L.PIXELATTR.fields["materialIndex"][1] // 4]] = False
    nan_want, nan_got = np.isnan(b.view(np.float32)) & is_float, np.isnan(a.view(np.float32)) & is_float
    assert nan_want.any() and (nan_got == nan_want).all()  # §4.13: a NaN where the restatement has one; sign and payload are not compared
    a[nan_want], b[nan_want] = 0, 0
    assert (a == b).all()
    # the G-buffer words by the rule of every other test here, over ALL shaded pixels: an infinite channel clamps to the same end code on both
    # sides; material 0 names single-level textures only, so its gbuffer1 words are bit-identical
    _same_gbuffers("special values", got, want, descs, m)
    c1, c0 = _channels(got["gbuffer1"], (10, 10, 10, 2)), _channels(got["gbuffer0"], (8, 8, 8, 8))
    # a NaN channel packs to code 0 on both sides (pow of a negative base and log2 of a non-positive value are NaN on both)
    nan = np.isnan(want["chan"]) & ((want["flags"] & VA.SHADED) != 0)[:, None]
    assert nan.any()
    both = np.concatenate([c0, c1], axis=1)
    assert (both[nan] == 0).all()


# ---- captured graph, pipeline

@pytest.mark.gpu
def test_decode_and_textured_attributes_replay_from_a_graph(ctx, tref):
    import ctypes as C
    import torch
    from niagara_amd import pipeline as P
    from niagara_amd._lib import TextureDesc, check, lib
    files, descs, table, texels, htexels = _texture_set(ctx)
    s = PC.attr_scene((96, 64))
    m = s["materials"].copy()
    m[0]["albedoTexture"], m[3]["normalTexture"], m[2]["emissiveTexture"] = 5, 1, 2
    s["materials"] = m
    rec = PC.random_records(s, 96 * 64, 13)
    want = _host(_textured(ctx, s, rec, 96, 64, table, len(descs), texels, len(htexels))[0])
    ctx.status()
    infos = host.texture_set_layout(files)[2]
    blocks = [P.to_device(np.frombuffer(f, np.uint8)[infos[i].payloadOffset:].copy(), ctx.device) for i, f in enumerate(files)]
    fresh = torch.full((len(htexels),), POISON32, dtype=torch.int32, device=ctx.device)
    out = _poisoned(ctx, 96 * 64)
    dev = [P.to_device(s[k], ctx.device) for k in ("draws", "meshlets", "data", "vertices", "materials")] + [P.to_device(rec, ctx.device)]

    def step():
        for i in range(len(files)):
            d = TextureDesc(*[int(descs[i + 1][k]) for k in ("offset", "width", "height", "levels")])
            check(lib.nv_texture_decode(ctx.h, P._stream(), P._ptr(blocks[i]), infos[i].format, infos[i].width, infos[i].height, infos[i].levels,
                                        P._ptr(fresh), C.byref(d)), "nv_texture_decode")
        _textured(ctx, s, rec, 96, 64, table, len(descs), fresh, len(htexels), out=out, dev=dev)

    def reset():
        fresh.fill_(POISON32)
        for k in ("attributes", "gbuffer0", "gbuffer1"):
            out[k].fill_(POISON if k == "attributes" else POISON32)
        out["totals"].zero_()

    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        reset()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            step()
        torch.cuda.synchronize()
        assert (out["gbuffer0"] == POISON32).all() and (fresh == POISON32).all()  # nothing ran during capture
        for _ in range(2):
            reset()
            graph.replay()
            torch.cuda.synchronize()
            got = _host(out)
            assert all(got[k].tobytes() == want[k].tobytes() for k in want)
            assert fresh.cpu().numpy().view(np.uint32).tobytes() == htexels.tobytes()
    ctx.status()


@pytest.mark.gpu
def test_pipeline_set_textures_attributes_and_shade(tref, vref, aref, tmp_path_factory):
    import shade_ref as SR
    from niagara_amd import pipeline as P
    from niagara_amd._lib import NvError
    sref = SR.load(tmp_path_factory.mktemp("shade_ref_tex_gpu"))
    s, frame = _occluder_scene(vref, aref)
    w, h = s["viewport"]
    kw = dict(task_capacity=4096, cluster_capacity=4096 * 64, fused=True, vertices=s["vertices"], meshlet_data=s["data"], near_clip=False, stable_ids=True)
    pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], (w, h), **kw)
    try:
        vis = pipe.new_visibility()
        for _ in range(FRAMES):
            pipe.frame(s["cull"], post_pass=True, visibility=vis)
        res = pipe.resolve(s["cull"], vis)
        assert P.from_device(res["records"], L.VISRECORD).tobytes() == frame["resolve"]["records"].tobytes()
        with pytest.raises(NvError, match="set_textures"):
            pipe.attributes(s["cull"], res["records"], s["materials"], textures=True)
        path = tmp_path_factory.mktemp("dds") / "albedo.dds"
        path.write_bytes(s["textures"][0])
        pipe.set_textures([str(path)] + s["textures"][1:])  # a path and file images
        att = pipe.attributes(s["cull"], res["records"], s["materials"], textures=True)
        pipe.ctx.status()
        sdescs, stexels = host.texture_decode_host(s["textures"])
        want = _reference(tref, s, frame["resolve"]["records"], w, h, sdescs, stexels)
        got = dict(attributes=P.from_device(att["attributes"], L.PIXELATTR).copy(), gbuffer0=att["gbuffer0"].cpu().numpy().view(np.uint32).reshape(-1),
                   gbuffer1=att["gbuffer1"].cpu().numpy().view(np.uint32).reshape(-1), totals=att["totals"].cpu().numpy().view(np.uint64))
        _same("pipeline", got, want, sdescs, s["materials"])
        camera, sun = (0.0, 0.0, 0.0), np.array([0.35, 0.6, 0.72]) / np.linalg.norm([0.35, 0.6, 0.72])
        color = pipe.shade(s["cull"], att["gbuffer0"], att["gbuffer1"], camera, sun, shadow=None)
        pipe.ctx.status()
        depth = pipe.depth.cpu().numpy()
        sd = host.build_shade_data(synth.make_globals(s["cull"], (w, h)), camera, sun, 0, w, h)
        ref_color = sref.shade(sd, want["gbuffer0"].reshape(h, w), want["gbuffer1"].reshape(h, w), depth, shadow=None, znear=float(s["cull"]["znear"][0]))
        c = SR.channels(color.cpu().numpy().view(np.uint32))
        d = np.abs(c - SR.channels(ref_color))
        print("pipeline colour: %d channels, %d differ, largest difference %d" % (d.size, int((d != 0).sum()), int(d.max())))
        assert d.max() <= 1 and (c[..., 3] == 255).all()
    finally:
        pipe.ctx.close()


@pytest.mark.gpu
def test_sharded_pipeline_refuses_set_textures():
    from niagara_amd import pipeline as P
    from niagara_amd._lib import NvError
    s = synth.with_textures(VA.with_attributes(synth.occluder_scene(meshlet_bounds=oracle.meshlet_bounds)))
    kw = dict(task_capacity=4096, cluster_capacity=4096 * 64, fused=True, vertices=s["vertices"], meshlet_data=s["data"], stable_ids=True)
    pipe = P.ShardedVisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], rank=0, world=1, **kw)
    try:
        with pytest.raises(NvError, match="set_textures"):
            pipe.set_textures(s["textures"])
    finally:
        pipe.ctx.close()


# ---- the code objects

@pytest.mark.parametrize("source,kernel", [("texdecode", "texture_decode_kernel"), ("visattr_tex", "visibility_attributes_kernelILb1ELb1E")])
def test_new_kernels_use_no_scratch_memory(source, kernel, tmp_path):
    """the kernel's metadata as the compiler writes it (the Makefile's flags): 0 bytes of private segment, no spilled vector register"""
    import subprocess
    csrc = os.path.join(os.path.dirname(HERE), "niagara_amd", "csrc")
    asm = str(tmp_path / (source + ".s"))
    subprocess.check_call(["hipcc", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize", "--offload-arch=gfx950", "--cuda-device-only",
                           "-S", os.path.join(csrc, source + ".hip"), "-o", asm], stderr=subprocess.DEVNULL)
    text = open(asm).read()
    entry = [e for e in text[text.index("amdhsa.kernels:"):].split("\n  - .")[1:] if kernel in e.split(".name:")[1].split()[0]]
    assert len(entry) == 1, "kernel metadata not found"
    field = lambda name: int(entry[0].split("." + name + ":")[1].split()[0])
    print("%s: %d VGPRs, %d SGPRs, %d bytes LDS, %d bytes scratch" % (kernel, field("vgpr_count"), field("sgpr_count"), field("group_segment_fixed_size"),
                                                                     field("private_segment_fixed_size")))
    assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0
