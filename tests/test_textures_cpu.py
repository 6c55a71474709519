"""The material textures on the CPU: texmath.h's block decode (through nv_texture_decode_host) and tests/texture_ref.c's
against the bytes of niagara's decoder (tests/golden/textures/bc_blocks.npz), the DDS accept / reject table of loadImage, level offsets, the software
sampler against the restatement (bit for bit where the level of detail clamps to 0, within the derived bound of the fp64 build otherwise),
wrap and level-selection cases, non-finite coordinates, and the texture paths of a scene cache."""
import os

import numpy as np
import pytest

import texture_ref as TR
from niagara_amd import host, synth
from niagara_amd import layouts as L
from niagara_amd._lib import NvError

HERE = os.path.dirname(os.path.abspath(__file__))
DXGI = {1: (71, 72), 2: (74, 75), 3: (77, 78), 4: (80, 81), 5: (83, 84), 6: (95, 96), 7: (98, 99)}
U = 2.0 ** -24


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return TR.load(tmp_path_factory.mktemp("texture_ref_cpu"))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "textures", "bc_blocks.npz"))


def _strip(fmt, blocks):
    """n blocks as a (4 n) x 4 texture of one level: (DDS file image, function that turns its texels back into (n, 64) bytes)"""
    n = len(blocks)
    data = TR.dds_header(DXGI[fmt][0], 4 * n, 4, 1, dx10=True) + np.ascontiguousarray(blocks).tobytes()
    return data, lambda t: np.ascontiguousarray(t.reshape(4, n, 4).transpose(1, 0, 2)).reshape(n, 16).view(np.uint8).reshape(n, 64)


@pytest.mark.parametrize("name,fmt", [("bc1", 1), ("bc2", 2), ("bc3", 3), ("bc7", 7)])
def test_both_decoders_equal_the_reference_decoders_bytes(name, fmt, ref, golden):
    blocks, want = golden[name], golden[name + "_rgba"]
    assert len(blocks) == {"bc1": 256, "bc2": 128, "bc3": 256, "bc7": 8 * 64 + 32}[name]
    if fmt == 7:  # the fixture holds what the issue asks for: every mode, and the reserved mode
        modes = np.array([(int(b[0]) & -int(b[0])).bit_length() - 1 for b in blocks])
        assert [int((modes == m).sum()) for m in range(8)] == [64] * 8 and int((modes == -1).sum()) == 32
        assert not want[modes == -1].any()
    if fmt == 1:
        c = blocks[:, :4].copy().view("<u2")
        assert (c[:, 0] > c[:, 1]).sum() >= 64 and (c[:, 0] < c[:, 1]).sum() >= 64 and (c[:, 0] == c[:, 1]).sum() >= 32
    assert ref.decode_blocks(fmt, blocks).tobytes() == want.tobytes()
    data, back = _strip(fmt, blocks)
    descs, texels = host.texture_decode_host([data])
    assert descs[1].tolist() == (0, 4 * len(blocks), 4, 1)
    assert back(texels).tobytes() == want.tobytes()


# ---- the DDS reader

def _file(fmt=1, width=8, height=8, levels=1, dx10=False, extra=0, **over):
    size = TR.image_size_bc(width, height, levels, 8 if fmt in (1, 4, 80, 81, 71, 72) else 16)[0]
    return TR.dds_header(fmt, width, height, levels, dx10=dx10, **over) + bytes(size + extra if extra >= 0 else max(0, size + extra))


def test_dds_accepts_every_spelling_of_every_format():
    for fmt, four in ((1, "DXT1"), (2, "DXT3"), (3, "DXT5"), (4, "ATI1"), (5, "ATI2")):
        d = host.dds_parse(_file(fmt, 20, 12, 5))
        assert (d["format"], d["width"], d["height"], d["levels"], d["payloadOffset"]) == (fmt, 20, 12, 5, 128), four
        assert d["blockBytes"] == (8 if fmt in (1, 4) else 16)
    for fmt, codes in DXGI.items():
        for code in codes:
            d = host.dds_parse(_file(code, 8, 8, 2, dx10=True))
            assert (d["format"], d["payloadOffset"], d["blockBytes"]) == (fmt, 148, 8 if fmt in (1, 4) else 16), code


@pytest.mark.parametrize("why,data", [
    ("magic", _file(magic=0x20534445)),                              # textures.cpp:168
    ("no header", _file()[:100]),                                     # :172
    ("magic only", _file()[:4]),                                      # :168/172
    ("no DX10 header", _file(98, dx10=True)[:140]),                   # :176
    ("header size", _file(size=120)),                                 # :179
    ("pixel format size", _file(pf_size=24)),                         # :179
    ("cube map", _file(caps2=0x200)),                                 # :182
    ("volume", _file(caps2=0x200000)),                                # :182
    ("DX10 dimension", _file(98, dx10=True, dimension=4)),            # :185
    ("unknown FourCC", _file(fourcc=0x32545844)),                     # :189 "DXT2"
    ("unknown DXGI format", _file(28, dx10=True)),                    # :189 R8G8B8A8
    ("short payload", _file(extra=-1)),                               # :203
    ("bytes behind the payload", _file(extra=1)),                     # :206
    ("no payload", _file()[:128]),                                    # :203
])
def test_dds_rejects_what_loadimage_rejects(why, data):
    with pytest.raises(NvError, match="NV_EFORMAT"):
        host.dds_parse(data)


def test_bc4_bc5_bc6h_parse_and_are_refused_by_the_set():
    ok = _file(1)
    for data in (_file(4), _file(5), _file(80, dx10=True), _file(84, dx10=True), _file(95, dx10=True), _file(96, dx10=True)):
        assert host.dds_parse(data)["format"] in (4, 5, 6)
        with pytest.raises(NvError, match="NV_ETEXFORMAT"):
            host.texture_set_layout([ok, data])
        with pytest.raises(NvError, match="NV_ETEXFORMAT"):
            host.texture_decode_host([data])


@pytest.mark.parametrize("width,height,levels", [(4, 4, 1), (20, 12, 5), (1, 1, 1), (256, 64, 9), (256, 64, 3)])
@pytest.mark.parametrize("fmt", [1, 3])
def test_level_offsets_follow_getimagesizebc(width, height, levels, fmt):
    d = host.dds_parse(_file(fmt, width, height, levels))
    total, offsets = TR.image_size_bc(width, height, levels, 8 if fmt == 1 else 16)
    assert d["payloadBytes"] == total and d["levelOffset"] == offsets
    if (width, height, levels) == (20, 12, 5):
        assert [(max(1, 20 >> l), max(1, 12 >> l)) for l in range(5)] == [(20, 12), (10, 6), (5, 3), (2, 1), (1, 1)]
        assert offsets == [k * (8 if fmt == 1 else 16) for k in (0, 15, 21, 23, 24)]
    descs, words, _ = host.texture_set_layout([_file(fmt, width, height, levels), _file(1, 4, 4, 1)])
    assert descs[0].tolist() == (0, 0, 0, 0)
    assert descs[1].tolist() == (0, width, height, levels)
    assert descs[2].tolist() == (TR.chain_words(width, height, levels), 4, 4, 1) and words == descs[2]["offset"] + 16


# ---- the sampler

def _random_dds(rng, fmt, width, height, levels):
    size = TR.image_size_bc(width, height, levels, TR.BLOCK_BYTES[fmt])[0]
    blocks = rng.integers(0, 256, size, dtype=np.uint8)
    if fmt == 7:
        blocks[0::16] |= 1 << 6  # no reserved blocks: content everywhere
    return TR.dds_header(DXGI[fmt][0], width, height, levels, dx10=True) + blocks.tobytes()


@pytest.fixture(scope="module")
def texset(ref):
    """textures 1..5: 64 x 64 with its 7 levels (BC7), 20 x 12 with 5 (BC3), 1 x 1 (BC1), 8 x 8 single level (BC2), 16 x 4 with 5 (BC1); decoded
    by the library and by the restatement: equal"""
    rng = np.random.default_rng(41)
    files = [_random_dds(rng, 7, 64, 64, 7), _random_dds(rng, 3, 20, 12, 5), _random_dds(rng, 1, 1, 1, 1), _random_dds(rng, 2, 8, 8, 1),
             _random_dds(rng, 1, 16, 4, 5)]
    descs, texels = host.texture_decode_host(files)
    rdescs, rtexels = ref.decode_set(files)
    assert descs.tobytes() == rdescs.tobytes() and texels.tobytes() == rtexels.tobytes()
    return descs, texels


def _lib_samples(descs, texels, tex_id, uv, dx, dy):
    return np.stack([host.texture_sample_host(descs, texels, tex_id, uv[i], dx[i], dy[i]) for i in range(len(uv))])


WRAP = [0.0, 1.0, -0.25, 2.0, -3.0, 7.0, 1.0 - 2.0 ** -11, 65504.0, -65504.0, 0.5, -1e-10, 1e-10, 0.999999, 123.456]


def test_sampler_is_the_restatement_bit_for_bit_where_lambda_is_zero(ref, texset):
    descs, texels = texset
    rng = np.random.default_rng(5)
    grid = np.array([(u, v) for u in WRAP for v in WRAP], np.float32)
    uv = np.concatenate([grid, rng.uniform(-3, 3, (400, 2)).astype(np.float32)])
    zero = np.zeros_like(uv)
    for tex_id in (1, 2, 3, 4, 5):  # zero derivatives: lambda clamps to 0 on every texture
        want, ok = ref.sample(descs, texels, tex_id, uv)
        assert ok.all()
        got = _lib_samples(descs, texels, tex_id, uv, zero, zero)
        assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist(), tex_id
    # single-level textures: any derivative clamps to level 0
    big = rng.uniform(-4, 4, uv.shape).astype(np.float32)
    for tex_id in (3, 4):
        want, _ = ref.sample(descs, texels, tex_id, uv, big, big[::-1])
        got = _lib_samples(descs, texels, tex_id, uv, big, big[::-1].copy())
        assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist(), tex_id
    assert ref.bad_indices() == 0


def test_wrap_crosses_the_border_texels(ref, texset):
    """REPEAT: at uv = 0 (and every integer) the footprint is the LAST and the FIRST texel of the row and column, half each"""
    descs, texels = texset
    d = descs[4]  # 8 x 8, one level; random content: the border texels differ
    t = texels[d["offset"]:d["offset"] + 64].reshape(8, 8)
    px = lambda y, x: np.array([(int(t[y, x]) >> s & 255) / 255.0 for s in (0, 8, 16, 24)])
    assert not np.array_equal(px(0, 0), px(0, 7)) and not np.array_equal(px(0, 0), px(7, 0))
    corner = (px(7, 7) + px(7, 0) + px(0, 7) + px(0, 0)) / 4
    for uv in ((0.0, 0.0), (1.0, 1.0), (-3.0, 7.0), (65504.0, -65504.0)):
        got = host.texture_sample_host(descs, texels, 4, uv)
        assert np.abs(got - corner).max() < 4 * U, uv
    # a CLAMP sampler would return texel (0, 0) alone there
    assert np.abs(host.texture_sample_host(descs, texels, 4, (0.0, 0.0)) - px(0, 0)).max() > 1e-3
    # texel centres: exactly the texel
    for x, y in ((0, 0), (7, 7), (3, 5)):
        got = host.texture_sample_host(descs, texels, 4, ((x + 0.5) / 8, (y + 0.5) / 8))
        assert np.array_equal(got, px(y, x).astype(np.float32))
    # -0.25 is 0.75
    assert np.array_equal(host.texture_sample_host(descs, texels, 4, (-0.25, -0.25)), host.texture_sample_host(descs, texels, 4, (0.75, 0.75)))


def test_minification_by_a_power_of_two_selects_that_level_alone(ref, texset):
    descs, texels = texset
    rng = np.random.default_rng(6)
    for tex_id in (1, 2, 5):
        d = descs[tex_id]
        W, H, levels = int(d["width"]), int(d["height"]), int(d["levels"])
        uv = rng.uniform(-2, 2, (24, 2)).astype(np.float32)
        for k in range(levels + 3):
            dx = np.tile(np.array([2.0 ** k / W, 0.0], np.float32), (len(uv), 1))
            dy = np.tile(np.array([0.0, 2.0 ** k / H], np.float32), (len(uv), 1))
            level = min(k, levels - 1)  # lambda past the last level clamps
            one = descs.copy()  # a descriptor of that level alone
            one[tex_id] = (d["offset"] + TR.chain_words(W, H, level), max(1, W >> level), max(1, H >> level), 1)
            want = _lib_samples(one, texels, tex_id, uv, np.zeros_like(dx), np.zeros_like(dy))
            got = _lib_samples(descs, texels, tex_id, uv, dx, dy)
            assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist(), (tex_id, k)
            # the x derivative alone decides when it is the larger one: H in place of W in rho would pick another level on 20 x 12 and 16 x 4
            got_x = _lib_samples(descs, texels, tex_id, uv, dx, np.zeros_like(dy))
            assert got_x.view(np.uint32).tolist() == want.view(np.uint32).tolist(), (tex_id, k)
            r, _ = ref.sample(descs, texels, tex_id, uv, dx, dy)
            assert got.view(np.uint32).tolist() == r.view(np.uint32).tolist()
    assert ref.bad_indices() == 0


def test_trilinear_lies_within_the_derived_bound_of_the_fp64_build(ref, texset):
    """|fp32 - fp64| <= (3 (W + H) + 32) 2^-24 per channel — 3 W u and 3 H u from the coordinate's roundings (the filter is
    continuous with slope <= 1 per texel), 16 u from lambda's (log2 and the four products; the blend of levels is continuous in lambda), 16 u
    for the fetch and the nine roundings of three nested blends.  Counted, not fitted."""
    descs, texels = texset
    rng = np.random.default_rng(7)
    n = 3000
    uv = rng.uniform(-3, 3, (n, 2)).astype(np.float32)
    scale = (2.0 ** rng.uniform(-9, 1, (n, 1))).astype(np.float32)
    dx, dy = (rng.normal(size=(n, 2)) * scale).astype(np.float32), (rng.normal(size=(n, 2)) * scale).astype(np.float32)
    for tex_id in (1, 2, 5):
        W, H, levels = int(descs[tex_id]["width"]), int(descs[tex_id]["height"]), int(descs[tex_id]["levels"])
        ref.hits("f64")
        r64, _ = ref.sample(descs, texels, tex_id, uv, dx, dy, real="f64")
        hits = ref.hits("f64")
        assert (hits[:levels] > 0).all() and hits[15] > n // 5, hits  # every level is selected, many with a fraction
        r32, _ = ref.sample(descs, texels, tex_id, uv, dx, dy)
        got = _lib_samples(descs, texels, tex_id, uv, dx, dy)
        bound = (3 * (W + H) + 32) * U
        print("texture %d: |lib - f64| max %.3g, |ref32 - f64| max %.3g, bound %.3g; lib == ref32 on %.1f %% of the channels" %
              (tex_id, np.abs(got - r64).max(), np.abs(r32 - r64).max(), bound, 100 * (got.view(np.uint32) == r32.view(np.uint32)).mean()))
        assert np.abs(got - r64).max() <= bound
        assert np.abs(r32 - r64).max() <= bound
    assert ref.bad_indices("f64") == 0 and ref.bad_indices() == 0


def test_non_finite_coordinates_load_nothing_out_of_range(ref, texset):
    """every index the restatement forms is checked against the buffer (its counter stays 0), the library gives the same bits, and a NaN that
    reaches the result is a NaN on both sides (the UNORM pack makes it code 0)"""
    descs, texels = texset
    special = np.array([np.nan, np.inf, -np.inf, 65504.0, -65504.0, 3.4e38, -3.4e38, 1e-45, -1e-45, 0.0, -0.0, 0.3], np.float32)
    uv = np.array([(a, b) for a in special for b in special], np.float32)
    before = ref.bad_indices()
    for tex_id in (1, 2, 3, 5):
        for dx, dy in ((np.zeros_like(uv), np.zeros_like(uv)), (uv[::-1].copy(), uv.copy()), (np.full_like(uv, 0.01), uv.copy())):
            want, ok = ref.sample(descs, texels, tex_id, uv, dx, dy)
            assert ok.all()
            got = _lib_samples(descs, texels, tex_id, uv, dx, dy)
            same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
            levels = int(descs[tex_id]["levels"])
            if levels == 1 or not dx.any():
                assert same.all(), tex_id
            else:  # lambda goes through log2: close, and NaN exactly where the restatement has one
                assert (np.isnan(got) == np.isnan(want)).all()
                assert np.nanmax(np.abs(got - want), initial=0.0) <= 1e-4
    assert ref.bad_indices() == before == 0
    finite = np.isfinite(uv).all(axis=1)
    got = _lib_samples(descs, texels, 1, uv, np.zeros_like(uv), np.zeros_like(uv))
    assert np.isfinite(got[finite]).all() and np.isnan(got[~finite]).all(axis=1).all()


def test_sample_refuses_bad_ids_and_descriptors(texset):
    descs, texels = texset
    for tex_id in (0, len(descs), 0xFFFFFFFF):
        with pytest.raises(NvError, match="NV_EINVAL"):
            host.texture_sample_host(descs, texels, tex_id, (0.5, 0.5))
    for field, value in (("offset", len(texels) - TR.chain_words(64, 64, 7) + 1), ("width", 0), ("height", 16385), ("levels", 0), ("levels", 16),
                         ("offset", 0xFFFFFFFF)):
        bad = descs.copy()
        bad[1][field] = value
        with pytest.raises(NvError, match="NV_EINVAL"):
            host.texture_sample_host(bad, texels, 1, (0.5, 0.5))
    last = descs.copy()  # a chain that ends exactly at the buffer's end is in range
    last[1]["offset"] = len(texels) - TR.chain_words(64, 64, 7)
    host.texture_sample_host(last, texels, 1, (0.5, 0.5), (1.0, 0.0), (0.0, 1.0))


# ---- synth's encoder

def test_synth_dds_round_trips_through_the_reader_and_both_decoders(ref):
    s = synth.with_textures(dict(vertices=np.zeros(3, L.VERTEX), draws=np.zeros(7, L.MESHDRAW)))
    assert len(s["textures"]) == 4 and (s["materials"]["emissiveTexture"] == 4).all() and (s["materials"]["albedoTexture"] == 1).all()
    for data, image in zip(s["textures"], synth.texture_images(64)):
        d = host.dds_parse(data)
        assert (d["format"], d["width"], d["height"], d["levels"]) == (1, 64, 64, 7)
    descs, texels = host.texture_decode_host(s["textures"])
    rdescs, rtexels = ref.decode_set(s["textures"])
    assert descs.tobytes() == rdescs.tobytes() and texels.tobytes() == rtexels.tobytes()
    # the min / max encoder keeps a smooth image within the endpoints' quantisation and a third of the block's range
    for i, image in enumerate(synth.texture_images(64)):
        level0 = texels[descs[i + 1]["offset"]:descs[i + 1]["offset"] + 64 * 64].view(np.uint8).reshape(64, 64, 4)
        assert np.abs(level0[..., :3].astype(int) - image[..., :3].astype(int)).max() <= 64
        assert (level0[..., 3] == 255).all()
    odd = synth.dds_bytes(np.random.default_rng(3).integers(0, 256, (12, 20, 4), dtype=np.uint8))
    assert host.dds_parse(odd)["levels"] == 5 and len(odd) == 128 + 25 * 8
    assert host.dds_parse(synth.dds_bytes(np.zeros((4, 4, 3), np.uint8), mips=False))["levels"] == 1


# ---- the texture paths of a scene cache

def _append_paths(path, paths):
    """tests/scenecache_writer.py writes the path records as junk; this rewrites the file's tail as saveSceneCache does (:192-197)"""
    with open(path, "r+b") as f:
        f.seek(0, 2)
        f.seek(f.tell() - 256 * len(paths))
        for p in paths:
            f.write(os.fsencode(p)[:255].ljust(256, b"\0"))


@pytest.mark.parametrize("paths", [[], ["textures/albedo.dds"], ["a.dds", "dir/" + "x" * 251, "c/normal map.dds"]])
def test_scenecache_texture_paths(paths, tmp_path):
    import scenecache_writer as SW
    meshes, total = synth.make_meshes(2, 2, 10)
    meshlets = synth.make_meshlets(total)
    draws = host.synth_draws(5, 2, 10.0)
    f = str(tmp_path / "scene.cache")
    SW.write_scene_cache(f, meshes, meshlets, draws, texture_paths=len(paths))
    _append_paths(f, paths)
    assert all(len(p) <= 255 for p in paths) and (len(paths) < 3 or len(paths[1]) == 255)
    assert host.scenecache_info(f).texturePathCount == len(paths)
    assert host.scenecache_texture_paths(f) == paths
    if paths:  # a file cut inside the records
        with open(f, "r+b") as fh:
            fh.truncate(host.scenecache_info(f).drawOffset + 100)
        with pytest.raises(NvError):
            host.scenecache_texture_paths(f)
