"""The classic path with textures on the MI355X.

nv_rasterdepth_indexed_textured against tests/raster_indexed_alpha_ref.c: depth, visibility words, d_totals4 and d_alphaTotals2 bit for bit
(§4.20's band rule is not applied: no case here needed it), nv_rasterdepth_indexed_blocks against the decoded entry point bit for bit.
nv_visibility_attributes_indexed_textured against texture_ref.c's fragment statements over the indexed records
(raster_indexed_alpha_ref.attributes) under tests/test_textures_gpu.py's comparison, taken as it stands (_same: records and totals bit for
bit, gbuffer1 within one code and bit for bit without a level of detail, gbuffer0 within one code), the block form bit for bit against the
decoded one.  Then the pipeline's classic frame with textures against the cluster frame on the same device."""
import numpy as np
import pytest

import pixel_cases as PC
import raster_alpha_ref as RA
import raster_indexed_alpha_ref as RIA
import raster_ref as RR
import test_textures_gpu as TG
import test_visindexed_cpu as TC
import test_visindexed_gpu as VG
import test_visindexed_textured_cpu as TCT
from niagara_amd import host
from niagara_amd import layouts as L

POISON = 0x5A
INT_MAX = 2 ** 31 - 1
riaref, tref, viref, iaref = TCT.riaref, TCT.tref, TCT.viref, TCT.iaref  # the restatements' fixtures


@pytest.fixture(scope="module")
def ctx():
    from niagara_amd import pipeline as P
    c = P.Context()
    yield c
    c.close()


def _set(ctx, tex, files=None):
    """the keyword arguments of the set for Context.rasterdepth_indexed_textured (tex: host materials / descs / texels and the count overrides
    of the restatement) or, with `files`, for rasterdepth_indexed_blocks over the block form of those DDS images"""
    from niagara_amd import pipeline as P
    dev = ctx.device
    mats, descs, texels = tex.get("materials"), tex.get("descs"), tex.get("texels")
    kw = dict(materials=None if mats is None else P.to_device(np.ascontiguousarray(mats, L.MATERIAL), dev),
              material_count=tex.get("material_count", 0 if mats is None else len(mats)))
    if files is not None:
        bdescs, hblocks = host.texture_blocks_host(files)
        kw.update(textures=P.to_device(bdescs, dev), texture_count=len(bdescs), blocks=P.to_device(hblocks, dev), units16=len(hblocks) // 16)
        return kw
    kw.update(textures=None if descs is None else P.to_device(np.ascontiguousarray(descs, L.TEXTUREDESC), dev),
              texture_count=tex.get("texture_count", 0 if descs is None else len(descs)),
              texels=None if texels is None else P.to_device(np.ascontiguousarray(texels, np.uint32), dev),
              texel_words=tex.get("texel_words", 0 if texels is None else len(texels)))
    return kw


def _raster(ctx, args, w, h, offsets, tex, near_clip=0, limit=None, depth=None, vis=None, files=None):
    """one call of nv_rasterdepth_indexed_textured (files: of nv_rasterdepth_indexed_blocks) over cleared or loaded targets: the restatement's
    dict.  offsets None: both visibility pointers NULL"""
    import torch
    from niagara_amd import pipeline as P
    dev = ctx.device
    g, commands, count, draws, indices, vertices = args
    ctx.set_option(P.NV_OPT_RASTER_NEAR_CLIP, near_clip)
    if limit is not None:
        ctx.set_option(P.NV_OPT_RASTER_SMALL_LIMIT, limit)
    try:
        dcb = P.to_device(np.ascontiguousarray(commands, L.DRAWCMD), dev)
        dccb = P.to_device(np.array([count, 0, 0, 0], np.uint32), dev)
        db, ib, vb = P.to_device(draws, dev), P.to_device(np.ascontiguousarray(indices, np.uint32), dev), P.to_device(vertices, dev)
        ob = None if offsets is None else P.to_device(np.ascontiguousarray(offsets, np.uint64), dev)
        d = torch.zeros((h, w), dtype=torch.float32, device=dev) if depth is None else torch.from_numpy(np.ascontiguousarray(depth)).to(dev)
        v = None if offsets is None else (torch.zeros((h, w), dtype=torch.int64, device=dev) if vis is None
                                          else torch.from_numpy(np.ascontiguousarray(vis).view(np.int64)).to(dev))
        tot, alpha = torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
        entry = ctx.rasterdepth_indexed_textured if files is None else ctx.rasterdepth_indexed_blocks
        entry(g, dcb, dccb, db, len(draws), ib, len(indices), vb, len(vertices), d, w, h, ob, v, tot, alpha_totals2=alpha, **_set(ctx, tex, files))
        ctx.status()
        return dict(depth=d.cpu().numpy(), visibility=None if v is None else v.cpu().numpy().view(np.uint64), totals=tot.cpu().numpy().view(np.uint64),
                    alpha=alpha.cpu().numpy().view(np.uint64))
    finally:
        ctx.set_option(P.NV_OPT_RASTER_SMALL_LIMIT, 16)
        ctx.set_option(P.NV_OPT_RASTER_NEAR_CLIP, 0)


def _same_raster(name, got, ref):
    diff = {k: (-1 if ref[k] is None else int((got[k].view(np.uint64 if k == "visibility" else np.uint32) !=
                                                ref[k].view(np.uint64 if k == "visibility" else np.uint32)).sum())) for k in ("depth", "visibility")}
    print("%s: kept %d dropped %d unevaluated %d (restated %d %d %d); depth / visibility words that differ %d / %d" %
          (name, int(got["totals"][3]), int(got["alpha"][0]), int(got["alpha"][1]), int(ref["totals"][3]), int(ref["alpha"][0]), int(ref["alpha"][1]),
           diff["depth"], diff["visibility"]))
    assert got["totals"].tolist() == ref["totals"].tolist() and got["alpha"].tolist() == ref["alpha"].tolist()
    assert diff["depth"] == 0 and diff["visibility"] in (0, -1) and (got["visibility"] is None) == (ref["visibility"] is None)


def _run(name, ctx, riaref, s, with_vis=True, near_clip=0, limit=None, tex=None):
    w, h = s["viewport"]
    tex = RIA.tex(s) if tex is None else tex
    offsets = s["offsets"] if with_vis else None
    got = _raster(ctx, RIA.args(s), w, h, offsets, tex, near_clip, limit)
    with np.errstate(all="ignore"):
        ref = riaref.raster(*RIA.args(s), w, h, offsets, near_clip=near_clip, **tex)
    _same_raster(name, got, ref)
    return got, ref


# ---------------------------------------------------------------------------------------------------------------- the raster

@pytest.mark.gpu
@pytest.mark.parametrize("with_vis", [True, False])
@pytest.mark.parametrize("mips", [False, True])
@pytest.mark.parametrize("viewport", [(67, 37), (320, 192)])
def test_the_cutout_wall_equals_the_restatement(viewport, mips, with_vis, ctx, riaref, tref):
    """67 x 37: every triangle of the wall is small (a lane walks it alone, its corners in registers); 320 x 192: every triangle takes the wave
    path (its corners ride in LDS), and a 256-texel set keeps the texture minified there too"""
    s = RIA.occluder(tref, viewport, mips, size=256 if mips and viewport[0] == 320 else 64)
    got, ref = _run("occluder %dx%d mips %d visibility %d" % (viewport + (mips, with_vis)), ctx, riaref, s, with_vis)
    assert ref["alpha"][0] > 200 and ref["totals"][3] > 200 and ref["alpha"][1] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("mips", [False, True])
def test_commands_across_chunk_ends_on_both_raster_paths(mips, ctx, riaref, tref):
    """commands of 1, 63, 64, 65 and 200 triangles (a command's t crosses chunk ends, a wave starts in the middle of a command, its queue fills
    more than once) at 64 x 48, every triangle through the LDS queue (0), split between the paths (the default, 16) and through the lane path
    (INT_MAX): the restatement's bits each time, hence the same bits on both paths"""
    s = RIA.soup(tref, TC.SIZES, 31, mips, materials=(0, 2))
    outs = [_run("soup, limit %d, mips %d" % (limit, mips), ctx, riaref, s, limit=limit) for limit in (0, 16, INT_MAX)]
    ref = outs[0][1]
    assert ref["totals"][1] == sum(TC.SIZES) and ref["alpha"][0] > 300 and ref["totals"][3] > 300
    for got, _ in outs[1:]:
        for k in ("depth", "visibility", "totals", "alpha"):
            assert got[k].tobytes() == outs[0][0][k].tobytes(), k


@pytest.mark.gpu
def test_a_wave_takes_tested_opaque_and_tested_commands_in_turn(ctx, riaref, tref):
    """four commands per wave of the launch, in the repeating order alpha-tested (the cut-out albedo), opaque (no albedo texture), alpha-tested
    under another factor: whichever three or more consecutive commands a wave takes, its wave-uniform record must reload"""
    import torch
    waves = torch.cuda.get_device_properties(ctx.device).multi_processor_count * 6 * 4  # rasterindexed.h: RI_BLOCKS_PER_CU x RI_WAVES
    n = 4 * waves
    s = RIA.sequence(tref, True, n)
    assert s["materials"]["albedoTexture"].tolist()[:3] == [1, 0, 1] and s["draws"]["materialIndex"][:6].tolist() == [0, 1, 2, 0, 1, 2]
    ctx.reserve(n)
    got, ref = _run("command sequence, %d commands over %d waves" % (n, waves), ctx, riaref, s)
    assert ref["totals"][0] == n and ref["alpha"][0] > n and ref["totals"][3] > n


@pytest.mark.gpu
@pytest.mark.parametrize("mips", [False, True])
def test_the_clipped_floor_takes_uv_from_the_original_triangle(mips, ctx, riaref, tref):
    s = RIA.floor(tref, (320, 192), mips)
    got, ref = _run("floor 320x192 near clip, mips %d" % mips, ctx, riaref, s, near_clip=1)
    assert ref["alpha"][0] > 500 and ref["totals"][3] > 500
    unclipped = riaref.raster(*RIA.args(s), 320, 192, s["offsets"], **RIA.tex(s))
    assert unclipped["depth"].tobytes() != ref["depth"].tobytes()  # the clip is in play


@pytest.mark.gpu
@pytest.mark.parametrize("name", TCT.RULE_CASES)
def test_each_rule_case_through_the_abi(name, ctx, riaref, tref):
    s, _, kw, expect = TCT.rule_case(tref, name)
    got, ref = _run(name, ctx, riaref, s, tex=kw)
    assert (ref["alpha"][1] > 500) == (expect == "all-unevaluated") and (ref["alpha"][0] > 500) == (expect == "none")


@pytest.mark.gpu
@pytest.mark.parametrize("near_clip", [0, 1])
def test_without_post_pass_or_materials_it_is_the_untextured_entry_point(near_clip, ctx, tref):
    """nv_rasterdepth_indexed_visibility's bits on the same device; with both visibility pointers NULL nv_rasterdepth_indexed's"""
    s = RIA.floor(tref, (320, 192), True) if near_clip else RIA.occluder(tref, (67, 37), True)
    w, h = s["viewport"]
    for pp, tex in ((0, RIA.tex(s)), (0, dict()), (1, dict()), (1, dict(descs=s["descs"], texels=s["texels"]))):
        g = RR.globals_for(s["cull"], (w, h), pp)
        a = (g,) + RIA.args(s)[1:]
        plain = VG._raster(ctx, *a, w, h, s["offsets"], near_clip=near_clip)  # (it asserts nv_rasterdepth_indexed's depth and totals as well)
        got = _raster(ctx, a, w, h, s["offsets"], tex, near_clip=near_clip)
        assert plain[2][3] > 0
        assert got["depth"].tobytes() == plain[0].tobytes() and got["visibility"].tobytes() == plain[1].tobytes()
        assert got["totals"].tolist() == plain[2].tolist() and got["alpha"].tolist() == [0, 0]
        bare = _raster(ctx, a, w, h, None, tex, near_clip=near_clip)
        assert bare["depth"].tobytes() == plain[0].tobytes() and bare["totals"].tolist() == plain[2].tolist() and bare["alpha"].tolist() == [0, 0]


@pytest.mark.gpu
def test_refused_raster_calls_launch_nothing(ctx, tref):
    import torch
    from niagara_amd import pipeline as P
    from niagara_amd._lib import NvError
    s = RIA.occluder(tref, (67, 37), True)
    w, h = s["viewport"]
    dev = ctx.device
    g, commands, count, draws, indices, vertices = RIA.args(s)
    base = dict(globals_=g, dcb=P.to_device(commands, dev), dccb=P.to_device(np.array([count, 0, 0, 0], np.uint32), dev), db=P.to_device(draws, dev),
                draw_count=len(draws), ib=P.to_device(indices, dev), index_capacity=len(indices), vertices=P.to_device(vertices, dev),
                vertex_capacity=len(vertices), width=w, height=h, triangle_offsets=P.to_device(s["offsets"], dev),
                materials=P.to_device(s["materials"], dev), material_count=len(s["materials"]), textures=P.to_device(s["descs"], dev),
                texture_count=len(s["descs"]), texels=P.to_device(s["texels"], dev), texel_words=len(s["texels"]))
    depth = torch.full((h * w * 4 + 16,), POISON, dtype=torch.uint8, device=dev)
    vis = torch.full((h * w * 8 + 16,), POISON, dtype=torch.uint8, device=dev)
    tot = torch.full((4 * 8 + 16,), POISON, dtype=torch.uint8, device=dev)
    alpha = torch.full((2 * 8 + 16,), POISON, dtype=torch.uint8, device=dev)
    base.update(depth=depth, visibility=vis, totals4=tot, alpha_totals2=alpha)
    wrong = g.copy()
    wrong["screenWidth"] = w + 1
    byte = lambda t, k=4: t.view(torch.uint8).reshape(-1)[k:]
    table = [dict(width=0), dict(height=16385), dict(width=w + 1), dict(globals_=wrong), dict(depth=None), dict(dcb=None), dict(dccb=None), dict(db=None),
             dict(ib=None), dict(vertices=None), dict(triangle_offsets=None), dict(visibility=None), dict(depth=byte(depth, 2)), dict(visibility=byte(vis)),
             dict(triangle_offsets=byte(base["triangle_offsets"])), dict(totals4=byte(tot)), dict(alpha_totals2=byte(alpha)), dict(db=byte(base["db"])),
             dict(vertices=byte(base["vertices"])), dict(materials=byte(base["materials"])), dict(textures=byte(base["textures"])),
             dict(texels=byte(base["texels"], 2)), dict(ib=byte(base["ib"], 2)), dict(dcb=byte(base["dcb"], 2)), dict(dccb=byte(base["dccb"], 2)),
             dict(texels=None), dict(textures=None), dict(textures=None, texels=None), dict(material_count=0)]
    for kw in table:
        with pytest.raises(NvError, match="NV_EINVAL"):
            ctx.rasterdepth_indexed_textured(**{**base, **kw})
    with pytest.raises(NvError, match="NV_ENOMEM"):  # more commands than nv_reserve made room for: nv_rasterdepth_indexed's refusal
        ctx.rasterdepth_indexed_textured(**{**base, **dict(draw_count=2 ** 31)})
    ctx.status()
    for t in (depth, vis, tot, alpha):
        assert (t == POISON).all()
    depth[:h * w * 4] = 0  # (the poison is a larger word than any depth's bits: a maximum would leave it)
    ctx.rasterdepth_indexed_textured(**{**base, **dict(textures=None, texels=None, texture_count=0, texel_words=0, triangle_offsets=None, visibility=None)})
    ctx.status()  # no set and no target at all: every texture is absent, depth only
    assert (depth[:h * w * 4] != 0).any() and (depth[h * w * 4:] == POISON).all() and (alpha[16:] == POISON).all() and (vis == POISON).all()


def _bc_files():
    """a five-texture set whose first texture, the albedo every material of with_textures names, is BC7 with a full chain (then BC3, BC1, BC2,
    BC1): random blocks, so the alpha varies texel by texel"""
    return TG._texture_files(np.random.default_rng(23))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["bc1 cut-out", "bc7"])
def test_the_block_entry_point_equals_the_decoded_one(which, ctx, tref):
    """the wall at both viewports (both raster paths) and the clipped floor; BC1 punch-through alpha and BC7 (a random alpha per texel)"""
    for name, s, clip in (("occluder 67x37", RIA.occluder(tref, (67, 37), True), 0), ("occluder 320x192", RIA.occluder(tref, (320, 192), True, size=256), 0),
                          ("floor", RIA.floor(tref, (320, 192), True), 1)):
        files = s["textures"] if which == "bc1 cut-out" else _bc_files()
        descs, texels = host.texture_decode_host(files)
        tex = dict(materials=s["materials"], descs=descs, texels=texels)
        w, h = s["viewport"]
        dec = _raster(ctx, RIA.args(s), w, h, s["offsets"], tex, near_clip=clip)
        blk = _raster(ctx, RIA.args(s), w, h, s["offsets"], tex, near_clip=clip, files=files)
        print("%s, %s: kept %d dropped %d" % (name, which, int(dec["totals"][3]), int(dec["alpha"][0])))
        assert dec["alpha"][0] >= 1 and dec["totals"][3] >= 1  # both outcomes occur (the BC7 alpha is random: minified, few samples fall below 0.5)
        for k in ("totals", "alpha", "depth", "visibility"):
            assert dec[k].tobytes() == blk[k].tobytes(), k


# ---------------------------------------------------------------------------------------------------------------- the attribute pass

def _attr_scene(ctx):
    """occluder_scene_indexed with attributes under TG's five-texture set (BC7 64^2, BC3 20 x 12 x 5, BC1 1 x 1, BC2 8 x 8, BC1 64^2): materials
    that name textures of every format, one of them an id past the table"""
    files, descs, table, texels, htexels = TG._texture_set(ctx)
    s = TC.occluder_with_attributes()
    m = s["materials"].copy()
    names = [(1, 5, 4, 2), (len(descs), 2, 0xFFFFFFFF, 5), (2, 1, 0, 0), (5, 0, 1, 3), (0, 0, 0, 0)]
    for i in range(len(m)):
        m[i]["albedoTexture"], m[i]["normalTexture"], m[i]["specularTexture"], m[i]["emissiveTexture"] = names[i % len(names)]
    s["materials"] = m
    return s, dict(files=files, descs=descs, table=table, texels=texels, htexels=htexels)


def _attributes(ctx, g, records, w, h, s, ts, blocks=False, counts=None, draws=None):
    """one launch of nv_visibility_attributes_indexed_textured (blocks: of ..._blocks) into poisoned outputs: TG._host's dict"""
    from niagara_amd import pipeline as P
    dev = ctx.device
    draws = s["draws"] if draws is None else draws
    cnt = dict(draws=len(draws), indices=len(s["indices"]), vertices=len(s["vertices"]), materials=len(s["materials"]))
    cnt.update(counts or {})
    out = TG._poisoned(ctx, w * h)
    a = (g, P.to_device(np.ascontiguousarray(records, L.VISINDEXEDRECORD), dev), w, h, P.to_device(draws, dev), cnt["draws"], P.to_device(s["indices"], dev),
         cnt["indices"], P.to_device(s["vertices"], dev), cnt["vertices"], P.to_device(s["materials"], dev), cnt["materials"], out["attributes"],
         out["gbuffer0"], out["gbuffer1"], out["totals"])
    if blocks:
        bdescs, hblocks = host.texture_blocks_host(ts["files"])
        ctx.visibility_attributes_indexed_blocks(*a, P.to_device(bdescs, dev), len(bdescs), P.to_device(hblocks, dev), len(hblocks) // 16)
    else:
        ctx.visibility_attributes_indexed_textured(*a, ts["table"], len(ts["descs"]), ts["texels"], len(ts["htexels"]))
    ctx.status()
    return TG._host(out)


def _check_attributes(name, ctx, tref, iaref, g, rec, w, h, s, ts, counts=None, draws=None):
    """the decoded entry point against the restatement under TG._same, the block one against the decoded one bit for bit"""
    want = RIA.attributes(tref, iaref, g, rec, w, h, s["draws"] if draws is None else draws, s["indices"], s["vertices"], s["materials"], ts["descs"],
                          ts["htexels"], counts=counts)
    assert tref.bad_indices() == 0
    got = _attributes(ctx, g, rec, w, h, s, ts, counts=counts, draws=draws)
    TG._same(name, got, want, ts["descs"], s["materials"])
    blk = _attributes(ctx, g, rec, w, h, s, ts, blocks=True, counts=counts, draws=draws)
    for k in ("totals", "attributes", "gbuffer1", "gbuffer0"):
        assert got[k].tobytes() == blk[k].tobytes(), "%s of the block entry point differs from the decoded one's" % k
    return got, want


@pytest.mark.gpu
def test_attributes_of_the_resolved_occluder_scene_equal_the_restatement(ctx, tref, iaref, viref):
    """the records the restated classic chain resolves at 320 x 192, every draw; and without a table nv_visibility_attributes_indexed's bytes"""
    s, ts = _attr_scene(ctx)
    w, h = s["viewport"]
    _, res, _, _, _ = TC.classic_records(s, viref)
    cd = s["cull"].copy()
    cd["cullingEnabled"] = 0
    g = RR.globals_for(cd, (w, h), 0)
    got, want = _check_attributes("occluder", ctx, tref, iaref, g, res["records"], w, h, s, ts)
    assert want["totals"][0] > w * h // 4 and 0 < want["totals"][3] < want["totals"][0]
    bare = _attributes(ctx, g, res["records"], w, h, s, dict(ts, table=None, descs=[], texels=None, htexels=[]))
    plain = VG._attributes(ctx, g, res["records"], w, h, s["draws"], s["indices"], s["vertices"], s["materials"])
    assert all(bare[k].tobytes() == plain[k].tobytes() for k in ("attributes", "gbuffer0", "gbuffer1")) and bare["totals"][:3].tolist() == plain["totals"][:3].tolist()
    assert (bare["gbuffer0"] != got["gbuffer0"]).any()  # and the textures do change the picture


@pytest.mark.gpu
def test_attributes_second_trip_of_the_persistent_grid(ctx, tref, iaref):
    import torch
    cus = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    w, h, items = PC.second_trip_sizes(cus)["pixel"]
    first = PC.check_second_trip(items, w, h, cus)
    s, ts = _attr_scene(ctx)
    g = RR.globals_for(host.build_cull_data(viewport=(w, h)), (w, h), 0)
    rec = VG._attr_records(s, w * h, 7, run=29)
    got, want = _check_attributes("second trip", ctx, tref, iaref, g, rec, w, h, s, ts)
    assert want["totals"][0] > 0 and want["totals"][1] > 0 and want["totals"][3] > 0
    assert (got["attributes"].view(np.uint32).reshape(w * h, 16)[first:] != 0x5A5A5A5A).any(), "nothing of the second trip was written"


@pytest.mark.gpu
def test_attributes_run_edges_across_materials_and_invalid_records(ctx, tref, iaref):
    """a run start on lanes 0, 1, 15-17, 31-33, 47-49, 62, 63 by each word of the key alone — by the draw alone it is one triangle under two
    materials whose textures differ — and by the depth alone (no start); a first lane that is invalid or empty with valid lanes behind it; a
    ragged last wave; every invalid class; a material index past the table; an index capacity that cuts a run's triangle"""
    s, ts = _attr_scene(ctx)
    draws, meshes = s["draws"].copy(), s["meshes"]
    two = [i for i in range(len(draws)) if draws["meshIndex"][i] == draws["meshIndex"][len(draws) - 1]][:2]  # two draws of one mesh
    assert len(two) == 2
    draws["materialIndex"][two[0]], draws["materialIndex"][two[1]] = 0, 1
    assert s["materials"][0]["albedoTexture"] != s["materials"][1]["albedoTexture"]
    lod = meshes["lods"][int(draws["meshIndex"][two[0]]), 0]
    vo = int(meshes["vertexOffset"][int(draws["meshIndex"][two[0]])])
    base = np.array((two[0], int(lod["indexOffset"]) + 6, vo, 77), dtype=L.VISINDEXEDRECORD)
    rows = []
    for start in (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 62, 63):
        for field, value in (("drawId", two[1]), ("indexPosition", int(lod["indexOffset"]) + 9), ("vertexOffset", vo + 1), ("depthBits", 78)):
            row = np.repeat(base.reshape(1), 64)
            row[field][start:] = value
            rows.append(row)
    for first in ((len(draws) + 1, 0, 0, 5), (0xFFFFFFFF, 0, 0, 0), (two[0], len(s["indices"]) - 2, vo, 5), (two[0], 0xFFFFFFFF, vo, 5),
                  (two[0], int(lod["indexOffset"]), len(s["vertices"]), 5), (0xFFFFFFFF,) * 4):
        row = np.repeat(base.reshape(1), 64)
        row[0] = np.array(first, dtype=L.VISINDEXEDRECORD)
        rows.append(row)
    rec = np.concatenate(rows + [np.repeat(base.reshape(1), 37)])
    w, h = len(rec), 1
    g = RR.globals_for(host.build_cull_data(viewport=(w, h)), (w, h), 0)
    got, want = _check_attributes("run edges", ctx, tref, iaref, g, rec, w, h, s, ts, draws=draws)
    assert want["totals"][1] == 4
    at = np.flatnonzero((rec["drawId"][1:] == two[1]) & (rec["drawId"][:-1] == two[0])) + 1  # the crossings by the draw alone
    assert len(at) >= 12 and (want["gbuffer0"][at] != want["gbuffer0"][at - 1]).any()
    bad = draws.copy()
    bad["materialIndex"][two[0]] = len(s["materials"])
    _check_attributes("material past the table", ctx, tref, iaref, g, rec, w, h, s, ts, draws=bad)
    cut = dict(indices=int(lod["indexOffset"]) + 9)  # the run's triangle at + 9 loses its last index
    _, short = _check_attributes("indices cut short", ctx, tref, iaref, g, rec, w, h, s, ts, counts=cut, draws=draws)
    assert short["totals"][1] > 4


@pytest.mark.gpu
def test_refused_attribute_calls_launch_nothing(ctx):
    import torch
    from niagara_amd import pipeline as P
    from niagara_amd._lib import NvError
    s, ts = _attr_scene(ctx)
    dev = ctx.device
    w, h = 16, 4
    g = RR.globals_for(host.build_cull_data(viewport=(w, h)), (w, h), 0)
    rec = torch.zeros(w * h * 16 + 16, dtype=torch.uint8, device=dev)
    db, ib, vb, mb = (P.to_device(s[k], dev) for k in ("draws", "indices", "vertices", "materials"))
    out = TG._poisoned(ctx, w * h + 4)
    nd, ni, nv, nm = len(s["draws"]), len(s["indices"]), len(s["vertices"]), len(s["materials"])

    def call(r=rec, width=w, d=db, i=ib, v=vb, m=mb, a=out["attributes"], t=out["totals"], glob=g, table=ts["table"], texels=ts["texels"]):
        ctx.visibility_attributes_indexed_textured(glob, r, width, h, d, nd, i, ni, v, nv, m, nm, a, out["gbuffer0"], out["gbuffer1"], t, table,
                                                   len(ts["descs"]), texels, len(ts["htexels"]))
    other = g.copy()
    other["screenWidth"] = w + 1
    u8 = lambda t, k: t.view(torch.uint8).reshape(-1)[k:]
    for kw in (dict(r=None), dict(d=None), dict(i=None), dict(v=None), dict(width=0), dict(glob=other), dict(m=None), dict(r=rec[8:]),
               dict(a=out["attributes"][8:]), dict(d=u8(db, 8)), dict(v=u8(vb, 8)), dict(m=u8(mb, 8)), dict(t=u8(out["totals"], 4)), dict(i=u8(ib, 2)),
               dict(table=None), dict(texels=None), dict(table=u8(ts["table"], 8)), dict(texels=u8(ts["texels"], 2))):
        with pytest.raises(NvError, match="NV_EINVAL"):
            call(**kw)
    ctx.status()
    assert (out["attributes"] == TG.POISON).all() and (out["gbuffer0"] == TG.POISON32).all() and (out["gbuffer1"] == TG.POISON32).all()
    assert (out["totals"] == 0).all()
    call()
    ctx.status()


# ---------------------------------------------------------------------------------------------------------------- the chain

def _frames(pipe, s, task, **kw):
    """two frames, resolve and textured attributes on `pipe`; then the post raster once more over the finished targets for its totals (kept and
    dropped do not depend on what the targets hold)"""
    import torch
    from niagara_amd import pipeline as P
    vis = pipe.new_visibility()
    for _ in range(2):
        pipe.frame(s["cull"], post_pass=True, visibility=vis, task=task, **kw)
    res = pipe.resolve(s["cull"], vis, classic=not task)
    att = pipe.attributes(s["cull"], res["records"], s["materials"], textures=True, classic=not task)
    depth = pipe.depth.cpu().numpy().copy()
    tot, alpha = torch.zeros(4, dtype=torch.int64, device=pipe.ctx.device), torch.zeros(2, dtype=torch.int64, device=pipe.ctx.device)
    if kw.get("textures"):
        raster = pipe.render_depth if task else pipe.render_draws
        raster(s["cull"], late=True, post_pass=1, visibility=vis, totals4=tot, textures=True, materials=s["materials"], alpha_totals2=alpha)
    pipe.ctx.status()
    out = TG._host(att)
    out.update(depth=depth, records=P.from_device(res["records"], L.VISRECORD if task else L.VISINDEXEDRECORD).copy(), kept=int(tot[3].item()),
               alpha=alpha.cpu().numpy().tolist(), att=att, vis=vis)
    return out


@pytest.mark.gpu
def test_the_classic_frame_with_textures_shows_what_the_cluster_frame_shows(tref, iaref, tmp_path_factory):
    """with_textures(occluder_scene_indexed(), cutout=True) at 320 x 192, the wall in the post pass: frame(task=False, textures=True) ->
    resolve(classic=True) -> attributes(classic=True, textures=True) -> shade()"""
    import shade_ref as SR
    import test_shade_gpu as TS
    import test_shadow_alpha_cpu as SC
    import test_shadowtrace_gpu as STG
    import torch
    from niagara_amd import pipeline as P
    from niagara_amd import synth
    from niagara_amd._lib import NvError
    sref = SR.load(tmp_path_factory.mktemp("shade_ref_vit"))
    s, t = SC.cutout_occluder()
    s["draws"]["position"][s["wall"]] += np.array(RA.WALL_SHIFT, np.float32)
    w, h = s["viewport"]
    assert (w, h) == (320, 192)
    TC.order_condition(s)
    cluster = STG._pipeline(s, 0)
    try:
        cluster.set_textures(s["textures"])
        want = _frames(cluster, s, True, textures=True, materials=s["materials"])
    finally:
        cluster.ctx.close()
    pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], **VG._pipe_kw(s))
    try:
        vis = pipe.new_visibility()
        for kw in (dict(), dict(materials=s["materials"])):  # no set, with and without the table: nothing is launched
            with pytest.raises(NvError, match="set_textures"):
                pipe.frame(s["cull"], post_pass=True, task=False, visibility=vis, textures=True, **kw)
        pipe.cull(s["cull"], late=False, task=False)
        with pytest.raises(NvError, match="set_textures"):
            pipe.render_draws(s["cull"], late=False, textures=True, materials=s["materials"])
        pipe.set_textures(s["textures"])
        with pytest.raises(NvError, match="materials="):
            pipe.frame(s["cull"], post_pass=True, task=False, visibility=vis, textures=True)
        with pytest.raises(NvError, match="materials="):
            pipe.render_draws(s["cull"], late=False, textures=True)
        solid = _frames(pipe, s, False)
        got = _frames(pipe, s, False, textures=True, materials=s["materials"])
        behind, behind_solid = (int(np.isin(o["records"]["drawId"], s["hidden"]).sum()) for o in (got, solid))
        print("pixels that resolve to a box behind the wall: %d with textures, %d without; kept %d dropped %d unevaluated %d (cluster path %d %s)" %
              (behind, behind_solid, got["kept"], got["alpha"][0], got["alpha"][1], want["kept"], want["alpha"]))
        assert behind > 0 and behind_solid == 0
        assert got["alpha"] == want["alpha"] and got["kept"] == want["kept"] and got["alpha"][0] > 1000
        assert got["depth"].tobytes() == want["depth"].tobytes()
        for k in ("attributes", "gbuffer0", "gbuffer1"):
            assert got[k].tobytes() == want[k].tobytes(), k
        assert got["totals"].tolist() == want["totals"].tolist() and got["totals"][3] == 0

        # shade() behind it, against tests/shade_ref.c on the RESTATED G-buffers of the records the frame resolved
        g = synth.make_globals(s["cull"], (w, h))
        restated = RIA.attributes(tref, iaref, g, got["records"], w, h, s["draws"], s["indices"], s["vertices"], s["materials"], t["descs"], t["texels"])
        TG._same("classic frame", got, restated, t["descs"], s["materials"])
        camera, sun = (0.0, 0.0, 0.0), np.array([0.35, 0.6, 0.72]) / np.linalg.norm([0.35, 0.6, 0.72])
        color = pipe.shade(s["cull"], got["att"]["gbuffer0"], got["att"]["gbuffer1"], camera, sun, shadow=None)
        pipe.ctx.status()
        sd = host.build_shade_data(g, camera, sun, 0, w, h)
        shaded = sref.shade(sd, restated["gbuffer0"].reshape(h, w), restated["gbuffer1"].reshape(h, w), got["depth"], znear=float(s["cull"]["znear"][0]),
                            shadow=None)
        TS._close("shade behind the textured classic frame", SR.channels(color.cpu().numpy().view(np.uint32)), SR.channels(shaded), alpha=True)
        # the traced, alpha-tested shadow needs nothing new behind a classic frame
        pipe.build_rt_scene(s["meshes"], s["indices"], s["vertices"], s["draws"], texcoords=True)
        traced = pipe.shade(s["cull"], got["att"]["gbuffer0"], got["att"]["gbuffer1"], camera, STG.SUN, shadow="trace", blur=False, textures=True,
                            materials=s["materials"])
        pipe.ctx.status()
        mask = pipe.shadow_image.cpu().numpy()
        assert (mask == 0).any() and (mask == 255).any() and (traced.cpu().numpy() != 0).any()

        # the post raster and the attribute pass replayed from a captured graph give the same bytes
        mat = P.to_device(np.ascontiguousarray(s["materials"], L.MATERIAL), pipe.ctx.device)
        depth0 = torch.zeros_like(pipe.depth)
        tot, alpha = torch.zeros(4, dtype=torch.int64, device=pipe.ctx.device), torch.zeros(2, dtype=torch.int64, device=pipe.ctx.device)
        rec = pipe.resolve(s["cull"], got["vis"], classic=True)["records"]
        n = w * h
        out = dict(attributes=torch.zeros(n * 64, dtype=torch.uint8, device=pipe.ctx.device), gbuffer0=torch.zeros(n, dtype=torch.int32, device=pipe.ctx.device),
                   gbuffer1=torch.zeros(n, dtype=torch.int32, device=pipe.ctx.device), totals=torch.zeros(4, dtype=torch.int64, device=pipe.ctx.device))
        form, tset = pipe._texture_set()

        def step(v):
            pipe.render_draws(s["cull"], late=True, post_pass=1, visibility=v, totals4=tot, textures=True, materials=mat, alpha_totals2=alpha)
            pipe.ctx.visibility_attributes_indexed_textured(g, rec, w, h, pipe.db, pipe.draw_count, pipe.ib, pipe.index_count, pipe.vb, pipe.vertex_count, mat,
                                                            len(s["materials"]), out["attributes"], out["gbuffer0"], out["gbuffer1"], out["totals"], *tset)
        tensors = lambda v: (pipe.depth, v, tot, alpha, out["attributes"], out["gbuffer0"], out["gbuffer1"], out["totals"])
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            eager_v = pipe.new_visibility()
            pipe.depth.copy_(depth0)
            step(eager_v)
            torch.cuda.synchronize()
            eager = [x.cpu().numpy().copy() for x in tensors(eager_v)]
            assert eager[3][0] > 1000 and eager[2][3] > 1000 and eager[5].tobytes() == got["gbuffer0"].tobytes()
            graph_v = pipe.new_visibility()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=st):
                step(graph_v)
            torch.cuda.synchronize()
            for _ in range(2):
                pipe.depth.copy_(depth0)
                for x in tensors(graph_v)[1:]:
                    x.zero_()
                graph.replay()
                torch.cuda.synchronize()
                for x, e in zip(tensors(graph_v), eager):
                    assert x.cpu().numpy().tobytes() == e.tobytes()
        pipe.ctx.status()
    finally:
        pipe.ctx.close()
    # the other prerequisites: no index buffer, no stable ids with a visibility target
    kw = dict(VG._pipe_kw(s))
    del kw["indices"]
    bare = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], **kw)
    try:
        bare.set_textures(s["textures"])
        with pytest.raises(NvError, match="indices="):
            bare.frame(s["cull"], task=False, textures=True, materials=s["materials"])
        with pytest.raises(NvError):
            bare.attributes(s["cull"], bare.new_visibility(), s["materials"], textures=True, classic=True)
    finally:
        bare.ctx.close()
    loose = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], **dict(VG._pipe_kw(s), stable_ids=False))
    try:
        loose.set_textures(s["textures"])
        with pytest.raises(NvError, match="stable"):
            loose.frame(s["cull"], task=False, textures=True, materials=s["materials"], visibility=loose.new_visibility())
    finally:
        loose.ctx.close()
