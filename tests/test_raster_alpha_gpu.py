"""nv_rasterdepth_textured on the MI355X against the restatement tests/raster_alpha_ref.c.

Comparison rule.  Where the texture has one level, or the level of detail clamps to 0, depth target, visibility target and all six totals equal
the restatement byte for byte.  Where a mip chain is in play the device's log2 may differ from glibc's in the last bit of the level of detail: a
sample whose restated |alpha - 0.5| <= B (B = §4.18's counted bound (3 (W + H) + 32) 2^-24 of the texture plus 2^-24 for the product with the
factor) is UNDECIDED.  A pixel no undecided sample covers must be bit-identical; one that an undecided sample covers must hold a value between
the restatement's result with every undecided sample dropped and with every one kept (both targets are maxima); `dropped` may differ by at most
the number of undecided samples.  Undecided samples are at most 0.1 % of the alpha-tested ones in every case — a condition on the inputs,
asserted on the restatement here and in tests/test_raster_alpha_cpu.py, not a measurement of the device."""
import numpy as np
import pytest

import raster_alpha_ref as RA
import raster_ref as RR
import test_raster_alpha_cpu as AC
import test_raster_gpu as TG
import texture_ref as TR
from niagara_amd import layouts as L

POISON = 0x5A


@pytest.fixture(scope="session")
def aref(tmp_path_factory):
    return RA.load(tmp_path_factory.mktemp("raster_alpha_ref_gpu"))


@pytest.fixture(scope="session")
def tref(tmp_path_factory):
    return TR.load(tmp_path_factory.mktemp("texture_ref_alpha_gpu"))


@pytest.fixture(scope="module")
def ctx():
    from niagara_amd import pipeline as P
    c = P.Context()
    yield c
    c.close()


def _gpu(ctx, args, w, h, tex, near_clip=0, stable=0, limit=None, alpha_totals=True):
    """nv_rasterdepth_textured through Context.rasterdepth_textured: dict of depth, visibility, totals, alpha.  tex: materials / descs / texels
    (host arrays, each optional) and the count overrides of raster_alpha_ref.AlphaRef.raster"""
    import torch
    from niagara_amd import pipeline as P
    dev = ctx.device
    ctx.set_option(P.NV_OPT_RASTER_NEAR_CLIP, near_clip)
    ctx.set_option(P.NV_OPT_RASTER_VISIBILITY_ID, stable)
    if limit is not None:
        ctx.set_option(P.NV_OPT_RASTER_SMALL_LIMIT, limit)
    try:
        t = [P.to_device(a, dev) for a in args[1:]]
        mats, descs, texels = tex.get("materials"), tex.get("descs"), tex.get("texels")
        dm = None if mats is None else P.to_device(np.ascontiguousarray(mats, L.MATERIAL), dev)
        dd = None if descs is None else P.to_device(np.ascontiguousarray(descs, L.TEXTUREDESC), dev)
        dt = None if texels is None else P.to_device(np.ascontiguousarray(texels, np.uint32), dev)
        d = torch.zeros((h, w), dtype=torch.float32, device=dev)
        v = torch.zeros((h, w), dtype=torch.int64, device=dev)
        tot = torch.zeros(4, dtype=torch.int64, device=dev)
        alpha = torch.zeros(2, dtype=torch.int64, device=dev) if alpha_totals else None
        kw = dict(materials=dm, material_count=tex.get("material_count", 0 if mats is None else len(mats)), textures=dd,
                  texture_count=tex.get("texture_count", 0 if descs is None else len(descs)), texels=dt,
                  texel_words=tex.get("texel_words", 0 if texels is None else len(texels)), alpha_totals2=alpha)
        ctx.rasterdepth_textured(args[0], *t, d, w, h, v, tot, **kw)
        ctx.status()
        return dict(depth=d.cpu().numpy(), visibility=v.cpu().numpy().view(np.uint64), totals=tot.cpu().numpy().view(np.uint64),
                    alpha=None if alpha is None else alpha.cpu().numpy().view(np.uint64))
    finally:
        ctx.set_option(P.NV_OPT_RASTER_SMALL_LIMIT, 16)
        ctx.set_option(P.NV_OPT_RASTER_NEAR_CLIP, 0)
        ctx.set_option(P.NV_OPT_RASTER_VISIBILITY_ID, 0)


def _compare(name, got, ref, band):
    """ref(policy) -> the restatement's output.  band = False: byte for byte; True: the rule of the module's docstring"""
    rule = ref(0)
    c = rule["counters"]
    und = rule["undecided"]
    diff = {k: int((got[k].view(np.uint64 if k == "visibility" else np.uint32) != rule[k].view(np.uint64 if k == "visibility" else np.uint32)).sum())
            for k in ("depth", "visibility")}
    print("%s: kept %d dropped %d unevaluated %d (restated %d %d %d); %d alpha-tested samples, %d undecided on %d pixels; depth / visibility words that differ %d / %d" %
          (name, int(got["totals"][3]), int(got["alpha"][0]), int(got["alpha"][1]), int(rule["totals"][3]), int(rule["alpha"][0]), int(rule["alpha"][1]),
           c["tested_samples"], c["undecided"], int(und.sum()), diff["depth"], diff["visibility"]))
    if not band:
        assert c["undecided"] == 0
        assert got["totals"].tolist() == rule["totals"].tolist() and got["alpha"].tolist() == rule["alpha"].tolist()
        assert diff == dict(depth=0, visibility=0)
        return rule
    assert c["undecided"] <= AC.UNDECIDED_CAP * c["tested_samples"]
    lo, hi = (ref(1), ref(2)) if c["undecided"] else (rule, rule)
    for k, t in (("depth", np.uint32), ("visibility", np.uint64)):
        g, r, a, b = (x[k].view(t) for x in (got, rule, lo, hi))
        assert (g[~und] == r[~und]).all()
        assert ((a[und] <= g[und]) & (g[und] <= b[und])).all()
    assert got["totals"][:3].tolist() == rule["totals"][:3].tolist() and int(got["alpha"][1]) == int(rule["alpha"][1])
    assert int(got["totals"][3]) + int(got["alpha"][0]) == int(rule["totals"][3]) + int(rule["alpha"][0])
    assert abs(int(got["alpha"][0]) - int(rule["alpha"][0])) <= c["undecided"]
    return rule


def _run(name, ctx, aref, s, band, near_clip=0, stable=0, limit=None, tex=None):
    w, h = s["viewport"]
    tex = AC._tex(s) if tex is None else tex
    got = _gpu(ctx, RA.args(s), w, h, tex, near_clip, stable, limit)
    ref = lambda policy: aref.raster(*RA.args(s), w, h, near_clip=near_clip, stable=stable, band=band, policy=policy,
                                     small_limit=16 if limit is None else limit, **tex)
    return got, _compare(name, got, ref, band)


# ---------------------------------------------------------------------------------------------------------------- 1, 2: the cut-out occluder scene

@pytest.mark.gpu
@pytest.mark.parametrize("stable", [0, 1])
@pytest.mark.parametrize("mips", [False, True])
@pytest.mark.parametrize("viewport", [(67, 37), (320, 192)])
def test_the_cutout_wall_equals_the_restatement(viewport, mips, stable, ctx, aref, tref):
    """67 x 37: every triangle of the wall is small (a lane walks it alone, its taps diverge), the texture is minified; 320 x 192: every triangle
    takes the wave path, and a 256-texel set keeps it minified there too"""
    s = RA.occluder(tref, viewport, mips, size=256 if mips and viewport[0] == 320 else 64)
    aref.hits()
    got, rule = _run("occluder %dx%d mips %d stable %d" % (viewport + (mips, stable)), ctx, aref, s, mips, stable=stable)
    c, hits = rule["counters"], aref.hits()
    assert c["slots_tested"] == 16 and rule["alpha"][0] > 200 and rule["totals"][3] > 200
    assert (c["tested_small"] > 0 and c["tested_large"] == 0) if viewport[0] == 67 else (c["tested_large"] > 0 and c["tested_small"] == 0)
    assert not mips or hits[15] > 0.9 * c["tested_samples"]  # the level of detail is fractional: two levels are blended


@pytest.mark.gpu
def test_both_raster_paths_write_the_same_bits(ctx, aref, tref):
    """NV_OPT_RASTER_SMALL_LIMIT 0 (every triangle through the wave path) and a limit between the wall's box sizes (some down each path)"""
    s = RA.occluder(tref, (320, 192), True, size=256)
    split = None
    for limit in (42, 48, 49, 56, 63):
        c = aref.raster(*RA.args(s), 320, 192, small_limit=limit, **AC._tex(s))["counters"]
        if c["tested_small"] > 100 and c["tested_large"] > 100:
            split = limit
            break
    assert split is not None
    a, rule = _run("occluder 320x192, limit 0", ctx, aref, s, True, limit=0)
    b, _ = _run("occluder 320x192, limit %d" % split, ctx, aref, s, True, limit=split)
    assert rule["counters"]["tested_small"] == 0
    for k in ("depth", "visibility", "totals", "alpha"):
        assert a[k].tobytes() == b[k].tobytes()


# ---------------------------------------------------------------------------------------------------------------- 3: slot after slot in one wave

@pytest.mark.gpu
@pytest.mark.parametrize("mips", [False, True])
def test_a_wave_takes_tested_opaque_and_tested_slots_in_turn(mips, ctx, aref, tref):
    import torch
    waves = torch.cuda.get_device_properties(ctx.device).multi_processor_count * 6 * 4  # niagara_amd/csrc/rasterdepth.h: RD_BLOCKS_PER_CU x RD_WAVES
    slots = 4 * waves
    s = RA.sequence(tref, mips, slots)
    got, rule = _run("slot sequence, %d slots over %d waves, mips %d" % (slots, waves, mips), ctx, aref, s, mips)
    c = rule["counters"]
    assert -(-slots // waves) >= 3  # every wave takes three or more consecutive slots
    assert c["slots_tested"] > slots // 2 and c["slots_constant"] >= slots // 3 and c["tested_cut_stamps"] >= slots // 3 and c["tested_large"] > 0 and c["tested_small"] == 0
    assert rule["alpha"][0] > slots and rule["totals"][3] > slots


# ---------------------------------------------------------------------------------------------------------------- 4: near clip

@pytest.mark.gpu
@pytest.mark.parametrize("stable", [0, 1])
@pytest.mark.parametrize("mips", [False, True])
def test_the_clipped_floor_takes_uv_from_the_original_triangle(mips, stable, ctx, aref, tref):
    s = RA.floor(tref, (320, 192), mips)
    got, rule = _run("floor 320x192 near clip, mips %d stable %d" % (mips, stable), ctx, aref, s, mips, near_clip=1, stable=stable)
    assert rule["counters"]["tested_clipped"] >= 4 and rule["alpha"][0] > 500 and rule["totals"][3] > 500


# ---------------------------------------------------------------------------------------------------------------- 5: the rule, case by case

@pytest.mark.gpu
@pytest.mark.parametrize("name", AC.RULE_CASES)
def test_each_rule_case_through_the_abi(name, ctx, aref, tref):
    s, _, kw, _ = AC.rule_case(tref, name)
    got, rule = _run(name, ctx, aref, s, True, tex=kw)
    assert (rule["counters"]["nan_alpha"] > 500) == (name == "NaN uv")


# ---------------------------------------------------------------------------------------------------------------- 6: the launches that do not test

@pytest.mark.gpu
@pytest.mark.parametrize("near_clip", [0, 1])
def test_without_post_pass_or_materials_it_is_nv_rasterdepth(near_clip, ctx, tref):
    from niagara_amd import pipeline as P
    s = RA.floor(tref, (320, 192), True) if near_clip else RA.occluder(tref, (67, 37), True)
    w, h = s["viewport"]
    for pp, tex in ((0, AC._tex(s)), (0, dict()), (1, dict()), (1, dict(descs=s["descs"], texels=s["texels"]))):
        g = RR.globals_for(s["cull"], (w, h), pp)
        a = (g,) + RA.args(s)[1:]
        ctx.set_option(P.NV_OPT_RASTER_NEAR_CLIP, near_clip)
        try:
            plain = TG._gpu(ctx, a, w, h)
        finally:
            ctx.set_option(P.NV_OPT_RASTER_NEAR_CLIP, 0)
        got = _gpu(ctx, a, w, h, tex, near_clip=near_clip)
        assert plain[2][3] > 0
        assert got["depth"].tobytes() == plain[0].tobytes() and got["visibility"].tobytes() == plain[1].tobytes()
        assert got["totals"].tolist() == plain[2].tolist() and got["alpha"].tolist() == [0, 0]


# ---------------------------------------------------------------------------------------------------------------- 7: refusals

@pytest.mark.gpu
def test_refused_calls_launch_nothing(ctx, tref):
    import torch
    from niagara_amd import pipeline as P
    from niagara_amd._lib import NvError
    s = RA.occluder(tref, (67, 37), True)
    w, h = s["viewport"]
    dev = ctx.device
    names = ("dcb", "db", "mlb", "meshlet_data", "vertices", "cib", "ccb")
    base = dict(zip(names, (P.to_device(a, dev) for a in RA.args(s)[1:])))
    base.update(globals_=s["g"], width=w, height=h, materials=P.to_device(s["materials"], dev), material_count=len(s["materials"]),
                textures=P.to_device(s["descs"], dev), texture_count=len(s["descs"]), texels=P.to_device(s["texels"], dev), texel_words=len(s["texels"]))
    depth = torch.full((h * w * 4 + 16,), POISON, dtype=torch.uint8, device=dev)
    vis = torch.full((h * w * 8 + 16,), POISON, dtype=torch.uint8, device=dev)
    tot = torch.full((4 * 8 + 16,), POISON, dtype=torch.uint8, device=dev)
    alpha = torch.full((2 * 8 + 16,), POISON, dtype=torch.uint8, device=dev)
    base.update(depth=depth, visibility=vis, totals4=tot, alpha_totals2=alpha)
    wrong = s["g"].copy()
    wrong["screenWidth"] = w + 1
    byte = lambda t, k=4: t[k:]  # a flat uint8 tensor k bytes on
    table = [dict(width=0), dict(height=16385), dict(width=w + 1), dict(globals_=wrong), dict(depth=None), dict(dcb=None), dict(vertices=None),
             dict(depth=byte(depth, 2)), dict(visibility=byte(vis)), dict(totals4=byte(tot)), dict(alpha_totals2=byte(alpha)), dict(db=byte(base["db"])),
             dict(vertices=byte(base["vertices"])), dict(materials=byte(base["materials"])), dict(textures=byte(base["textures"])),
             dict(texels=byte(base["texels"], 2)), dict(mlb=byte(base["mlb"], 2)), dict(meshlet_data=byte(base["meshlet_data"], 2)),
             dict(cib=byte(base["cib"], 2)), dict(ccb=byte(base["ccb"], 2)), dict(dcb=byte(base["dcb"], 2)),
             dict(texels=None), dict(textures=None), dict(textures=None, texels=None), dict(material_count=0)]
    for kw in table:
        with pytest.raises(NvError):
            ctx.rasterdepth_textured(**{**base, **kw})
    ctx.status()
    for t in (depth, vis, tot, alpha):
        assert (t == POISON).all()
    depth[:h * w * 4] = 0  # (the poison is a larger word than any depth's bits: a maximum would leave it)
    ctx.rasterdepth_textured(**{**base, **dict(textures=None, texels=None, texture_count=0, texel_words=0)})  # no set at all: every texture is absent
    ctx.status()
    assert (depth[:h * w * 4] != 0).any() and (depth[h * w * 4:] == POISON).all() and (alpha[16:] == POISON).all()


# ---------------------------------------------------------------------------------------------------------------- 8: the frame

@pytest.mark.gpu
def test_the_frame_shows_what_stands_behind_the_holes(aref, tref):
    """frame(post_pass=True, textures=True) -> resolve -> attributes(textures=True) -> shade(shadow="trace", textures=True) at 320 x 192, and the
    entry point inside a captured graph"""
    import torch
    import test_shadow_alpha_cpu as SC
    import test_shadowtrace_gpu as TS
    from niagara_amd import pipeline as P
    from niagara_amd._lib import NvError
    s, _ = SC.cutout_occluder()
    s["draws"]["position"][s["wall"]] += np.array(RA.WALL_SHIFT, np.float32)
    w, h = s["viewport"]
    wall = s["wall"][0]
    pipe = TS._pipeline(s, 0)
    try:
        vis = pipe.new_visibility()
        with pytest.raises(NvError) as e:
            pipe.frame(s["cull"], post_pass=True, visibility=vis, textures=True, materials=s["materials"])
        assert "set_textures" in str(e.value)
        pipe.set_textures(s["textures"])
        with pytest.raises(NvError) as e:
            pipe.frame(s["cull"], post_pass=True, visibility=vis, textures=True)
        assert "materials=" in str(e.value)

        def records(**kw):
            post = {}

            def grab(name):
                if name == "post":
                    c4, cc4 = pipe.dccb.cpu().numpy().view(np.uint32), pipe.ccb.cpu().numpy().view(np.uint32).copy()
                    post.update(commands=P.from_device(pipe.dcb, L.TASKCMD)[:int(c4[1]) * 64].copy(), cc4=cc4,
                                cib=pipe.cib.cpu().numpy().view(np.uint32)[:int(cc4[2]) * 256].copy())
            for _ in range(2):
                pipe.frame(s["cull"], post_pass=True, visibility=vis, on_phase=grab, **kw)
            res = pipe.resolve(s["cull"], vis)
            pipe.ctx.status()
            return P.from_device(res["records"], L.VISRECORD).copy(), res, post
        solid, _, _ = records()
        rec, res, post = records(textures=True, materials=s["materials"])
        behind = np.isin(rec["drawId"], s["hidden"])
        print("pixels that resolve to the wall / to a box behind it: %d / %d with textures, %d / %d without" %
              (int((rec["drawId"] == wall).sum()), int(behind.sum()), int((solid["drawId"] == wall).sum()), int(np.isin(solid["drawId"], s["hidden"]).sum())))
        assert behind.sum() >= 1 and not np.isin(solid["drawId"], s["hidden"]).any()
        # every pixel that resolves to the wall is one the restatement keeps, on the post launch's own list
        descs, texels = tref.decode_set(s["textures"])
        g = RR.globals_for(s["cull"], (w, h), 1)
        out = aref.raster(g, post["commands"], s["draws"], s["meshlets"], s["data"], s["vertices"], post["cib"], post["cc4"], w, h, stable=1, log=2 * w * h,
                          materials=s["materials"], descs=descs, texels=texels)
        smp = out["samples"]
        kept = np.zeros(w * h, bool)
        sel = (smp["drawId"] == wall) & (smp["keep"] == 1)
        kept[smp["py"][sel].astype(np.int64) * w + smp["px"][sel]] = True
        assert sel.sum() > 1000 and kept[rec["drawId"] == wall].all()
        # the rest of the chain runs on it
        att = pipe.attributes(s["cull"], res["records"], s["materials"], attributes=False, textures=True)
        pipe.build_rt_scene(s["meshes"], s["indices"], s["vertices"], s["draws"], texcoords=True)
        color = pipe.shade(s["cull"], att["gbuffer0"], att["gbuffer1"], (0.0, 0.0, 0.0), TS.SUN, shadow="trace", blur=False, textures=True, materials=s["materials"])
        pipe.ctx.status()
        assert (color.cpu().numpy().reshape(-1)[behind] != 0).any()

        # the post raster inside a captured graph replays to the same bytes
        depth0 = torch.zeros_like(pipe.depth)
        eager_v = pipe.new_visibility()
        tot, alpha = torch.zeros(4, dtype=torch.int64, device=pipe.ctx.device), torch.zeros(2, dtype=torch.int64, device=pipe.ctx.device)

        def raster(v):
            pipe.render_depth(s["cull"], late=True, post_pass=1, visibility=v, totals4=tot, textures=True, materials=mat, alpha_totals2=alpha)
        mat = P.to_device(np.ascontiguousarray(s["materials"], L.MATERIAL), pipe.ctx.device)
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            pipe.depth.copy_(depth0)
            raster(eager_v)
            torch.cuda.synchronize()
            eager = [t.cpu().numpy().copy() for t in (pipe.depth, eager_v, tot, alpha)]
            assert eager[3][0] > 1000 and eager[2][3] > 1000
            graph_v = pipe.new_visibility()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=st):
                raster(graph_v)
            torch.cuda.synchronize()
            for _ in range(2):
                pipe.depth.copy_(depth0), graph_v.zero_(), tot.zero_(), alpha.zero_()
                graph.replay()
                torch.cuda.synchronize()
                for t, e in zip((pipe.depth, graph_v, tot, alpha), eager):
                    assert t.cpu().numpy().tobytes() == e.tobytes()
        pipe.ctx.status()
    finally:
        pipe.ctx.close()
