"""The classic path with textures on the CPU: the restatement of nv_rasterdepth_indexed_textured
(tests/raster_indexed_alpha_ref.c) pinned to what is already pinned — its keep or drop of every covered sample equals the discard decision of
the attribute pass's restatement (tests/texture_ref.c) for the same triangle at the same pixel, without a test it is the indexed restatement
(tests/visindexed_ref.c) bit for bit, and over the index buffer recovered from the meshlets it is the cluster restatement
(tests/raster_alpha_ref.c) — and each case of the rule on its own.  The GPU file (tests/test_visindexed_textured_gpu.py) compares the four
new entry points with these restatements; the conditions its cases rely on are asserted here on the restatement's side."""
import os
import re

import numpy as np
import pytest

import raster_alpha_ref as RA
import raster_indexed_alpha_ref as RIA
import raster_ref as RR
import test_raster_alpha_cpu as AC
import texture_ref as TR
import visattr_ref as VA
import visindexed_ref as VI
from niagara_amd import layouts as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("nv_visibility_attributes_indexed_textured", "nv_visibility_attributes_indexed_blocks", "nv_rasterdepth_indexed_textured",
                "nv_rasterdepth_indexed_blocks")


@pytest.fixture(scope="session")
def riaref(tmp_path_factory):
    return RIA.load(tmp_path_factory.mktemp("raster_indexed_alpha_ref_cpu"))


@pytest.fixture(scope="session")
def aref(tmp_path_factory):
    return RA.load(tmp_path_factory.mktemp("raster_alpha_ref_vit"))


@pytest.fixture(scope="session")
def tref(tmp_path_factory):
    return TR.load(tmp_path_factory.mktemp("texture_ref_vit"))


@pytest.fixture(scope="session")
def viref(tmp_path_factory):
    return VI.load(tmp_path_factory.mktemp("visindexed_ref_vit"))


@pytest.fixture(scope="session")
def iaref(tmp_path_factory):
    import visattr_indexed_ref as VAI
    return VAI.load(tmp_path_factory.mktemp("visattr_indexed_ref_vit"))


def test_abi_has_the_four_entry_points():
    from niagara_amd import _lib
    header = open(os.path.join(ROOT, "include", "niagara_vis.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)


# ---------------------------------------------------------------------------------------------------------------- 1: pinned to the attribute pass

def records_of(s, samples, sel, n):
    """one NvVisIndexedRecord per pixel: the triangle of the samples `sel` at their pixels (at most one of them per pixel)"""
    w = s["viewport"][0]
    rec = np.zeros(n, L.VISINDEXEDRECORD)
    rec["drawId"] = 0xffffffff
    c = s["icommands"][samples["command"][sel]]
    at = samples["py"][sel].astype(np.int64) * w + samples["px"][sel]
    rec["drawId"][at], rec["vertexOffset"][at] = c["drawId"], c["vertexOffset"]
    rec["indexPosition"][at] = c["firstIndex"] + 3 * samples["triangle"][sel]
    return rec, at


def discard_of_the_attribute_pass(tref, iaref, s, samples):
    """per sample: albedo.a < 0.5 as the textured indexed attribute restatement shades the sample's triangle at the sample's pixel.  A pixel
    covered k times is shaded in k images"""
    w, h = s["viewport"]
    flag = np.zeros(len(samples), bool)
    pixel = samples["py"].astype(np.int64) * w + samples["px"]
    order = np.argsort(pixel, kind="stable")
    rank = np.zeros(len(samples), np.int64)
    sp = pixel[order]
    start = np.r_[0, np.flatnonzero(sp[1:] != sp[:-1]) + 1]
    rank[order] = np.arange(len(sp)) - np.repeat(start, np.diff(np.r_[start, len(sp)]))
    for layer in range(int(rank.max()) + 1):
        sel = np.flatnonzero(rank == layer)
        rec, at = records_of(s, samples, sel, w * h)
        out = RIA.attributes(tref, iaref, s["g"], rec, w, h, s["draws"], s["indices"], s["vertices"], s["materials"], s["descs"], s["texels"], taps=True)
        fl = out["flags"][at]
        assert ((fl & VA.SHADED) != 0).all() and not (fl & TR.NOT_SAMPLED).any()
        mi = out["attributes"]["materialIndex"][at]
        alpha = s["materials"]["diffuseFactor"][mi, 3] * np.where(s["materials"]["albedoTexture"][mi] > 0, out["taps"][at, 0, 3], np.float32(1))
        flag[sel] = alpha < np.float32(0.5)
    return flag, int(rank.max()) + 1


def test_keep_or_drop_is_the_attribute_pass_discard_decision(riaref, tref, iaref):
    """the cut-out wall in the post pass, and the cut-out floor under the camera with near clip on (pieces: the ORIGINAL triangle's corners)"""
    for name, s, clip in (("occluder", RIA.occluder(tref, (320, 192), True), 0), ("floor", RIA.floor(tref, (320, 192), True), 1)):
        w, h = s["viewport"]
        out = riaref.raster(*RIA.args(s), w, h, s["offsets"], near_clip=clip, log=4 * w * h, **RIA.tex(s))
        smp = out["samples"]
        assert (smp["status"] == RIA.SAMPLED).all()
        flag, layers = discard_of_the_attribute_pass(tref, iaref, s, smp)
        diff = int((flag != (smp["keep"] == 0)).sum())
        print("%s %dx%d: %d covered samples in %d layers, %d kept, %d dropped, %d differences" %
              (name, w, h, len(smp), layers, int(smp["keep"].sum()), int((smp["keep"] == 0).sum()), diff))
        assert diff == 0
        assert int(smp["keep"].sum()) >= 500 and int((smp["keep"] == 0).sum()) >= 500
        assert int(out["totals"][3]) == int(smp["keep"].sum()) and out["alpha"].tolist() == [int((smp["keep"] == 0).sum()), 0]
        if clip:  # the clip is in play: without it the same launch covers other samples
            assert riaref.raster(*RIA.args(s), w, h, s["offsets"], **RIA.tex(s))["depth"].tobytes() != out["depth"].tobytes()


# ---------------------------------------------------------------------------------------------------------------- 2: the launches that do not test

def test_without_post_pass_or_materials_it_is_the_indexed_restatement(riaref, tref, viref):
    s = RIA.floor(tref, (67, 37), True)
    w, h = s["viewport"]
    for clip in (0, 1):
        for pp in (0, 1):
            g = RR.globals_for(s["cull"], (w, h), pp)
            plain = viref.raster(g, *RIA.args(s)[1:], w, h, s["offsets"], near_clip=clip)
            for tex in [dict()] + ([RIA.tex(s)] if pp == 0 else []):  # no materials with either postPass; postPass == 0 with materials
                out = riaref.raster(g, *RIA.args(s)[1:], w, h, s["offsets"], near_clip=clip, **tex)
                assert out["depth"].view(np.uint32).tobytes() == plain[0].view(np.uint32).tobytes() and out["visibility"].tobytes() == plain[1].tobytes()
                assert out["totals"].tolist() == plain[2].tolist() and out["alpha"].tolist() == [0, 0] and plain[2][3] > 0
                both_null = riaref.raster(g, *RIA.args(s)[1:], w, h, None, near_clip=clip, **tex)  # depth only
                assert both_null["visibility"] is None and both_null["depth"].tobytes() == out["depth"].tobytes()
                assert both_null["totals"].tolist() == plain[2].tolist()
    out = riaref.raster(*RIA.args(s), w, h, s["offsets"], **RIA.tex(s))  # and with both the launch differs
    assert out["alpha"][0] > 0 and out["depth"].tobytes() != plain[0].tobytes()


# ---------------------------------------------------------------------------------------------------------------- 3: the rule, case by case

RULE_CASES = ("materialIndex past the table", "factor 0.4", "factor 0.6", "texture id past the table", "descriptor refused", "NaN uv")


def rule_case(tref, name):
    """(scene of two commands: the wall, material 0, and a box beside it, opaque from material 1; the box alone; the raster's keyword arguments;
    expectation).  "none": no sample of the wall survives; "all": every sample does; "all-unevaluated": and is counted as unevaluated"""
    s, _ = AC._two_draws(tref)
    box = int(s["beside"][0])
    kw = RIA.tex(s)
    m = s["materials"].copy()
    kw["materials"] = m
    m["albedoTexture"][1] = 0
    m["diffuseFactor"][1, 3] = 1.0
    expect = "all-unevaluated"
    if name.startswith("factor"):
        m["albedoTexture"][0] = 0
        m["diffuseFactor"][0, 3] = np.float32(0.4 if name == "factor 0.4" else 0.6)
        expect = "none" if name == "factor 0.4" else "all"
    elif name == "materialIndex past the table":
        s["draws"]["materialIndex"][0] = len(m)
    elif name == "texture id past the table":
        m["albedoTexture"][0] = len(s["descs"])
    elif name == "descriptor refused":
        d = s["descs"].copy()
        d["levels"][1] = 0
        kw["descs"] = d
    else:
        v = s["vertices"].copy()
        mesh = s["meshes"][0]
        first, count = int(mesh["vertexOffset"]), int(mesh["vertexCount"])
        v["tu"][first:first + count] = 0x7e00
        s["vertices"] = v
        expect = "all"
    return RIA.indexed(s, [0, box]), RIA.indexed(s, [box]), kw, expect


@pytest.mark.parametrize("name", RULE_CASES)
def test_each_rule_case_changes_the_output_where_it_should(name, riaref, tref, viref):
    s, alone, kw, expect = rule_case(tref, name)
    w, h = s["viewport"]
    plain = viref.raster(*RIA.args(s), w, h, s["offsets"])       # both commands, no test
    box = viref.raster(*RIA.args(alone), w, h, alone["offsets"])  # the box alone (its triangles keep their names: the offsets are the scene's)
    wall_samples = int(plain[2][3]) - int(box[2][3])
    with np.errstate(all="ignore"):
        out = riaref.raster(*RIA.args(s), w, h, s["offsets"], log=4 * w * h, **kw)
    print("%s: %d samples of the wall, %d of the box; kept %d, dropped %d, unevaluated %d" %
          (name, wall_samples, int(box[2][3]), int(out["totals"][3]), int(out["alpha"][0]), int(out["alpha"][1])))
    assert wall_samples > 500 and box[2][3] > 0
    assert int(out["totals"][3]) + int(out["alpha"][0]) == int(plain[2][3])
    assert out["totals"][:2].tolist() == [2, plain[2][1]] and out["totals"][2] == plain[2][2]
    if expect == "none":
        assert out["depth"].tobytes() == box[0].tobytes() and out["visibility"].tobytes() == box[1].tobytes()
        assert out["alpha"].tolist() == [wall_samples, 0]
    else:
        assert out["depth"].tobytes() == plain[0].tobytes() and out["visibility"].tobytes() == plain[1].tobytes()
        assert out["alpha"].tolist() == [0, wall_samples if expect == "all-unevaluated" else 0]
    nan = np.isnan(out["samples"]["alpha"])
    assert (nan.sum() > 500) == (name == "NaN uv") and (out["samples"]["keep"][nan] == 1).all()


# ---------------------------------------------------------------------------------------------------------------- 4: the cluster restatement

@pytest.mark.parametrize("viewport", [(67, 37), (320, 192)])
def test_the_cluster_restatement_draws_the_same_image(viewport, riaref, aref, tref):
    """the wall's meshlets through raster_alpha_ref.c and its index buffer (synth.indexed_geometry: the meshlets' triangles, in order) through
    the indexed restatement: the same depth image, and per pixel the same number of kept and of dropped samples"""
    s = RIA.occluder(tref, viewport, True)
    w, h = viewport
    a = aref.raster(*RA.args(s), w, h, stable=1, log=4 * w * h, **RIA.tex(s))
    b = riaref.raster(*RIA.args(s), w, h, s["offsets"], log=4 * w * h, **RIA.tex(s))
    assert a["depth"].view(np.uint32).tobytes() == b["depth"].view(np.uint32).tobytes()
    assert a["totals"][2:].tolist() == b["totals"][2:].tolist() and a["alpha"].tolist() == b["alpha"].tolist()
    for keep in (0, 1):
        per_pixel = [np.bincount((o["samples"]["py"].astype(np.int64) * w + o["samples"]["px"])[o["samples"]["keep"] == keep], minlength=w * h) for o in (a, b)]
        assert (per_pixel[0] == per_pixel[1]).all() and per_pixel[0].sum() > 0


# ---------------------------------------------------------------------------------------------------------------- 5: what the GPU file relies on

def frame_on_the_restatements(riaref, viref, s, textures):
    """the classic frame's three phases on the CPU, everything visible: every opaque draw (post_pass 0), then the post launch — the wall — over
    the loaded targets, with or without the alpha test: (depth, visibility, the post launch's output)"""
    w, h = s["viewport"]
    opaque = RIA.indexed(s, [int(d) for d in np.flatnonzero(s["draws"]["postPass"] == 0)])
    g0 = RR.globals_for(s["cull"], (w, h), 0)
    depth, vis, _ = viref.raster(g0, *RIA.args(opaque)[1:], w, h, s["offsets"])
    post = riaref.raster(*RIA.args(s), w, h, s["offsets"], depth=depth, vis=vis, log=4 * w * h, **(RIA.tex(s) if textures else dict()))
    return post


@pytest.mark.parametrize("viewport", [(67, 37), (320, 192)])
def test_the_wall_keeps_and_drops_samples_and_a_draw_behind_it_shows(viewport, riaref, viref, tref):
    s = RIA.occluder(tref, viewport, True)
    w, h = viewport
    wall = [int(d) for d in s["wall"]]
    textured, solid = (frame_on_the_restatements(riaref, viref, s, t) for t in (True, False))
    smp = textured["samples"]
    assert np.isin(s["icommands"]["drawId"][smp["command"]], wall).all()
    assert int(smp["keep"].sum()) >= 1 and int((smp["keep"] == 0).sum()) >= 1
    behind = [np.isin(viref.resolve(s["cull"], o["visibility"], s["draws"], s["meshes"], s["offsets"])["records"]["drawId"], s["hidden"]).sum()
              for o in (textured, solid)]
    print("%dx%d: the wall keeps %d samples and drops %d; pixels that resolve to a box behind it: %d with the test, %d without" %
          (w, h, int(smp["keep"].sum()), int((smp["keep"] == 0).sum()), behind[0], behind[1]))
    assert behind[0] >= 1 and behind[1] == 0


# ---------------------------------------------------------------------------------------------------------------- the code objects

@pytest.mark.parametrize("source,kernel,count", [("rasterindexed_alpha", "rasterindexed_kernel", 2), ("rasterindexed_blocks", "rasterindexed_kernel", 2),
                                                 ("visattr_indexed_tex", "visibility_attributes_kernel", 1),
                                                 ("visattr_indexed_blocks", "visibility_attributes_kernel", 1),
                                                 ("rasterdepth", "rasterdepth_kernel", 4), ("rasterdepth_alpha", "rasterdepth_kernel", 4),
                                                 ("rasterindexed", "rasterindexed_kernel", 2), ("rasterindexed_vis", "rasterindexed_kernel", 2)])
def test_new_kernels_use_no_scratch_memory(source, kernel, count, tmp_path):
    """the classic path's textured instantiations and the raster kernels of both paths, compiled with the Makefile's flags: 0 bytes of private segment, no spilled vector register"""
    import subprocess
    csrc = os.path.join(ROOT, "niagara_amd", "csrc")
    asm = str(tmp_path / (source + ".s"))
    subprocess.check_call(["hipcc", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize", "--offload-arch=gfx950", "--cuda-device-only",
                           "-S", os.path.join(csrc, source + ".hip"), "-o", asm], stderr=subprocess.DEVNULL)
    text = open(asm).read()
    entries = [e for e in text[text.index("amdhsa.kernels:"):].split("\n  - .")[1:] if kernel in e.split(".name:")[1].split()[0]]
    assert len(entries) == count
    for e in entries:
        field = lambda name: int(e.split("." + name + ":")[1].split()[0])
        print("%s: %d VGPRs, %d SGPRs, %d bytes LDS, %d bytes scratch" % (e.split(".name:")[1].split()[0], field("vgpr_count"), field("sgpr_count"),
                                                                         field("group_segment_fixed_size"), field("private_segment_fixed_size")))
        assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0
