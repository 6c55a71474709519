"""The alpha-tested depth raster on the CPU: the restatement tests/raster_alpha_ref.c pinned to what is already pinned — its
keep or drop of every covered sample equals the discard flag of the attribute pass's restatement (tests/texture_ref.c, held bit for bit to
mesh.frag.glsl by tests/test_shading_vs_ref.py) for the same triangle at the same pixel — and each case of the rule on its own.  The GPU file
(tests/test_raster_alpha_gpu.py) compares nv_rasterdepth_textured with this restatement; the conditions its comparison relies on (paths
reached, the share of undecided samples) are asserted here on the restatement's side."""
import numpy as np
import pytest

import raster_alpha_ref as RA
import raster_clip_ref as RC
import raster_ref as RR
import texture_ref as TR
import visattr_ref as VA
from niagara_amd import layouts as L

UNDECIDED_CAP = 1e-3  # of the alpha-tested covered samples (the issue's condition; the texture's geometry puts the share near 1e-5)


@pytest.fixture(scope="session")
def aref(tmp_path_factory):
    return RA.load(tmp_path_factory.mktemp("raster_alpha_ref_cpu"))


@pytest.fixture(scope="session")
def tref(tmp_path_factory):
    return TR.load(tmp_path_factory.mktemp("texture_ref_alpha_cpu"))


@pytest.fixture(scope="session")
def rref(tmp_path_factory):
    return RR.load(tmp_path_factory.mktemp("raster_ref_alpha_cpu"))


@pytest.fixture(scope="session")
def clib(tmp_path_factory):
    return RC.load(tmp_path_factory.mktemp("raster_clip_ref_alpha_cpu"))


def _tex(s):
    return dict(materials=s["materials"], descs=s["descs"], texels=s["texels"])


def _same(a, depth, vis, totals):
    assert a["depth"].view(np.uint32).tobytes() == depth.view(np.uint32).tobytes()
    assert a["visibility"].tobytes() == vis.tobytes()
    assert a["totals"].tolist() == totals.tolist()


def _flags_of_the_attribute_pass(tref, s, samples, w, h):
    """per sample: the discard flag tr_attributes gives the record {draw, meshlet, triangle} at the sample's pixel.  A pixel covered k times is
    shaded in k images"""
    flag = np.zeros(len(samples), bool)
    pixel = samples["py"].astype(np.int64) * w + samples["px"]
    order = np.argsort(pixel, kind="stable")
    rank = np.zeros(len(samples), np.int64)  # the sample's number among those of its pixel
    sp = pixel[order]
    start = np.r_[0, np.flatnonzero(sp[1:] != sp[:-1]) + 1]
    rank[order] = np.arange(len(sp)) - np.repeat(start, np.diff(np.r_[start, len(sp)]))
    for layer in range(int(rank.max()) + 1):
        sel = np.flatnonzero(rank == layer)
        rec = np.zeros(w * h, L.VISRECORD)
        rec["drawId"] = 0xffffffff
        rec["drawId"][pixel[sel]], rec["meshletIndex"][pixel[sel]], rec["triangle"][pixel[sel]] = samples["drawId"][sel], samples["meshlet"][sel], samples["triangle"][sel]
        with np.errstate(all="ignore"):
            out = tref.attributes(s["g"], rec, w, h, s["draws"], s["meshlets"], s["data"], s["vertices"], s["materials"], s["descs"], s["texels"], taps=True)
        fl = out["flags"][pixel[sel]]
        assert ((fl & VA.SHADED) != 0).all() and not (fl & TR.NOT_SAMPLED).any()
        mi = out["attributes"]["materialIndex"][pixel[sel]]
        alpha = s["materials"]["diffuseFactor"][mi, 3] * np.where(s["materials"]["albedoTexture"][mi] > 0, out["taps"][pixel[sel], 0, 3], np.float32(1))
        flag[sel] = alpha < np.float32(0.5)  # test_shading_vs_ref.py: ref["discard"] == shaded & (post > 0) & (alpha < 0.5)
    return flag, int(rank.max()) + 1


# ---------------------------------------------------------------------------------------------------------------- 1, 4: pinned

def test_keep_or_drop_is_the_attribute_pass_discard_flag(aref, tref):
    """the cut-out occluder scene (wall in the post pass) and the cut-out floor under the camera with near clip on (pieces: the ORIGINAL
    triangle's corners): zero differences between the restatement's keep / drop and tr_attributes' flag, sample by sample"""
    kept = dropped = 0
    for name, s, clip in (("occluder", RA.occluder(tref, (320, 192), True), 0), ("floor", RA.floor(tref, (320, 192), True), 1),
                          ("floor, no clip", RA.floor(tref, (67, 37), False), 0)):
        w, h = s["viewport"]
        out = aref.raster(*RA.args(s), w, h, near_clip=clip, log=4 * w * h, **_tex(s))
        smp = out["samples"]
        assert (smp["status"] == RA.SAMPLED).all()
        flag, layers = _flags_of_the_attribute_pass(tref, s, smp, w, h)
        diff = int((flag != (smp["keep"] == 0)).sum())
        print("%s %dx%d: %d covered samples in %d layers, %d kept, %d dropped, %d clipped pieces, %d differences" %
              (name, w, h, len(smp), layers, int(smp["keep"].sum()), int((smp["keep"] == 0).sum()), out["counters"]["tested_clipped"], diff))
        assert diff == 0
        assert clip == 0 or out["counters"]["tested_clipped"] >= 4
        assert int(out["totals"][3]) == int(smp["keep"].sum()) and int(out["alpha"][0]) == int((smp["keep"] == 0).sum())
        # tests/test_raster_clip_cpu.py's property: a pixel centre is covered at most once per triangle, pieces included
        key = (smp["py"].astype(np.int64) * w + smp["px"]) << 32 | smp["index"].astype(np.int64) << 7 | smp["triangle"]
        assert len(np.unique(key)) == len(key)
        kept, dropped = kept + int(smp["keep"].sum()), dropped + int((smp["keep"] == 0).sum())
    assert kept >= 500 and dropped >= 500


# ---------------------------------------------------------------------------------------------------------------- 2: the launches that do not test

def test_without_post_pass_or_materials_it_is_the_plain_raster(aref, tref, rref, clib):
    s = RA.occluder(tref, (67, 37), True)
    w, h = s["viewport"]
    for clip in (0, 1):
        for pp in (0, 1):
            g = RR.globals_for(s["cull"], (w, h), pp)
            plain = clib.cluster(clip).raster(g, *RA.args(s)[1:], w, h, visibility=True)
            if clip == 0:  # rr_rasterdepth itself
                plain = rref.raster(g, *RA.args(s)[1:], w, h, visibility=True)
            for tex in [dict()] + ([_tex(s)] if pp == 0 else []):  # no materials with either postPass; postPass == 0 with materials
                out = aref.raster(g, *RA.args(s)[1:], w, h, near_clip=clip, **tex)
                _same(out, *plain)
                assert out["alpha"].tolist() == [0, 0] and plain[2][3] > 0
    # and with them the launch differs
    out = aref.raster(*RA.args(s), w, h, **_tex(s))
    assert out["alpha"][0] > 0 and out["depth"].tobytes() != plain[0].tobytes()


# ---------------------------------------------------------------------------------------------------------------- 3: the rule, case by case

def _two_draws(tref):
    """the occluder scene's wall (material 0, draw 0) and its first box beside the wall (another material), both in one post launch"""
    s = RA.occluder(tref, (67, 37), True)
    box = s["beside"][0]
    s["draws"]["materialIndex"][box] = 1
    s["commands"], s["cib"], s["cc4"] = RA.draw_list(s, [0, box])
    alone = dict(s)
    alone["commands"], alone["cib"], alone["cc4"] = RA.draw_list(s, [box])
    # the box keeps the slot indices it has in the list of both: its words must be comparable
    alone["cib"] = s["cib"].copy()
    wall_slots = int(s["meshes"][0]["lods"][0]["meshletCount"])
    alone["cib"][:wall_slots] = 0xffffffff
    alone["commands"] = s["commands"]
    return s, alone


RULE_CASES = ("factor 0.49", "factor 0.5", "materialIndex past the table", "texture id past the table", "descriptor refused", "NaN uv")


def rule_case(tref, name):
    """(scene, keyword arguments of the raster, expectation): "none": no sample of the wall survives; "all": every sample does, "all-unevaluated":
    and is counted as unevaluated"""
    s, alone = _two_draws(tref)
    kw = _tex(s)
    m = s["materials"].copy()
    kw["materials"] = m
    m["albedoTexture"][1] = 0  # the box: opaque from its factor
    m["diffuseFactor"][1, 3] = 1.0
    if name.startswith("factor"):
        m["albedoTexture"][0] = 0
        m["diffuseFactor"][0, 3] = np.float32(0.49 if name == "factor 0.49" else 0.5)
        return s, alone, kw, "none" if name == "factor 0.49" else "all"
    if name == "materialIndex past the table":
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
        s["vertices"] = alone["vertices"] = v
        return s, alone, kw, "all"
    return s, alone, kw, "all-unevaluated"


@pytest.mark.parametrize("name", RULE_CASES)
def test_each_rule_case_changes_the_output_where_it_should(name, aref, tref, rref):
    s, alone, kw, expect = rule_case(tref, name)
    w, h = s["viewport"]
    plain = rref.raster(*RA.args(s), w, h, visibility=True)          # both draws, no test
    box = rref.raster(*RA.args(alone), w, h, visibility=True)        # the box alone
    wall_samples = int(plain[2][3]) - int(box[2][3])
    out = aref.raster(*RA.args(s), w, h, **kw)
    print("%s: %d samples of the wall, %d of the box; kept %d, dropped %d, unevaluated %d" %
          (name, wall_samples, int(box[2][3]), int(out["totals"][3]), int(out["alpha"][0]), int(out["alpha"][1])))
    assert wall_samples > 500 and box[2][3] > 0
    assert int(out["totals"][3]) + int(out["alpha"][0]) == int(plain[2][3])
    assert out["totals"][:3].tolist() == plain[2][:3].tolist()
    if expect == "none":
        assert out["depth"].tobytes() == box[0].tobytes() and out["visibility"].tobytes() == box[1].tobytes()
        assert out["alpha"].tolist() == [wall_samples, 0]
    else:
        assert out["depth"].tobytes() == plain[0].tobytes() and out["visibility"].tobytes() == plain[1].tobytes()
        assert out["alpha"].tolist() == [0, wall_samples if expect == "all-unevaluated" else 0]
    assert (out["counters"]["nan_alpha"] > 500) == (name == "NaN uv")


# ---------------------------------------------------------------------------------------------------------------- 5: what the GPU file relies on

def gpu_cases(tref):
    """name -> (scene, near clip): the inputs tests/test_raster_alpha_gpu.py runs with a mip chain in play"""
    return {"occluder 67x37": (RA.occluder(tref, (67, 37), True), 0), "occluder 320x192, 256-texel set": (RA.occluder(tref, (320, 192), True, size=256), 0),
            "floor 320x192, near clip": (RA.floor(tref, (320, 192), True), 1), "slot sequence": (RA.sequence(tref, True, 3 * 1024), 0)}


def test_undecided_samples_stay_under_the_cap_on_the_gpu_files_inputs(aref, tref):
    aref.hits()
    for name, (s, clip) in gpu_cases(tref).items():
        w, h = s["viewport"]
        out = aref.raster(*RA.args(s), w, h, near_clip=clip, band=True, **_tex(s))
        c, hits = out["counters"], aref.hits()
        print("%s: %d alpha-tested samples, %d undecided, small / large pieces %d / %d, samples per level %s, with a fractional level %d" %
              (name, c["tested_samples"], c["undecided"], c["tested_small"], c["tested_large"], hits[:6].tolist(), int(hits[15])))
        assert c["tested_samples"] > 500 and c["undecided"] <= UNDECIDED_CAP * c["tested_samples"]
        assert out["undecided"].sum() <= c["undecided"]
        assert hits[15] > 0  # a blend of two levels is in play: the device's log2 matters
    # the rule cases run under the band rule too
    for name in RULE_CASES:
        s, _, kw, _ = rule_case(tref, name)
        c = aref.raster(*RA.args(s), 67, 37, band=True, **kw)["counters"]
        assert c["undecided"] <= UNDECIDED_CAP * c["tested_samples"]
