"""The shading fixtures without the reference tree and without a GPU: tests/golden/shade/*.npz hold what the reference's own
shaders, run on the CPU, make of fixed inputs (tests/golden/generate.py, section `shade`).  The fp32 builds of the restatements replay every
fixture with zero differences — words and values handed to the stores, a NaN matching a NaN — so the GPU replays of test_shade_gpu.py,
test_bloom_gpu.py, test_visattr_gpu.py and test_textures_gpu.py may keep the bounds those files derive for glibc's against the device's pow /
exp2.  The 90 % (99 % for pass 0) share of equal channels those bounds ask for is a condition on the inputs: the last test moves the
restatement's pow / exp2 results by 2 ULP on the fixtures' inputs and stays inside both conditions, as test_shade_cpu.py does on its own."""
import os

import numpy as np
import pytest

import bloom_ref as BR
import shade_cases as SC
import shade_ref as SR
import texture_ref as TR
import visattr_ref as VA

same = SC.same_bits
FILES = SC.FIXTURES


@pytest.fixture(scope="module")
def sref(tmp_path_factory):
    return SR.load(tmp_path_factory.mktemp("shade_ref_fixtures"))


@pytest.fixture(scope="module")
def bref(tmp_path_factory):
    return BR.load(tmp_path_factory.mktemp("bloom_ref_fixtures"))


@pytest.fixture(scope="module")
def aref(tmp_path_factory):
    return VA.load(tmp_path_factory.mktemp("visattr_ref_fixtures"))


@pytest.fixture(scope="module")
def tref(tmp_path_factory):
    return TR.load(tmp_path_factory.mktemp("texture_ref_fixtures"))


def _zero(name, ok):
    ok = np.asarray(ok)
    print("%s: %d elements, %d differ" % (name, ok.size, int((~ok).sum())))
    assert ok.all(), "%s: %d of %d differ, first at %s" % (name, int((~ok).sum()), ok.size, np.argwhere(~ok)[:4].tolist())


_size, _sd = SC.fixture_size, SC.fixture_shade_data


def test_the_fixtures_are_the_three_sizes_and_stay_small():
    assert [os.path.basename(p) for p in FILES] == sorted("%dx%d.npz" % s for s in SC.FIXTURE_SIZES)
    total = sum(os.path.getsize(p) for p in FILES)
    print("tests/golden/shade: %d bytes" % total)
    assert total <= os.path.getsize(os.path.join(SC.HERE, "golden", "mesh", "kitten.npz"))


@pytest.mark.parametrize("path", FILES, ids=SC.FIXTURE_IDS)
def test_shadow_and_final_replay(path, sref, bref):
    f = np.load(path)
    w, h = _size(f)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    for cb in (0, 1):
        got, value = sref.shadow_fill(f["shadow"], f["depth"], cb, value=True)
        owned = (~(y ^ cb) & 1) == (x & 1)
        _zero("fill cb %d, words" % cb, got == f["fill%d_words" % cb])
        _zero("fill cb %d, values" % cb, same(value[owned], f["fill%d_value" % cb][owned]))
    for direction in (0, 1):
        got, value = sref.shadow_blur(f["shadow"], f["depth"], direction, float(f["znear"]), value=True)
        _zero("blur direction %d, words" % direction, got == f["blur%d_words" % direction])
        _zero("blur direction %d, values" % direction, same(value, f["blur%d_value" % direction]))
    for shadows in (0, 1):
        shadow = f["shadow"] if shadows else None
        got, value = sref.shade_final(_sd(f, shadows), f["gbuffer0"], f["gbuffer1"], f["depth"], shadow, value=True)
        _zero("final shadows %d, words" % shadows, got == f["final%d_words" % shadows])
        _zero("final shadows %d, values" % shadows, same(value[..., :3] + value[..., 3:], f["final%d_value" % shadows]))
        got, value = bref.shade_final_bloom(_sd(f, shadows), f["gbuffer0"], f["gbuffer1"], f["depth"], shadow, f["bloom0"], value=True)
        _zero("final + bloom shadows %d, words" % shadows, got == f["finalbloom%d_words" % shadows])
        _zero("final + bloom shadows %d, values" % shadows, same(value[..., :3] + value[..., 3:], f["finalbloom%d_value" % shadows]))


@pytest.mark.parametrize("path", FILES, ids=SC.FIXTURE_IDS)
def test_bloom_replay(path, bref):
    f = np.load(path)
    d = BR.desc(*_size(f))
    got, value = bref.extract(f["bloom_g0"], value=True)
    _zero("extract, words", got == f["extract_words"])
    _zero("extract, values", same(value, f["extract_value"]))
    given = BR.unpack(f["levels"], d)
    down = [bref.downsample(given[l - 1], value=True) for l in range(1, d["levels"])]
    _zero("downsample, words", BR.pack([given[0]] + [a for a, _ in down]) == f["down_words"])
    _zero("downsample, values", same(np.concatenate([b.reshape(-1, 3) for _, b in down]), f["down_value"]))
    given = BR.unpack(f["levels2"], d)
    for k, radius in enumerate(SC.RADII):
        up = [bref.upsample(given[l + 1], given[l], radius, value=True) for l in range(d["levels"] - 1)]
        _zero("upsample radius %g, words" % radius, BR.pack([a for a, _ in up] + [given[-1]]) == f["up%d_words" % k])
        _zero("upsample radius %g, values" % radius, same(np.concatenate([b.reshape(-1, 3) for _, b in up]), f["up%d_value" % k]))
    _zero("the loop", BR.pack(bref.chain(f["bloom_g0"])) == f["loop_words"])


@pytest.mark.parametrize("path", FILES, ids=SC.FIXTURE_IDS)
def test_fragment_stage_replay(path, aref, tref):
    f = np.load(path)
    w, h = _size(f)
    s, rec = SC.fixture_frag_scene(path, f)
    plain = SC.untextured(s["materials"])
    want = aref.attributes(s["g"], rec, w, h, s["draws"], s["meshlets"], s["data"], s["vertices"], plain)
    shaded = (want["flags"] & VA.SHADED) != 0
    _zero("factor-only, gbuffer0", want["gbuffer0"] == f["frag_gbuffer0"])
    _zero("factor-only, gbuffer1", want["gbuffer1"] == f["frag_gbuffer1"])
    alpha = plain["diffuseFactor"][want["attributes"]["materialIndex"], 3]
    _zero("factor-only, discard under POST 1", f["frag_discard"] == (shaded & (alpha < np.float32(0.5))))
    files, descs, texels = SC.frag_textures()
    want = tref.attributes(s["g"], rec, w, h, s["draws"], s["meshlets"], s["data"], s["vertices"], s["materials"], descs, texels, taps=True)
    assert not (want["flags"] & TR.NOT_SAMPLED).any()
    _zero("textured, gbuffer0", want["gbuffer0"] == f["fragtex_gbuffer0"])
    _zero("textured, gbuffer1", want["gbuffer1"] == f["fragtex_gbuffer1"])
    mi = want["attributes"]["materialIndex"]
    alpha = s["materials"]["diffuseFactor"][mi, 3] * np.where(s["materials"]["albedoTexture"][mi] > 0, want["taps"][:, 0, 3], np.float32(1))
    _zero("textured, discard under POST 1", f["fragtex_discard"] == (shaded & (alpha < np.float32(0.5))))


def test_perturbed_pow_and_exp2_stay_inside_the_gpu_replays_conditions(sref, bref):
    """tests/test_shade_cpu.py's experiment on the fixtures' inputs: every pow / non-integer exp2 result of the fp32 restatement moved by 2 ULP
    (up, down, a fixed mix) stays within one code of the fixture's expectation, with at least 90 % of the channels equal (99 % of pass 0's UFLOAT
    codes, tests/test_bloom_cpu.py's condition): the two conditions of the GPU replays' comparisons."""
    try:
        for path in FILES:
            f = np.load(path)
            x, y = np.meshgrid(np.arange(f["depth"].shape[1]), np.arange(f["depth"].shape[0]))
            owned = [(~(y ^ cb) & 1) == (x & 1) for cb in (0, 1)]  # the GPU replay compares the texels a fill owns
            for mode in (1, 2, 3):
                sref.perturb(mode, 2), bref.perturb(mode, 2)
                got = dict(extract=BR.codes(bref.extract(f["bloom_g0"])))
                for k in (0, 1):
                    shadow = f["shadow"] if k else None
                    got["fill%d" % k] = sref.shadow_fill(f["shadow"], f["depth"], k)[owned[k]]
                    got["blur%d" % k] = sref.shadow_blur(f["shadow"], f["depth"], k, float(f["znear"]))
                    got["final%d" % k] = SR.channels(sref.shade_final(_sd(f, k), f["gbuffer0"], f["gbuffer1"], f["depth"], shadow))
                    got["finalbloom%d" % k] = SR.channels(bref.shade_final_bloom(_sd(f, k), f["gbuffer0"], f["gbuffer1"], f["depth"], shadow, f["bloom0"]))
                sref.perturb(0), bref.perturb(0)
                for k, v in got.items():
                    want = BR.codes(f["extract_words"]) if k == "extract" else SR.channels(f[k + "_words"]) if k.startswith("final") else f[k + "_words"][owned[int(k[-1])]] if k.startswith("fill") else f[k + "_words"]
                    d = np.abs(v.astype(np.int64) - want.astype(np.int64))
                    print("%s mode %d %s: %d of %d differ, largest %d" % (os.path.basename(path), mode, k, int((d != 0).sum()), d.size, int(d.max())))
                    assert d.max() <= 1, (path, mode, k)
                    assert (d == 0).mean() >= (0.99 if k == "extract" else 0.9), (path, mode, k, float((d == 0).mean()))
    finally:
        sref.perturb(0), bref.perturb(0)
