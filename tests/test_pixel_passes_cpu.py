"""The cases of tests/test_pixel_passes_gpu.py on the CPU (tests/pixel_cases.py): the conditions under which a green GPU run says something.
The second-trip sizes are what DESIGN.md §4.12 states at 256 compute units; the run-edge images start a run on every lane, on the DPP row
edges with every single-word difference and with key (0, 0, 0); the special-value scene takes both causes of the degenerate branch, writes
NaN words, and its ordinary material factors sit away from the rounding boundaries of the G-buffer codes.  No GPU."""
import numpy as np
import pytest

import pixel_cases as PC
import visattr_ref as VA
import visbuffer_ref as VB


@pytest.fixture(scope="module")
def vref(tmp_path_factory):
    return VB.load(tmp_path_factory.mktemp("visbuffer_ref_pixel_cpu"))


@pytest.fixture(scope="module")
def aref(tmp_path_factory):
    return VA.load(tmp_path_factory.mktemp("visattr_ref_pixel_cpu"))


# ---- 1. the second trip

def test_second_trip_sizes_at_256_compute_units():
    g = PC.trip_items(256)
    assert g == 524288
    sizes = PC.second_trip_sizes(256)
    assert sizes["pixel"] == (2051, 257, 527107) and 527107 - g == 2819 == 44 * 64 + 3
    assert sizes["fill"] == (2051, 514, 527364) and (2051 + 1) // 2 * 514 == 527364
    w, h, n4 = sizes["depth_aligned"]
    assert (w, h, n4) == (2051, 1029, 527619) and w * h % 4 == 3
    w, h, n2 = sizes["vis_aligned"]
    assert (w, h, n2) == (2051, 515, 528132) and w * h % 2 == 1
    w, h, n = sizes["extract"]
    assert ((w + 1) // 2, (h + 1) // 2, n) == (2051, 257, 527107)
    for cus in (1, 8, 64, 104, 128, 228, 256, 304, 320):  # every size passes its own condition unless cus % 64 == 63
        for name, (w, h, items) in PC.second_trip_sizes(cus).items():
            assert PC.check_second_trip(items, w, h, cus) == cus * 2048, (cus, name)
    with pytest.raises(AssertionError):
        PC.check_second_trip(320 * 192, 320, 192, 256)  # the frame scenes: no second trip
    with pytest.raises(AssertionError):
        PC.check_second_trip(g + 128, 2048, 257, 256)  # a whole last wave


def test_encode_words_is_visbuffer_refs_encode():
    rng = np.random.default_rng(1)
    z, m, t = rng.integers(0, 0x3F800001, 200), rng.integers(0, VB.MVI_END, 200), rng.integers(0, 128, 200)
    z[0], m[0], t[0] = 0x3F800000, VB.MVI_END - 1, 127
    assert PC.encode_words(z, m, t).tolist() == [VB.encode(int(a), int(b), int(c)) for a, b, c in zip(z, m, t)]


def test_second_trip_records_have_runs_of_one_to_nine_and_no_sample():
    s = PC.attr_scene((2051, 257))
    r = PC.random_records(s, 2051 * 257, 3)
    lane, start, diff, named, key = PC.run_starts(dict(records=r))
    edges = np.nonzero(diff != 0)[0]
    runs = np.diff(edges)
    assert runs.min() == 1 and 4.5 < runs.mean() < 5.6 and (runs[named[edges[:-1]]] <= 18).all()  # (equal neighbours merge now and then: 1 in 384)
    assert 0.05 < (~named).mean() < 0.15
    assert len(np.unique(key[named], axis=0)) == len(PC.all_valid_keys(s)) == 3 * 128


# ---- 2. run edges

def test_run_edge_cases_start_a_run_on_every_lane_and_row_edge():
    s = PC.attr_scene((64, 12))
    valid, invalid = PC.key_set(s)
    assert (0, 0, 0) in valid and 10 <= len(valid) <= 14 and len(invalid) == 2
    cases = PC.run_edge_cases(s)
    assert sorted(cases) == ["a", "b", "c", "d", "e"] and len(cases["e"]) == 4 and len(cases["d"]) == 6
    started = np.zeros(64, bool)
    single = {(lane, word): False for lane in PC.ROW_EDGES for word in (1, 2, 4)}
    zero = {lane: False for lane in PC.ROW_EDGES}
    is_valid = lambda k: np.isin(k.astype(np.int64) @ np.array([1 << 40, 1 << 20, 1]), [(d << 40) + (m << 20) + t for d, m, t in valid])
    for group, images in cases.items():
        for im in images:
            assert im["width"] == 64 or group in ("d", "e")
            assert len(im["records"]) == im["width"] * im["height"]
            lane, start, diff, named, key = PC.run_starts(im)
            ok = is_valid(key)
            both = np.zeros(len(key), bool)
            both[1:] = ok[1:] & ok[:-1]
            started[lane[start & named & (lane != 0)]] = True  # lane 0 starts one in every wave anyway
            started[0] = True
            for ln in PC.ROW_EDGES:
                at = lane == ln
                for word in (1, 2, 4):
                    single[ln, word] |= bool((at & both & (diff == word)).any())
                zero[ln] |= bool((at & start & (diff != 0) & (key == 0).all(axis=1)).any())
            if group == "a":
                assert (start & ok).all()  # every lane starts a run
            if group == "d":
                assert im["height"] == 1 and im["width"] in (321, 383) and not diff[:320].any() and not diff[322:].any()
    assert started.all(), np.nonzero(~started)[0]
    assert all(single.values()), single
    assert all(zero.values()), zero
    # (c) puts a boundary at every listed lane in every image, and (b) has the no-sample / (0, 0, 0) neighbours in both orders
    for im in cases["c"]:
        lane, start, diff, named, key = PC.run_starts(im)
        assert sorted(set(lane[diff != 0].tolist()) - {0}) == sorted(PC.BOUNDARIES)  # (lane 0: the next row's A after this row's B)
    lane, start, diff, named, key = PC.run_starts(cases["b"][0])
    zeros = (key == 0).all(axis=1)
    assert (zeros[1:] & ~named[:-1] & (diff[1:] == 1)).any() and (~named[1:] & zeros[:-1] & (diff[1:] == 1)).any()


def test_run_edge_cases_shade_and_count_their_invalid_keys(aref):
    textured_images = 0
    for group, images in PC.run_edge_cases(PC.attr_scene((64, 12))).items():
        for im in images:
            s = PC.attr_scene((im["width"], im["height"]))
            o = aref.attributes(s["g"], im["records"], im["width"], im["height"], s["draws"], s["meshlets"], s["data"], s["vertices"], s["materials"])
            assert o["totals"][0] > 0, im["name"]
            assert (o["totals"][1] > 0) == im["invalid"], im["name"]
            assert not (o["flags"] & VA.CLIPPED).any()  # the three draws are in front of the camera
            # draw 2 alone has the material that names textures: counted exactly where its keys are shaded
            assert o["totals"][3] == ((im["records"]["drawId"] == 2) & ((o["flags"] & VA.SHADED) != 0)).sum(), im["name"]
            textured_images += int(o["totals"][3] > 0)
    assert textured_images >= 10


def test_resolve_edge_words_have_the_runs_they_name(vref):
    s = PC.lod_scene()
    words = PC.resolve_edge_words(s)
    assert sorted(words) == ["boundary after an empty word", "boundary after another cluster", "unresolved first lane"]
    for name, (w, width, height) in words.items():
        assert width == 64 and len(w) == 64 * height
        for lod in (1, 0):
            cd = s["cull"].copy()
            cd["lodEnabled"] = lod
            r = vref.resolve(cd, w, s["draws"], s["meshes"], s["mvb_words"])["records"]
            resolved = r["drawId"] != PC.NONE
            mvi = ((w & np.uint64(VB.ID_MASK)).astype(np.int64) - 1) >> 7
            lane = np.arange(len(w)) % 64
            if name.startswith("boundary"):
                for b in PC.BOUNDARIES:  # mvi 0 starts a resolved run at every listed lane
                    row = PC.BOUNDARIES.index(b)
                    assert (mvi[row * 64 + b:row * 64 + 64] == 0).all() and resolved[row * 64 + b:row * 64 + 64].all() and mvi[row * 64 + b - 1] != 0
                assert resolved[lane == 0].all() == (name == "boundary after another cluster")
            else:
                head = np.ones(len(w), bool)
                head[1:] = mvi[1:] != mvi[:-1]
                unresolved = (r["drawId"] == PC.NONE) & (r["meshletIndex"] == PC.NONE)
                follows = np.zeros(len(w), bool)  # a resolved pixel of the same run and wave right behind an unresolved first one
                follows[1:] = head[:-1] & unresolved[:-1] & ~head[1:] & resolved[1:] & (lane[1:] != 0)
                assert follows.sum() > 20 and (unresolved[head & (lane != 0)]).all()


# ---- 3. the degenerate branch and special values

def _special(aref):
    s = PC.special_scene()
    w, h = s["viewport"]
    args = (s["g"], s["records"], w, h, s["draws"], s["meshlets"], s["data"], s["vertices"], s["materials"])
    return s, aref.attributes(*args), aref.attributes(*args, real="f64")


def test_special_scene_takes_both_causes_of_the_degenerate_branch(aref):
    """The two causes are told apart through the fp64 build of the same statements.  Three equal vertices give b0 = b1 = b2 = 0 exactly in any
    precision: sum == 0 in both builds.  The largest fp16 positions under a scale of 1e30 give clip coordinates near 1e35, whose products
    overflow fp32 (non-finite lambda, sum NaN or infinite: not 0) and stay finite in fp64, where the triangle is not degenerate"""
    s, o, o64 = _special(aref)
    r = s["records"]
    names = [n for n, _ in PC.SPECIAL_TRIANGLES]
    pair = lambda draw, tri: (r["drawId"] == PC.SPECIAL_DRAWS.index(draw)) & (r["triangle"] == names.index(tri))
    deg, deg64 = (o["flags"] & VA.DEGENERATE) != 0, (o64["flags"] & VA.DEGENERATE) != 0
    assert np.bincount(r["drawId"] * len(names) + r["triangle"], minlength=72).min() >= 7  # every pair meets several pixels
    equal = pair("ordinary", "three equal")
    assert equal.sum() >= 7 and deg[equal].all() and deg64[equal].all()
    overflow = pair("scale 1e30", "largest halves")
    assert overflow.sum() >= 7 and deg[overflow].all() and not deg64[overflow].any()
    assert o["totals"][2] == deg.sum() and o["totals"].tolist() == [len(r), 0, int(deg.sum()), int(((o["flags"] & VA.TEXTURED) != 0).sum())]
    assert o["totals"][3] > 0
    plain = pair("ordinary", "ordinary") | pair("ordinary, rotated", "ordinary")
    assert not deg[plain].any() and np.isfinite(o["vals"][plain]).all() and not (o["flags"][plain] & VA.CLIPPED).any()
    assert (~deg).sum() > len(r) // 4  # valid non-degenerate pixels
    for tri in ("in the camera plane", "behind the camera"):
        assert ((o["flags"][pair("ordinary", tri)] & VA.CLIPPED) != 0).all()
    # a degenerate pixel takes its first corner: lambda = (1, 0, 0)
    assert (o["bary"][deg] == 0).all()
    # NaN output words, and finite words next to them
    nan = np.isnan(o["vals"])
    assert nan.any() and 0.02 < nan.mean() < 0.9
    assert nan[deg].any() and nan[~deg].any()


def test_special_materials_give_exact_codes_and_ordinary_ones_stay_off_the_boundaries(aref):
    s, o, o64 = _special(aref)
    mat = s["draws"]["materialIndex"][s["records"]["drawId"]]
    ordinary = np.isin(mat, PC.ORDINARY_MATERIALS)
    c, c64 = o["chan"], o64["chan"]
    # 1 + emissivef is 0 under material 4 (log2 = -inf) and negative under material 5 (NaN)
    assert np.isneginf(c[mat == 4, 3]).all() and np.isnan(c[mat == 5, 3]).all() and (mat == 4).any() and (mat == 5).any()
    # special factors: every gbuffer0 channel is 0 or 255, by the same route in both builds (NaN, an infinity or a value outside [0, 1])
    codes = lambda g: np.stack([(g >> np.uint32(8 * k)) & np.uint32(255) for k in range(4)], -1).astype(np.int64)
    g, g64 = codes(o["gbuffer0"]), codes(o64["gbuffer0"])
    assert np.isin(g[~ordinary], (0, 255)).all() and (g[~ordinary] == g64[~ordinary]).all()
    for k in range(4):
        v = c64[~ordinary, k]
        assert (np.isnan(v) | (v <= 0.0) | (v >= 1.0)).all()
    assert set(np.unique(g[~ordinary]).tolist()) == {0, 255}
    # ordinary factors: 255 * value of the fp64 build lies at least 0.01 code from a rounding boundary, so an error of a few ULP of fp32 in
    # pow or log2 on either side cannot change the code; the restatement alone is then equal to its fp64 build at every channel
    v = 255.0 * c64[ordinary, :4]
    assert ordinary.any() and np.isfinite(v).all()
    frac = np.abs(v - np.floor(v) - 0.5)
    assert frac.min() >= 0.01, frac.min()
    assert (g[ordinary] == g64[ordinary]).all()
    assert (g == g64).mean() >= 0.9
    # specular.w -1, 2 and NaN: codes 0, 1023 and 0
    sw = (o["gbuffer1"] >> np.uint32(20)) & np.uint32(1023)
    assert (sw[mat == 2] == 0).all() and (sw[mat == 3] == 1023).all() and (sw[mat == 4] == 0).all()
