"""The persistent per-pixel kernels on the MI355X where the rest of the suite does not reach (cases from
tests/pixel_cases.py, their coverage conditions in tests/test_pixel_passes_cpu.py):

1. the second trip of `for (i = first; i < n; i += stride)`: images of a little more than numCUs * 8 * 256 work items, ending in a ragged wave,
   through nv_visibility_resolve, nv_visibility_attributes, nv_shade_final, nv_shade_final_bloom, nv_shadow_fill, nv_bloom_extract,
   nv_depth_merge and nv_visibility_merge;
2. the run detection of nv_visibility_attributes and nv_visibility_resolve on hand-made images: a run start on every lane, on the DPP row
   edges, between keys one word apart, across waves and into a ragged last wave;
3. the degenerate branch and non-finite vertex, draw and material fields through nv_visibility_attributes.

Every comparison is the one the entry point's own test file uses, against the same restatement on the same bytes.  Outputs are poisoned
(0x5A) before every launch and, where the entry point's helpers carry one, followed by a tail that must keep its bytes."""
import numpy as np
import pytest

import bloom_ref as BR
import pixel_cases as PC
import shade_ref as SR
import test_bloom_gpu as TB
import test_depth_merge_gpu as TD
import test_shade_gpu as TS
import test_visattr_gpu as TA
import test_visbuffer_gpu as TV
import visattr_ref as VA
import visbuffer_ref as VB
from niagara_amd import host
from niagara_amd import layouts as L

POISON = 0x5A
POISON32 = 0x5A5A5A5A


@pytest.fixture(scope="module")
def vref(tmp_path_factory):
    return VB.load(tmp_path_factory.mktemp("visbuffer_ref_pixel_gpu"))


@pytest.fixture(scope="module")
def aref(tmp_path_factory):
    return VA.load(tmp_path_factory.mktemp("visattr_ref_pixel_gpu"))


@pytest.fixture(scope="module")
def sref(tmp_path_factory):
    return SR.load(tmp_path_factory.mktemp("shade_ref_pixel_gpu"))


@pytest.fixture(scope="module")
def bref(tmp_path_factory):
    return BR.load(tmp_path_factory.mktemp("bloom_ref_pixel_gpu"))


@pytest.fixture(scope="module")
def ctx():
    from niagara_amd import pipeline as P
    c = P.Context()
    yield c
    c.close()


def _cus(ctx):
    """the compute units persistent_grid(ctx, 8) multiplies by 8 (niagara_amd/csrc/context.hip reads the same property; pixel_cases.trip_items)"""
    import torch
    return torch.cuda.get_device_properties(ctx.device).multi_processor_count


def _trips(name, differs, written, g):
    """differs / written: per work item.  Says which trip a difference is in, and requires that the later trips wrote something"""
    differs, written = np.asarray(differs, bool).reshape(-1), np.asarray(written, bool).reshape(-1)
    print("%s: %d of %d items differ from the reference in the first trip, %d of %d in the later ones" %
          (name, int(differs[:g].sum()), g, int(differs[g:].sum()), len(differs) - g))
    assert len(written) > g and written[g:].any(), "nothing of the second trip was written"


# ---- 1. the second trip

_SHARED = {}


def _shared(key, make):
    if key not in _SHARED:
        _SHARED[key] = make()
    return _SHARED[key]


def _resolve(ctx, s, cd, words, w, h, seen_words):
    """one launch of nv_visibility_resolve over the scene's draws and meshes into poisoned records and cleared counters: TV._resolved's host copies"""
    import torch
    from niagara_amd import pipeline as P
    dev, draws, meshes = ctx.device, s["draws"], s["meshes"]
    out = dict(records=torch.full((w * h * 16,), POISON, dtype=torch.uint8, device=dev), meshlet_seen=torch.zeros(seen_words, dtype=torch.int32, device=dev),
               draw_pixels=torch.zeros(len(draws), dtype=torch.int32, device=dev), totals=torch.zeros(4, dtype=torch.int64, device=dev))
    ctx.visibility_resolve(cd, torch.from_numpy(words.view(np.int64)).to(dev), w, h, P.to_device(draws, dev), len(draws), P.to_device(meshes, dev), len(meshes),
                           out["records"], out["meshlet_seen"], out["draw_pixels"], out["totals"])
    ctx.status()
    return TV._resolved(out)


@pytest.mark.gpu
def test_resolve_takes_its_second_trip(ctx, vref):
    cus = _cus(ctx)
    w, h, n = PC.second_trip_sizes(cus)["pixel"]
    g = PC.check_second_trip(n, w, h, cus)
    s = PC.lod_scene()
    draws, meshes = s["draws"], s["meshes"]
    words = PC.resolve_words(draws, n)
    for lod in (1, 0):
        cd = s["cull"].copy()
        cd["lodEnabled"] = lod
        want = vref.resolve(cd, words, draws, meshes, s["mvb_words"])
        got = _resolve(ctx, s, cd, words, w, h, len(want["seen"]))
        raw = got["records"].view(np.uint32).reshape(n, 4)
        _trips("resolve, lodEnabled %d" % lod, (raw != want["records"].view(np.uint32).reshape(n, 4)).any(axis=1), (raw != POISON32).any(axis=1), g)
        TV._same_resolve(got, want, len(draws))
        assert 0 < want["totals"][1] < want["totals"][0]


def _attributes(ctx, s, records, w, h):
    """one launch of nv_visibility_attributes over exactly-sized device buffers into poisoned outputs: the host copies of TA._host"""
    import torch
    from niagara_amd import pipeline as P
    dev, n = ctx.device, w * h
    out = dict(attributes=torch.full((n * 64,), POISON, dtype=torch.uint8, device=dev), gbuffer0=torch.full((n,), POISON32, dtype=torch.int32, device=dev),
               gbuffer1=torch.full((n,), POISON32, dtype=torch.int32, device=dev), totals=torch.zeros(4, dtype=torch.int64, device=dev))
    t = [P.to_device(s[k], dev) for k in ("draws", "meshlets", "data", "vertices", "materials")]
    ctx.visibility_attributes(s["g"], P.to_device(records, dev), w, h, t[0], len(s["draws"]), t[1], len(s["meshlets"]), t[2], len(s["data"]), t[3],
                              len(s["vertices"]), t[4], len(s["materials"]), out["attributes"], out["gbuffer0"], out["gbuffer1"], out["totals"])
    ctx.status()
    return TA._host(out)


def _reference(aref, s, records, w, h):
    return aref.attributes(s["g"], records, w, h, s["draws"], s["meshlets"], s["data"], s["vertices"], s["materials"])


@pytest.mark.gpu
def test_attributes_take_their_second_trip(ctx, aref):
    cus = _cus(ctx)
    w, h, n = PC.second_trip_sizes(cus)["pixel"]
    g = PC.check_second_trip(n, w, h, cus)
    s = PC.attr_scene((w, h))
    records = PC.random_records(s, n, 3)
    want = _reference(aref, s, records, w, h)
    got = _attributes(ctx, s, records, w, h)
    a, b = got["attributes"].view(np.uint32).reshape(n, 16), want["attributes"].view(np.uint32).reshape(n, 16)
    differs = (a != b).any(axis=1) | (got["gbuffer1"] != want["gbuffer1"])
    written = (a != POISON32).any(axis=1) & (got["gbuffer0"] != POISON32) & (got["gbuffer1"] != POISON32)
    _trips("attributes", differs, written, g)
    TA._same_attributes(got, want)
    shaded = (want["flags"] & VA.SHADED) != 0
    assert shaded[g:].any() and (~shaded[g:]).any() and want["totals"][0] == shaded.sum() > shaded[:g].sum() and want["totals"][3] > 0


def _shade_inputs(w, h):
    return _shared(("shade", w, h), lambda: SR.test_inputs(w, h))


@pytest.mark.gpu
@pytest.mark.parametrize("shadows", [0, 1])
def test_shade_final_takes_its_second_trip(shadows, ctx, sref):
    cus = _cus(ctx)
    w, h, n = PC.second_trip_sizes(cus)["pixel"]
    g = PC.check_second_trip(n, w, h, cus)
    i, sd = _shade_inputs(w, h), SR.test_shade_data(w, h, shadows)
    want = sref.shade_final(sd, i["gbuffer0"], i["gbuffer1"], i["depth"], i["shadow"] if shadows else None)
    g0, g1, depth, out = TS._dev(ctx, i["gbuffer0"]), TS._dev(ctx, i["gbuffer1"]), TS._dev(ctx, i["depth"]), TS._out(ctx, n * 4)
    shadow = TS._dev(ctx, i["shadow"]) if shadows else None
    ctx.shade_final(sd, g0, g1, depth, shadow, out, w, h)
    ctx.status()
    got = TS._host(out, n * 4, np.uint32, (h, w))
    _trips("final, shadows %d" % shadows, got != want, got != POISON32, g)
    TS._close("final %dx%d shadows %d" % (w, h, shadows), SR.channels(got), SR.channels(want), alpha=True)


@pytest.mark.gpu
@pytest.mark.parametrize("shadows", [0, 1])
def test_shade_final_bloom_takes_its_second_trip(shadows, ctx, bref):
    cus = _cus(ctx)
    w, h, n = PC.second_trip_sizes(cus)["pixel"]
    g = PC.check_second_trip(n, w, h, cus)
    d, desc = BR.desc(w, h), host.bloom_desc(w, h)
    i, sd = _shade_inputs(w, h), SR.test_shade_data(w, h, shadows)
    words = TB._poison_words(d)
    b0 = TB.bloom0_input(w, h)  # bloom_ref.test_levels' level 0 of this size
    assert b0.shape == (d["sizes"][0][1], d["sizes"][0][0])
    words[:b0.size] = b0.reshape(-1)
    want = bref.shade_final_bloom(sd, i["gbuffer0"], i["gbuffer1"], i["depth"], i["shadow"] if shadows else None, b0)
    g0, g1, depth, out, bloom = TB._dev(ctx, i["gbuffer0"]), TB._dev(ctx, i["gbuffer1"]), TB._dev(ctx, i["depth"]), TB._out(ctx, n * 4), TB._dev(ctx, words)
    shadow = TB._dev(ctx, i["shadow"]) if shadows else None
    ctx.shade_final_bloom(sd, g0, g1, depth, shadow, out, w, h, bloom, desc)
    ctx.status()
    got = TB._host(out, n * 4).reshape(h, w)
    _trips("final with bloom, shadows %d" % shadows, got != want, got != POISON32, g)
    TB._close8("final with bloom %dx%d shadows %d" % (w, h, shadows), got, want)
    assert bloom.cpu().numpy().tobytes() == words.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("checkerboard", [0, 1])
def test_shadow_fill_takes_its_second_trip(checkerboard, ctx, sref):
    cus = _cus(ctx)
    w, h, n = PC.second_trip_sizes(cus)["fill"]
    g = PC.check_second_trip(n, w, h, cus)
    assert w % 2 == 1 and n == (w + 1) // 2 * h
    i = _shared(("fill", w, h), lambda: SR.test_inputs(w, h))
    want = sref.shadow_fill(i["shadow"], i["depth"], checkerboard)
    shadow, depth = TS._dev(ctx, i["shadow"], TS.TAIL), TS._dev(ctx, i["depth"])
    ctx.shadow_fill(shadow, depth, w, h, checkerboard)
    ctx.status()
    got = TS._host(shadow, w * h, np.uint8, (h, w))
    # work item (gy, gx) owns the texel x = 2 gx + (~(gy ^ checkerboard) & 1) of row gy; past the odd width its store is dropped
    gy, gx = np.divmod(np.arange(n), (w + 1) // 2)
    px = 2 * gx + (~(gy ^ checkerboard) & 1)
    inside = px < w
    assert (~inside[g:]).any()  # the second trip meets the dropped store
    px = np.minimum(px, w - 1)
    _trips("fill, checkerboard %d" % checkerboard, inside & (got[gy, px] != want[gy, px]), inside & (got[gy, px] != i["shadow"][gy, px]), g)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    owned = (~(y ^ checkerboard) & 1) == (x & 1)
    assert (got[~owned] == i["shadow"][~owned]).all() and (want[~owned] == i["shadow"][~owned]).all()
    TS._close("fill %dx%d cb %d" % (w, h, checkerboard), got[owned], want[owned])


@pytest.mark.gpu
def test_bloom_extract_takes_its_second_trip(ctx, bref):
    cus = _cus(ctx)
    w, h, n = PC.second_trip_sizes(cus)["extract"]
    g = PC.check_second_trip(n, w, h, cus)
    d, desc = BR.desc(w, h), host.bloom_desc(w, h)
    n0 = d["sizes"][0][0] * d["sizes"][0][1]
    assert n0 == n and d["sizes"][0][0] <= 16384
    g0 = BR.test_gbuffer0(w, h)
    want = bref.extract(g0)
    src, out = TB._dev(ctx, g0), TB._out(ctx, d["total"] * 4)
    ctx.bloom_extract(src, w, h, out, desc)
    ctx.status()
    got = TB._host(out, d["total"] * 4)
    assert (got[n0:] == POISON32).all()  # the other levels keep their bytes
    _trips("extract", got[:n0] != want.reshape(-1), got[:n0] != POISON32, g)
    TB._adjacent("extract %dx%d" % (w, h), got[:n0].reshape(want.shape), want)
    assert src.cpu().numpy().tobytes() == g0.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("sources,offset", [(2, 0), (8, 0), (2, 1)])
def test_depth_merge_takes_its_second_trip(sources, offset, ctx):
    """aligned: one item per 16-byte group and the last three texels through the scalar tail, a.n4 * 4u + first; 4 bytes off the grid: the scalar
    loop, one item per texel"""
    cus = _cus(ctx)
    if offset:
        w, h, items = PC.second_trip_sizes(cus)["pixel"]
        per = 1
    else:
        w, h, items = PC.second_trip_sizes(cus)["depth_aligned"]
        per = 4
        assert items == w * h // 4 and w * h % 4 == 3
    g = PC.check_second_trip(items, w, h, cus)
    rng = np.random.default_rng(40 + sources + offset)
    dst = TD._bits(rng, w * h, True)
    srcs = [TD._bits(rng, w * h, True) for _ in range(sources)]
    # the ends: the last three texels (the aligned forms' scalar tail) and the first one lie strictly below one source each, a different source per
    # texel, so a texel the kernel does not visit keeps a word that is not the maximum
    ends = np.array([0, w * h - 3, w * h - 2, w * h - 1])
    for j, at in enumerate(ends):
        dst[at] = 0x00000100 + j
        for k, src in enumerate(srcs):
            src[at] = 0x3F000000 + 16 * j + k if k == (j + sources - 1) % sources else 0x00000010 + k
    want = np.maximum.reduce([dst] + srcs)
    assert (want[ends] != dst[ends]).all() and len(set(want[ends].tolist())) == len(ends)
    got, intact = TD._merge(ctx, dst, srcs, w, h, offset=offset)
    _trips("depth merge, %d sources, offset %d" % (sources, offset), got != want, got != dst, g * per)
    print("depth merge: the ends", got[ends].tolist(), want[ends].tolist())
    assert got[ends].tolist() == want[ends].tolist()
    assert intact and got.tobytes() == want.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("sources,skew", [(2, 0), (8, 0), (2, 1)])
def test_visibility_merge_takes_its_second_trip(sources, skew, ctx):
    """aligned: one item per pair of words and the odd last word through the scalar tail; 8-byte skew: the scalar loop, one item per word"""
    import torch
    cus = _cus(ctx)
    if skew:
        w, h, items = PC.second_trip_sizes(cus)["pixel"]
        per = 1
    else:
        w, h, items = PC.second_trip_sizes(cus)["vis_aligned"]
        per = 2
        assert items == w * h // 2 and w * h % 2 == 1
    g = PC.check_second_trip(items, w, h, cus)
    n = w * h
    rng = np.random.default_rng(50 + sources + skew)
    bufs = rng.integers(0, 1 << 63, (sources + 1, n + 1), dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, (sources + 1, n + 1), dtype=np.uint64)
    bufs[:, ::5] = 0
    bufs[1, 3] = np.uint64(VB.encode(0x3F800000, 7, 7))  # bit 63 set
    assert (bufs >> np.uint64(63)).any()
    # the ends of the view: the last word (the aligned forms' scalar tail), the one before it and the first lie strictly below one source each
    ends = np.array([0, n - 2, n - 1])
    for j, at in enumerate(ends):
        bufs[0, skew + at] = 100 + j
        for k in range(1, sources + 1):
            bufs[k, skew + at] = np.uint64(VB.encode(0x3F000000 + j, 11 + k, 5)) if k == 1 + (j + sources - 1) % sources else np.uint64(10 + k)
    t = [torch.from_numpy(b.view(np.int64)).to(ctx.device) for b in bufs]
    views = [x[skew:skew + n] for x in t]
    assert all(v.data_ptr() % 16 == 8 * skew for v in views)
    want = np.maximum.reduce([b[skew:skew + n] for b in bufs])
    assert (want[ends] != bufs[0][skew:skew + n][ends]).all()
    ctx.visibility_merge(views[0], views[1:], w, h)
    ctx.status()
    whole = t[0].cpu().numpy().view(np.uint64)
    got = whole[skew:skew + n]
    _trips("visibility merge, %d sources, skew %d" % (sources, skew), got != want, got != bufs[0][skew:skew + n], g * per)
    print("visibility merge: the ends", got[ends].tolist(), want[ends].tolist())
    assert got[ends].tolist() == want[ends].tolist()
    assert got.tobytes() == want.tobytes()
    assert whole[:skew].tobytes() == bufs[0][:skew].tobytes() and whole[skew + n:].tobytes() == bufs[0][skew + n:].tobytes()  # the words around the view
    for k in range(1, sources + 1):  # the sources are left alone
        assert t[k].cpu().numpy().view(np.uint64).tobytes() == bufs[k].tobytes()


# ---- 2. run edges

@pytest.mark.gpu
@pytest.mark.parametrize("group", ["a", "b", "c", "d", "e"])
def test_attribute_runs_start_where_the_keys_change(group, ctx, aref):
    """tests/test_pixel_passes_cpu.py states what the images cover together: a run start on every lane, on lanes 16, 32 and 48 after a key one
    word apart (each word) and with key (0, 0, 0)"""
    images = PC.run_edge_cases(PC.attr_scene((64, 12)))[group]
    for im in images:
        w, h = im["width"], im["height"]
        s = PC.attr_scene((w, h))
        want = _reference(aref, s, im["records"], w, h)
        lane, start, diff, named, key = PC.run_starts(im)
        assert (start & named & (lane != 0)).any() or group == "d", im["name"]  # the image has run starts inside a wave
        assert want["totals"][0] > 0 and (want["totals"][1] > 0) == im["invalid"], im["name"]
        got = _attributes(ctx, s, im["records"], w, h)
        print(im["name"], "totals", got["totals"].tolist(), want["totals"].tolist())
        TA._same_attributes(got, want)


@pytest.mark.gpu
def test_resolve_runs_start_where_the_cluster_changes(ctx, vref):
    """(c)'s boundaries on mvi with mvi 0 behind another cluster and behind an empty word, and runs whose first lane is unresolved (triangle >=
    96) while the lanes behind it are resolved: that lane adds to d_drawPixels and ORs into d_meshletSeen for pixels that are not its own"""
    s = PC.lod_scene()
    draws, meshes = s["draws"], s["meshes"]
    for name, (words, w, h) in PC.resolve_edge_words(s).items():
        for lod in (1, 0):
            cd = s["cull"].copy()
            cd["lodEnabled"] = lod
            want = vref.resolve(cd, words, draws, meshes, s["mvb_words"])
            assert want["totals"][0] > want["totals"][1] and want["draw_pixels"].sum() == want["totals"][0] - want["totals"][1] and want["seen"].any()
            assert (want["totals"][1] > 0) == (name == "unresolved first lane")
            got = _resolve(ctx, s, cd, words, w, h, len(want["seen"]))
            print(name, "lodEnabled", lod, "totals", got["totals"].tolist(), want["totals"].tolist())
            TV._same_resolve(got, want, len(draws))
            assert got["draw_pixels"].tolist() == want["draw_pixels"].tolist()


# ---- 3. the degenerate branch and special values

@pytest.mark.gpu
def test_degenerate_triangles_and_special_values_through_the_attribute_pass(ctx, aref):
    """where the restatement's attribute word is a NaN the device's is a NaN (sign and payload are not compared: the two
    sides' arithmetic units choose them differently); every other word of the record and every gbuffer1 word is bit-identical; gbuffer0 by the
    rule of the entry point's own tests.  totals[2] > 0: the degenerate branch runs on the device"""
    s = PC.special_scene()
    w, h = s["viewport"]
    n = w * h
    want = _reference(aref, s, s["records"], w, h)
    assert want["totals"][2] > 0 and want["totals"][3] > 0 and want["totals"][1] == 0 and want["totals"][0] == n
    got = _attributes(ctx, s, s["records"], w, h)
    print("special values: totals", got["totals"].tolist(), want["totals"].tolist())
    assert got["totals"].tolist() == want["totals"].tolist()
    a, b = got["attributes"].view(np.uint32).reshape(n, 16).copy(), want["attributes"].view(np.uint32).reshape(n, 16).copy()
    is_float = np.ones(16, bool)
    is_float[[L.PIXELATTR.fields["drawId"][1] // 4, L.PIXELATTR.fields["materialIndex"][1] // 4]] = False
    nan_want = np.isnan(b.view(np.float32)) & is_float
    nan_got = np.isnan(a.view(np.float32)) & is_float
    print("special values: %d NaN words in the reference, %d on the device" % (int(nan_want.sum()), int(nan_got.sum())))
    assert nan_want.any() and (nan_got == nan_want).all()
    a[nan_want], b[nan_want] = 0, 0
    bad = np.nonzero((a != b).any(axis=1))[0]
    print("special values: records differ at %d pixels; first:" % len(bad), [(int(i), np.nonzero(a[i] != b[i])[0].tolist()) for i in bad[:12]])
    assert len(bad) == 0
    assert got["gbuffer1"].tobytes() == want["gbuffer1"].tobytes()
    mat = s["draws"]["materialIndex"][s["records"]["drawId"]]
    ordinary = np.isin(mat, PC.ORDINARY_MATERIALS)
    c, r = TA._channels(got["gbuffer0"], (8, 8, 8, 8)), TA._channels(want["gbuffer0"], (8, 8, 8, 8))
    print("special values: gbuffer0: %d channels, %d differ, largest difference %d" % (c.size, int((c != r).sum()), int(np.abs(c - r).max())))
    assert (c[~ordinary] == r[~ordinary]).all() and np.isin(c[~ordinary], (0, 255)).all()  # special factors: exact codes
    assert np.abs(c - r).max() <= 1 and (c == r).mean() >= 0.9
