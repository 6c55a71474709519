"""The visibility buffer of the indexed draws on the MI355X: nv_rasterdepth_indexed_visibility and
nv_visibility_resolve_indexed bit-identical to their CPU restatement (tests/visindexed_ref.c) — commands whose triangle numbers cross chunk
ends, the lane path and the LDS queue, both faces, the near-plane clip, every skip rule of §4.11, ties, a span too small, sliced offsets —
with depth and totals equal to nv_rasterdepth_indexed's; the resolve on hand-made words of every class, on its second grid trip and on runs
that start on every lane that matters; the argument checks; and the chain replayed from a captured graph."""
import numpy as np
import pytest

import oracle
import pixel_cases as PC
import raster_ref as RR
import test_visindexed_cpu as TC
import visindexed_ref as VI
from niagara_amd import host, synth
from niagara_amd import layouts as L

INT_MAX = 2 ** 31 - 1
SIZES = TC.SIZES


@pytest.fixture(scope="session")
def viref(tmp_path_factory):
    return VI.load(tmp_path_factory.mktemp("visindexed_ref_gpu"))


@pytest.fixture(scope="session")
def iaref(tmp_path_factory):
    import visattr_indexed_ref as VAI
    return VAI.load(tmp_path_factory.mktemp("visattr_indexed_ref_gpu"))


@pytest.fixture(scope="session")
def sref(tmp_path_factory):
    import shade_ref as SR
    return SR.load(tmp_path_factory.mktemp("shade_ref_vi"))


@pytest.fixture(scope="module")
def ctx():
    from niagara_amd import pipeline as P
    c = P.Context()
    yield c
    c.close()


def _dev(a, dev, empty_bytes):
    import torch
    from niagara_amd import pipeline as P
    return P.to_device(a, dev) if len(a) else torch.zeros(empty_bytes, dtype=torch.uint8, device=dev)


def _raster(ctx, g, commands, count, draws, indices, vertices, w, h, offsets, limit=None, near_clip=0, depth=None, vis=None, draw_count=None,
            index_capacity=None, vertex_capacity=None):
    """nv_rasterdepth_indexed_visibility: (depth, visibility, totals); nv_rasterdepth_indexed over the same input must leave the same depth
    and totals"""
    import torch
    from niagara_amd import pipeline as P
    dev = ctx.device
    ctx.set_option(P.NV_OPT_RASTER_NEAR_CLIP, near_clip)
    if limit is not None:
        ctx.set_option(P.NV_OPT_RASTER_SMALL_LIMIT, limit)
    try:
        dcb = _dev(np.ascontiguousarray(commands, L.DRAWCMD), dev, 24)
        dccb = P.to_device(np.array([count, 0, 0, 0], np.uint32), dev)
        db, ib, vb = _dev(draws, dev, 48), _dev(np.ascontiguousarray(indices, np.uint32), dev, 4), _dev(vertices, dev, 16)
        ob = P.to_device(np.ascontiguousarray(offsets, np.uint64), dev)
        n = len(draws) if draw_count is None else draw_count
        caps = (len(indices) if index_capacity is None else index_capacity, len(vertices) if vertex_capacity is None else vertex_capacity)
        out = []
        for with_vis in (True, False):
            d = torch.zeros((h, w), dtype=torch.float32, device=dev) if depth is None else torch.from_numpy(np.ascontiguousarray(depth)).to(dev)
            v = (torch.zeros((h, w), dtype=torch.int64, device=dev) if vis is None
                 else torch.from_numpy(np.ascontiguousarray(vis).view(np.int64)).to(dev))
            tot = torch.zeros(4, dtype=torch.int64, device=dev)
            if with_vis:
                ctx.rasterdepth_indexed_visibility(g, dcb, dccb, db, n, ib, caps[0], vb, caps[1], d, w, h, ob, v, tot)
            else:
                ctx.rasterdepth_indexed(g, dcb, dccb, db, n, ib, caps[0], vb, caps[1], d, w, h, tot)
            ctx.status()
            out.append((d.cpu().numpy(), v.cpu().numpy().view(np.uint64), tot.cpu().numpy().view(np.uint64)))
        assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][2].tolist() == out[1][2].tolist()  # the depth-only entry point's bits
        return out[0]
    finally:
        ctx.set_option(P.NV_OPT_RASTER_SMALL_LIMIT, 16)
        ctx.set_option(P.NV_OPT_RASTER_NEAR_CLIP, 0)


def _same(gpu, ref):
    assert gpu[2].tolist() == ref[2].tolist()
    assert gpu[0].view(np.uint32).tobytes() == ref[0].view(np.uint32).tobytes()
    assert gpu[1].tobytes() == ref[1].tobytes()


def _ix(s):
    return s["commands"], s["count"], s["draws"], s["indices"], s["vertices"]


# ---- 1. the raster

@pytest.mark.gpu
@pytest.mark.parametrize("post_pass", [0, 1])
@pytest.mark.parametrize("limit", [0, 16, INT_MAX])
def test_raster_equals_the_restatement(limit, post_pass, ctx, viref):
    """commands of 1, 63, 64, 65 and 200 triangles (a command's t crosses chunk ends, a wave starts in the middle of a command) at 64 x 48,
    every triangle through the lane path (INT_MAX), through the LDS queue (0) and split between them (16)"""
    s = TC._soup(21)
    w, h = s["viewport"]
    g = RR.globals_for(s["cull"], (w, h), post_pass)
    ref = viref.raster(g, *_ix(s), w, h, s["offsets"])
    assert ref[2][1] == sum(SIZES) and (ref[1] != 0).sum() > 400
    _same(_raster(ctx, g, *_ix(s), w, h, s["offsets"], limit=limit), ref)


def _perturb(s):
    """every skip rule of §4.11 on a soup of nine commands: instanceCount 0 and 5, a drawId past drawCount, remainder indices, a wrapping
    vertexOffset, a 0xFFFFFFFF index, a last range that runs past the index buffer, and a count above drawCount"""
    c, ind = s["commands"].copy(), s["indices"].copy()
    n = len(c)
    c[1]["instanceCount"] = 0
    c[2]["drawId"] = n + 3
    c[3]["instanceCount"] = 5
    c[4]["indexCount"] += 2
    f, k = int(c[5]["firstIndex"]), int(c[5]["indexCount"])
    c[5]["vertexOffset"] = 2 ** 32 - 7
    ind[f:f + k] += np.uint32(7)
    ind[int(c[6]["firstIndex"]) + 4] = 0xFFFFFFFF
    c[n - 1]["indexCount"] += 30
    return dict(s, commands=c, indices=ind, count=n + 9)


@pytest.mark.gpu
@pytest.mark.parametrize("limit", [0, 16, INT_MAX])
def test_raster_skip_rules(limit, ctx, viref):
    s = VI.triangle_soup([40, 1, 63, 64, 65, 70, 66, 5, 130], 22)
    w, h = 64, 48
    g = RR.globals_for(host.build_cull_data(viewport=(w, h)), (w, h), 1)
    p = _perturb(s)
    ref = viref.raster(g, *_ix(p), w, h, p["offsets"])
    assert ref[2][0] == 7 and 0 < ref[2][2] < sum([40, 64, 65, 70, 66, 5, 130]) + 1
    _same(_raster(ctx, g, *_ix(p), w, h, p["offsets"], limit=limit), ref)
    # a target and a depth that are loaded, not cleared; capacities that cut the buffers short
    rng = np.random.default_rng(3)
    depth = rng.uniform(0, 0.02, (h, w)).astype(np.float32)
    vis = (depth.view(np.uint32).astype(np.uint64) << np.uint64(34)) | np.uint64(5)
    kw = dict(index_capacity=len(p["indices"]) - 100, vertex_capacity=len(p["vertices"]) - 50)
    ref = viref.raster(g, *_ix(p), w, h, p["offsets"], depth=depth, vis=vis, **kw)
    _same(_raster(ctx, g, *_ix(p), w, h, p["offsets"], limit=limit, depth=depth, vis=vis, **kw), ref)
    assert (ref[1] == vis).any() and (ref[1] != vis).any()


@pytest.mark.gpu
@pytest.mark.parametrize("near_clip", [0, 1])
def test_raster_near_clip_inside_the_geometry(near_clip, ctx, viref):
    """interior_scene_indexed at 320 x 192: the camera inside the geometry, both pieces of a clipped triangle carry its id"""
    s = synth.interior_scene_indexed(meshlet_bounds=oracle.meshlet_bounds)
    w, h = s["viewport"]
    cd = s["cull"].copy()
    cd["cullingEnabled"] = 0
    commands, count = TC._classic_commands(s, cd)
    offsets = host.assign_triangle_offsets(s["draws"], s["meshes"])
    for pp in (0, 1):
        g = RR.globals_for(cd, (w, h), pp)
        ref = viref.raster(g, commands, count, s["draws"], s["indices"], s["vertices"], w, h, offsets, near_clip=near_clip)
        for limit in (0, 16, INT_MAX):
            _same(_raster(ctx, g, commands, count, s["draws"], s["indices"], s["vertices"], w, h, offsets, limit=limit, near_clip=near_clip), ref)
    clipped = viref.raster(g, commands, count, s["draws"], s["indices"], s["vertices"], w, h, offsets, near_clip=1)
    assert near_clip == 0 or (clipped[1] != viref.raster(g, commands, count, s["draws"], s["indices"], s["vertices"], w, h, offsets)[1]).any()


def _quad_scene(z_second):
    """two draws of the same two-triangle quad, the second at depth z_second: coplanar when it equals the first's"""
    pos = np.array([(-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0)], np.float32)
    ind = np.array([0, 1, 2, 0, 2, 3], np.uint32)
    draws = np.zeros(2, dtype=L.MESHDRAW)
    draws["position"], draws["scale"], draws["orientation"] = [(0, 0, -4.0), (0, 0, z_second)], 1.0, (0, 0, 0, 1)
    meshes = np.zeros(1, dtype=L.MESH)
    meshes["lodCount"], meshes["vertexCount"] = 1, 4
    meshes["lods"]["indexCount"][0, 0] = 6
    commands = np.zeros(2, dtype=L.DRAWCMD)
    commands["drawId"], commands["indexCount"], commands["instanceCount"] = [0, 1], 6, 1
    return dict(meshes=meshes, draws=draws, commands=commands, count=2, indices=ind, vertices=VI.vertices_of(pos),
                offsets=host.assign_triangle_offsets(draws, meshes))


@pytest.mark.gpu
def test_raster_ties_go_to_the_larger_id_and_a_short_span_writes_no_word(ctx, viref):
    w, h = 64, 48
    g = RR.globals_for(host.build_cull_data(viewport=(w, h)), (w, h), 0)
    s = _quad_scene(-4.0)
    assert s["offsets"].tolist() == [0, 2, 4]
    for order in ((0, 1), (1, 0)):  # the command order does not matter
        c = s["commands"][list(order)]
        gpu = _raster(ctx, g, c, 2, s["draws"], s["indices"], s["vertices"], w, h, s["offsets"])
        _same(gpu, viref.raster(g, c, 2, s["draws"], s["indices"], s["vertices"], w, h, s["offsets"]))
        ids = (gpu[1][gpu[1] != 0] & np.uint64(VI.ID_MASK)) - np.uint64(1)
        assert len(ids) > 100 and set(ids.tolist()) == {2, 3}  # draw 1's triangles: the larger ids at equal depth
    # draw 1's span made too small (1 triangle): its second triangle writes depth and no word, draw 0's shows through in the target
    short = np.array([0, 2, 3], np.uint64)
    gpu = _raster(ctx, g, s["commands"], 2, s["draws"], s["indices"], s["vertices"], w, h, short)
    _same(gpu, viref.raster(g, s["commands"], 2, s["draws"], s["indices"], s["vertices"], w, h, short))
    ids = (gpu[1][gpu[1] != 0] & np.uint64(VI.ID_MASK)) - np.uint64(1)
    assert set(ids.tolist()) == {1, 2} and (gpu[0] != 0).sum() == (gpu[1] != 0).sum()
    # a nearer second draw with no span at all: depth from it everywhere it covers, words from draw 0 only
    near = _quad_scene(-3.0)
    none = np.array([0, 2, 2], np.uint64)
    gpu = _raster(ctx, g, near["commands"], 2, near["draws"], near["indices"], near["vertices"], w, h, none, limit=0)
    _same(gpu, viref.raster(g, near["commands"], 2, near["draws"], near["indices"], near["vertices"], w, h, none))
    assert (gpu[1] == 0).sum() > 0 and ((gpu[1] >> np.uint64(34)).astype(np.uint32) < gpu[0].view(np.uint32))[gpu[1] != 0].all()


@pytest.mark.gpu
def test_raster_offsets_sliced_at_a_non_zero_first_draw(ctx, viref):
    """a shard of draws [2, 5): rank-local drawIds, the full offsets advanced by 2: the words of the unsharded pass over those draws"""
    s = TC._soup(23)
    w, h = s["viewport"]
    g = RR.globals_for(s["cull"], (w, h), 1)
    full = s["commands"].copy()
    full["instanceCount"][:2] = 0
    part = s["commands"][2:].copy()
    part["drawId"] -= 2
    whole = _raster(ctx, g, full, 5, s["draws"], s["indices"], s["vertices"], w, h, s["offsets"])
    shard = _raster(ctx, g, part, 3, s["draws"][2:], s["indices"], s["vertices"], w, h, s["offsets"][2:])
    _same(shard, whole)
    _same(shard, viref.raster(g, part, 3, s["draws"][2:], s["indices"], s["vertices"], w, h, s["offsets"][2:]))
    ids = (shard[1][shard[1] != 0] & np.uint64(VI.ID_MASK)) - np.uint64(1)
    assert ids.min() >= s["offsets"][2]


@pytest.mark.gpu
def test_raster_argument_checks(ctx):
    import torch
    from niagara_amd import pipeline as P
    from niagara_amd._lib import NvError
    s = TC._soup(24)
    dev = ctx.device
    w, h = 64, 48
    g = RR.globals_for(s["cull"], (w, h), 0)
    dcb, db, ib, vb = (P.to_device(s[k], dev) for k in ("commands", "draws", "indices", "vertices"))
    dccb = P.to_device(np.array([5, 0, 0, 0], np.uint32), dev)
    ob = P.to_device(s["offsets"], dev)
    d = torch.zeros((h, w), dtype=torch.float32, device=dev)
    v = torch.zeros(h * w + 1, dtype=torch.int64, device=dev)
    ni, nv = len(s["indices"]), len(s["vertices"])
    good = [dcb, dccb, db, ib, vb, d, ob, v]

    def call(a, width=w, height=h, n=5):
        ctx.rasterdepth_indexed_visibility(g, a[0], a[1], a[2], n, a[3], ni, a[4], nv, a[5], width, height, a[6], a[7])
    for k in range(len(good)):  # every NULL row, the two new ones included
        with pytest.raises(NvError, match="NV_EINVAL"):
            call(good[:k] + [None] + good[k + 1:])
    ob8 = torch.zeros(8 * 7 + 4, dtype=torch.uint8, device=dev)
    for bad in (good[:6] + [ob8[4:], v], good[:7] + [v.view(torch.uint8)[4:]]):  # misaligned offsets, misaligned target
        with pytest.raises(NvError, match="NV_EINVAL"):
            call(bad)
    for width, height in ((65, 48), (64, 47), (0, 48)):
        with pytest.raises(NvError, match="NV_EINVAL"):
            call(good, width, height)
    with pytest.raises(NvError, match="NV_ENOMEM"):
        call(good, n=(1 << 20) + 1)
    call(good)
    ctx.status()
    assert (v[:h * w] != 0).any() and int(v[h * w]) == 0


# ---- 2. the resolve

def _resolve(ctx, cd, words, w, h, draws, meshes, offsets, records=True, draw_pixels=True, totals=True):
    """one launch of nv_visibility_resolve_indexed into poisoned records and cleared counters: VisIndexedRef.resolve's dict"""
    import torch
    from niagara_amd import pipeline as P
    dev = ctx.device
    rec = torch.full((w * h * 16,), 0x5A, dtype=torch.uint8, device=dev) if records else None
    dp = torch.zeros(max(1, len(draws)), dtype=torch.int32, device=dev) if draw_pixels else None
    tot = torch.zeros(4, dtype=torch.int64, device=dev) if totals else None
    ctx.visibility_resolve_indexed(cd, torch.from_numpy(np.ascontiguousarray(words, np.uint64).view(np.int64)).to(dev), w, h, _dev(draws, dev, 48),
                                   len(draws), _dev(meshes, dev, 208), len(meshes), P.to_device(np.ascontiguousarray(offsets, np.uint64), dev), rec,
                                   dp, tot)
    ctx.status()
    return dict(records=None if rec is None else P.from_device(rec, L.VISINDEXEDRECORD),
                draw_pixels=None if dp is None else dp.cpu().numpy().view(np.uint32)[:len(draws)],
                totals=None if tot is None else tot.cpu().numpy().view(np.uint64))


def _same_resolve(gpu, ref):
    for k in ("records", "draw_pixels", "totals"):
        if gpu[k] is not None:
            assert gpu[k].tobytes() == ref[k].tobytes(), k


def _words(s, n, seed, run=7):
    """n words over the scene's names: runs of `run` equal triangles, some past the last name, 20 % empty, a few no rasteriser writes"""
    rng = np.random.default_rng(seed)
    total = int(s["offsets"][-1])
    tri = np.repeat(rng.integers(0, total + 40, n // run + 1), run)[:n].astype(np.uint64)
    words = (rng.integers(0, 0x3F800001, n).astype(np.uint64) << np.uint64(34)) | (tri + np.uint64(1))
    words[rng.random(n) < 0.2] = 0
    words[5], words[6], words[7] = 9 << 34, VI.encode(3, VI.TRI34_END - 1), VI.encode(0x3F800000, 0)
    return words


@pytest.mark.gpu
@pytest.mark.parametrize("lod_enabled", [0, 1])
def test_resolve_equals_the_restatement(lod_enabled, ctx, viref):
    """the raster's own target on the two-LOD scene, then hand-made words of every class; each output switched off in turn"""
    s = TC.two_lod_scene()
    w, h = s["viewport"]
    cd = s["cull"].copy()
    cd["lodEnabled"] = lod_enabled
    offsets = host.assign_triangle_offsets(s["draws"], s["meshes"])
    commands, count = TC._classic_commands(s, cd)
    g = RR.globals_for(cd, (w, h), 1)
    vis = _raster(ctx, g, commands, count, s["draws"], s["indices"], s["vertices"], w, h, offsets)[1]
    ref = viref.resolve(cd, vis, s["draws"], s["meshes"], offsets)
    assert ref["totals"][0] > w * h // 8 and ref["totals"][1] == 0
    _same_resolve(_resolve(ctx, cd, vis, w, h, s["draws"], s["meshes"], offsets), ref)
    s = dict(s, offsets=offsets)
    words = _words(s, w * h, 5)
    draws, meshes = s["draws"].copy(), s["meshes"].copy()
    draws[0]["meshIndex"] = 99                             # a mesh index past the table
    meshes[1]["lods"]["indexCount"][:2] = 3 * 10           # a LOD shorter than the span
    meshes[3]["lods"]["indexOffset"][:2] = 0xFFFFFFFF - 3  # only triangle 0's positions fit 32 bits
    ref = viref.resolve(cd, words, draws, meshes, offsets)
    assert 0 < ref["totals"][1] < ref["totals"][0] < w * h
    _same_resolve(_resolve(ctx, cd, words, w, h, draws, meshes, offsets), ref)
    for off in range(3):
        kw = dict(records=off != 0, draw_pixels=off != 1, totals=off != 2)
        _same_resolve(_resolve(ctx, cd, words, w, h, draws, meshes, offsets, **kw), ref)
    # no draws at all; offsets that start above 0 (no draw has an offset <= tri34)
    _same_resolve(_resolve(ctx, cd, words, w, h, draws[:0], meshes, offsets[:1]), viref.resolve(cd, words, draws[:0], meshes, offsets[:1]))
    late = offsets + np.uint64(50)
    ref = viref.resolve(cd, words, draws, meshes, late)
    _same_resolve(_resolve(ctx, cd, words, w, h, draws, meshes, late), ref)
    assert (ref["records"][words != 0]["drawId"] == 0xFFFFFFFF).any()


@pytest.mark.gpu
def test_resolve_second_trip_of_the_persistent_grid(ctx, viref):
    import torch
    cus = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    w, h, items = PC.second_trip_sizes(cus)["pixel"]
    PC.check_second_trip(items, w, h, cus)
    s = TC._soup(25)
    words = _words(s, w * h, 6, run=37)
    ref = viref.resolve(s["cull"], words, s["draws"], s["meshes"], s["offsets"])
    _same_resolve(_resolve(ctx, s["cull"], words, w, h, s["draws"], s["meshes"], s["offsets"]), ref)


@pytest.mark.gpu
def test_resolve_run_edges(ctx, viref):
    """a run of another draw starting on lanes 0, 1, 15-17, 31-33, 47-49, 62, 63; neighbours that differ in the triangle only and in the depth
    only; an unresolved first lane with valid lanes behind it; a ragged last wave"""
    s = TC._soup(26)
    off = s["offsets"]
    rows = []
    for start in (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 62, 63):
        row = np.full(64, VI.encode(100, int(off[4]) + 3), np.uint64)
        row[start:] = VI.encode(100, int(off[2]) + 5)          # another draw from `start` on
        rows.append(row)
        row = np.full(64, VI.encode(100, int(off[4]) + 3), np.uint64)
        row[start:] = VI.encode(100, int(off[4]) + 4)          # the same draw, the next triangle
        rows.append(row)
        row = np.full(64, VI.encode(100, int(off[4]) + 3), np.uint64)
        row[start:] = VI.encode(101, int(off[4]) + 3)          # the depth only
        rows.append(row)
        row = np.full(64, VI.encode(100, int(off[3])), np.uint64)
        row[start] = VI.encode(7, int(off[-1]) + 9)            # one unresolved lane inside a run
        row[(start + 1) % 64] = 0                               # and one empty one
        rows.append(row)
    first = np.full(64, VI.encode(1, int(off[1]) + 1), np.uint64)
    first[0] = 5 << 34                                          # a first lane without an id, valid lanes behind it
    rows.append(first)
    first = first.copy()
    first[0] = VI.encode(1, int(off[-1]))                       # a first lane past the last name
    rows.append(first)
    words = np.concatenate(rows + [np.full(37, VI.encode(9, int(off[1])), np.uint64)])  # a ragged last wave
    w, h = len(words), 1
    ref = viref.resolve(s["cull"], words, s["draws"], s["meshes"], off)
    assert ref["totals"][1] == 13 + 2
    _same_resolve(_resolve(ctx, s["cull"], words, w, h, s["draws"], s["meshes"], off), ref)


@pytest.mark.gpu
def test_resolve_many_draws_per_wave(ctx, viref):
    """an image of many small draws: every pixel of a wave names another of 150 draws (more than the kernel's wave-uniform trips, so the
    lanes that stay open search for themselves), runs of 1, 2 and 5 pixels, every class of unresolved word among them, a ragged last wave"""
    s = VI.triangle_soup([3] * 150, 31)
    cd = host.build_cull_data(viewport=(64, 48), draw_count=150)
    off = s["offsets"]
    rng = np.random.default_rng(32)
    draws, meshes = s["draws"].copy(), s["meshes"].copy()
    draws["meshIndex"][7::31] = 999                       # mesh indices past the table
    meshes["lods"]["indexCount"][5::29, 0] = 3            # LODs shorter than the span
    for run in (1, 2, 5):
        n = 64 * 37 + 29
        d = np.repeat(rng.permutation(np.arange(150).repeat(n // 150 + 1))[:n // run + 1], run)[:n]
        tri = off[d] + rng.integers(0, 3, n).astype(np.uint64)
        words = (rng.integers(0, 0x3F800001, n).astype(np.uint64) << np.uint64(34)) | (tri + np.uint64(1))
        words[rng.random(n) < 0.1] = 0
        words[rng.random(n) < 0.05] = VI.encode(9, int(off[-1]) + 3)
        ref = viref.resolve(cd, words, draws, meshes, off)
        assert len(set(ref["records"]["drawId"][:64].tolist())) > 8 and 0 < ref["totals"][1] < ref["totals"][0]
        _same_resolve(_resolve(ctx, cd, words, n, 1, draws, meshes, off), ref)


@pytest.mark.gpu
def test_resolve_argument_checks(ctx):
    import torch
    from niagara_amd import pipeline as P
    from niagara_amd._lib import NvError
    s = TC._soup(27)
    dev = ctx.device
    w, h = 64, 48
    vis = torch.zeros(w * h + 1, dtype=torch.int64, device=dev)
    db, mb, ob = P.to_device(s["draws"], dev), P.to_device(s["meshes"], dev), P.to_device(s["offsets"], dev)
    rec = torch.zeros(w * h * 16 + 16, dtype=torch.uint8, device=dev)
    tot = torch.zeros(5, dtype=torch.int64, device=dev)
    cd = s["cull"]

    def call(v=vis, width=w, height=h, d=db, m=mb, o=ob, r=rec, t=tot, nd=5, nm=5):
        ctx.visibility_resolve_indexed(cd, v, width, height, d, nd, m, nm, o, r, None, t)
    for kw in (dict(v=None), dict(o=None), dict(d=None), dict(m=None), dict(width=0), dict(height=16385),
               dict(v=vis.view(torch.uint8)[4:]), dict(o=ob.view(torch.uint8)[4:]), dict(r=rec[8:]), dict(t=tot.view(torch.uint8)[4:]),
               dict(d=db.view(torch.uint8)[8:]), dict(m=mb.view(torch.uint8)[8:])):
        with pytest.raises(NvError, match="NV_EINVAL"):
            call(**kw)
    call(d=None, nd=0, o=ob[:1])  # no draws: the array may be NULL
    call()
    ctx.status()


# ---- 3. capture

@pytest.mark.gpu
def test_raster_resolve_and_attributes_replay_from_a_graph(ctx, viref, iaref):
    """the chain raster -> resolve -> attributes captured once and replayed once into poisoned outputs: each stage's restatement"""
    import torch
    import test_visattr_gpu as TA
    from niagara_amd import pipeline as P
    s = TC.occluder_with_attributes()
    w, h = s["viewport"]
    cd = s["cull"].copy()
    cd["cullingEnabled"] = 0
    offsets = host.assign_triangle_offsets(s["draws"], s["meshes"])
    commands, count = TC._classic_commands(s, cd)
    g = RR.globals_for(cd, (w, h), 1)
    want = viref.raster(g, commands, count, s["draws"], s["indices"], s["vertices"], w, h, offsets)
    want_res = viref.resolve(cd, want[1], s["draws"], s["meshes"], offsets)
    want_att = iaref.attributes(g, want_res["records"], w, h, s["draws"], s["indices"], s["vertices"], s["materials"])
    assert want_att["totals"][0] > w * h // 4
    dev = ctx.device
    dcb, db, mb, ib, vb, ob = (P.to_device(np.ascontiguousarray(a), dev) for a in (commands, s["draws"], s["meshes"], s["indices"], s["vertices"], offsets))
    mat = P.to_device(s["materials"], dev)
    att = dict(attributes=torch.zeros(w * h * 64, dtype=torch.uint8, device=dev), gbuffer0=torch.zeros(w * h, dtype=torch.int32, device=dev),
               gbuffer1=torch.zeros(w * h, dtype=torch.int32, device=dev), totals=torch.zeros(4, dtype=torch.int64, device=dev))
    dccb = P.to_device(np.array([count, 0, 0, 0], np.uint32), dev)
    d = torch.zeros((h, w), dtype=torch.float32, device=dev)
    v = torch.zeros((h, w), dtype=torch.int64, device=dev)
    rec = torch.zeros(w * h * 16, dtype=torch.uint8, device=dev)
    dp = torch.zeros(len(s["draws"]), dtype=torch.int32, device=dev)
    tot, rtot = torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)

    def step():
        for t in (d, v, dp, tot, rtot, att["totals"]):
            t.zero_()
        ctx.rasterdepth_indexed_visibility(g, dcb, dccb, db, len(s["draws"]), ib, len(s["indices"]), vb, len(s["vertices"]), d, w, h, ob, v, tot)
        ctx.visibility_resolve_indexed(cd, v, w, h, db, len(s["draws"]), mb, len(s["meshes"]), ob, rec, dp, rtot)
        ctx.visibility_attributes_indexed(g, rec, w, h, db, len(s["draws"]), ib, len(s["indices"]), vb, len(s["vertices"]), mat, len(s["materials"]),
                                          att["attributes"], att["gbuffer0"], att["gbuffer1"], att["totals"])
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        step()  # eagerly: the warm-up of every launch
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            step()
        torch.cuda.synchronize()
        rec.fill_(0x5A)
        v.fill_(-1)
        att["attributes"].fill_(0x5A)
        att["gbuffer0"].fill_(0x5A5A5A5A)
        att["gbuffer1"].fill_(0x5A5A5A5A)
        graph.replay()
        torch.cuda.synchronize()
    ctx.status()
    assert d.cpu().numpy().tobytes() == want[0].tobytes() and v.cpu().numpy().view(np.uint64).tobytes() == want[1].tobytes()
    assert tot.cpu().numpy().view(np.uint64).tolist() == want[2].tolist()
    got = dict(records=P.from_device(rec, L.VISINDEXEDRECORD), draw_pixels=dp.cpu().numpy().view(np.uint32),
               totals=rtot.cpu().numpy().view(np.uint64))
    _same_resolve(got, want_res)
    _same_attributes(TA._host(att), want_att)


# ---- 4. the attribute pass


def _attributes(ctx, g, records, w, h, draws, indices, vertices, materials=None, outputs=(True, True, True, True), counts=None):
    """one launch of nv_visibility_attributes_indexed into poisoned outputs: test_visattr_gpu._host's dict (None for an output switched off)"""
    import torch
    import test_visattr_gpu as TA
    from niagara_amd import pipeline as P
    dev = ctx.device
    n = w * h
    cnt = dict(draws=len(draws), indices=len(indices), vertices=len(vertices), materials=0 if materials is None else len(materials))
    cnt.update(counts or {})
    out = dict(attributes=torch.full((n * 64,), 0x5A, dtype=torch.uint8, device=dev) if outputs[0] else None,
               gbuffer0=torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=dev) if outputs[1] and materials is not None else None,
               gbuffer1=torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=dev) if outputs[2] and materials is not None else None,
               totals=torch.zeros(4, dtype=torch.int64, device=dev))
    rb = records if isinstance(records, torch.Tensor) else P.to_device(np.ascontiguousarray(records, L.VISINDEXEDRECORD), dev)
    ctx.visibility_attributes_indexed(g, rb, w, h, _dev(draws, dev, 48), cnt["draws"], _dev(np.ascontiguousarray(indices, np.uint32), dev, 4),
                                      cnt["indices"], _dev(vertices, dev, 16), cnt["vertices"],
                                      None if materials is None else P.to_device(materials, dev), cnt["materials"], out["attributes"],
                                      out["gbuffer0"], out["gbuffer1"], out["totals"] if outputs[3] else None)
    ctx.status()
    return TA._host(out)


def _same_attributes(got, want, gbuffers=True):
    """tests/test_visattr_gpu.py's conditions: records and gbuffer1 bit for bit, gbuffer0 within one code per channel and >= 90 % of the
    channels equal (pow and log2 are the device's), totals"""
    import test_visattr_gpu as TA
    TA._same_attributes(got, want, gbuffers)


@pytest.mark.gpu
def test_chain_on_the_occluder_scene_equals_the_restatements(ctx, viref, iaref):
    """raster -> resolve -> attributes over every draw of occluder_scene_indexed at 320 x 192: each stage against its restatement, with and
    without the material table, each output switched off in turn"""
    s = TC.occluder_with_attributes()
    w, h = s["viewport"]
    vis, res, offsets, commands, count = TC.classic_records(s, viref)
    cd = s["cull"].copy()
    cd["cullingEnabled"] = 0
    g = RR.globals_for(cd, (w, h), 0)
    gpu = _raster(ctx, g, commands, count, s["draws"], s["indices"], s["vertices"], w, h, offsets)
    assert gpu[1].tobytes() == vis.tobytes()
    got = _resolve(ctx, cd, gpu[1], w, h, s["draws"], s["meshes"], offsets)
    _same_resolve(got, res)
    rec = got["records"]
    want = iaref.attributes(g, rec, w, h, s["draws"], s["indices"], s["vertices"], s["materials"])
    assert want["totals"][0] > w * h // 4 and want["totals"][3] > 0
    _same_attributes(_attributes(ctx, g, rec, w, h, s["draws"], s["indices"], s["vertices"], s["materials"]), want)
    bare = iaref.attributes(g, rec, w, h, s["draws"], s["indices"], s["vertices"], None)
    _same_attributes(_attributes(ctx, g, rec, w, h, s["draws"], s["indices"], s["vertices"], None), bare, gbuffers=False)
    for off in range(4):
        o = _attributes(ctx, g, rec, w, h, s["draws"], s["indices"], s["vertices"], s["materials"], outputs=tuple(k != off for k in range(4)))
        if off != 0:
            assert o["attributes"].tobytes() == want["attributes"].tobytes()
        if off != 2:
            assert o["gbuffer1"].tobytes() == want["gbuffer1"].tobytes()
        assert o["totals"].tolist() == (want["totals"].tolist() if off != 3 else [0, 0, 0, 0])


def _attr_records(s, n, seed, run):
    """n records over the scene's triangles in runs of `run`: 15 % empty, and one in eight runs of each invalid class (a draw past the
    table, an index position at the buffer's end, a vertex offset that takes a corner past the vertices)"""
    rng = np.random.default_rng(seed)
    runs = n // run + 1
    d = rng.integers(0, len(s["draws"]), runs)
    lod = s["meshes"]["lods"][s["draws"]["meshIndex"][d], 0]
    t = (rng.random(runs) * (lod["indexCount"] // 3)).astype(np.int64)
    rec = np.zeros(runs, dtype=L.VISINDEXEDRECORD)
    rec["drawId"], rec["indexPosition"], rec["depthBits"] = d, lod["indexOffset"] + 3 * t, rng.integers(0, 0x3F800001, runs)
    rec["vertexOffset"] = s["meshes"]["vertexOffset"][s["draws"]["meshIndex"][d]]
    kind = rng.integers(0, 24, runs)
    rec["drawId"][kind == 0] = len(s["draws"]) + 2
    rec["indexPosition"][kind == 1] = len(s["indices"]) - 2
    rec["vertexOffset"][kind == 2] = len(s["vertices"])
    rec = np.repeat(rec, run)[:n]
    empty = rng.random(n) < 0.15
    rec[empty] = np.array((0xFFFFFFFF, 0, 0, 0), dtype=L.VISINDEXEDRECORD)
    return rec


@pytest.mark.gpu
def test_attributes_second_trip_of_the_persistent_grid(ctx, iaref):
    import torch
    cus = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    w, h, items = PC.second_trip_sizes(cus)["pixel"]
    PC.check_second_trip(items, w, h, cus)
    s = TC.occluder_with_attributes()
    g = RR.globals_for(host.build_cull_data(viewport=(w, h)), (w, h), 0)
    rec = _attr_records(s, w * h, 7, run=29)
    want = iaref.attributes(g, rec, w, h, s["draws"], s["indices"], s["vertices"], s["materials"])
    assert want["totals"][0] > 0 and want["totals"][1] > 0
    _same_attributes(_attributes(ctx, g, rec, w, h, s["draws"], s["indices"], s["vertices"], s["materials"]), want)


@pytest.mark.gpu
def test_attributes_run_edges_and_invalid_records(ctx, iaref):
    """a run start on lanes 0, 1, 15-17, 31-33, 47-49, 62, 63 by each word of the key alone (the draw, the index position, the vertex
    offset) and by the depth alone (no start); a first lane that is invalid or empty with valid lanes behind it; a ragged last wave; and
    every invalid class"""
    s = TC.occluder_with_attributes()
    draws, meshes = s["draws"], s["meshes"]
    two = [i for i in range(len(draws)) if draws["meshIndex"][i] == draws["meshIndex"][len(draws) - 1]][:2]  # two draws of one mesh
    assert len(two) == 2
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
    want = iaref.attributes(g, rec, w, h, draws, s["indices"], s["vertices"], s["materials"])
    assert want["totals"][1] == 4
    _same_attributes(_attributes(ctx, g, rec, w, h, draws, s["indices"], s["vertices"], s["materials"]), want)
    # a material index past the table, with and without the table; capacities that cut the buffers short
    bad = draws.copy()
    bad["materialIndex"][two[0]] = len(s["materials"])
    for mats in (s["materials"], None):
        want = iaref.attributes(g, rec, w, h, bad, s["indices"], s["vertices"], mats)
        _same_attributes(_attributes(ctx, g, rec, w, h, bad, s["indices"], s["vertices"], mats), want, gbuffers=mats is not None)
    cut = dict(indices=int(lod["indexOffset"]) + 9)  # the run's triangle at + 9 loses its last index
    want = iaref.attributes(g, rec, w, h, draws, s["indices"], s["vertices"], s["materials"], counts=cut)
    assert want["totals"][1] > 4
    _same_attributes(_attributes(ctx, g, rec, w, h, draws, s["indices"], s["vertices"], s["materials"], counts=cut), want)


@pytest.mark.gpu
def test_attributes_argument_checks(ctx):
    import torch
    from niagara_amd import pipeline as P
    from niagara_amd._lib import NvError
    s = TC.occluder_with_attributes()
    dev = ctx.device
    w, h = 16, 4
    g = RR.globals_for(host.build_cull_data(viewport=(w, h)), (w, h), 0)
    rec = torch.zeros(w * h * 16 + 16, dtype=torch.uint8, device=dev)
    db, ib, vb, mb = (P.to_device(s[k], dev) for k in ("draws", "indices", "vertices", "materials"))
    att = torch.zeros(w * h * 64 + 16, dtype=torch.uint8, device=dev)
    g0, g1 = torch.zeros(w * h + 1, dtype=torch.int32, device=dev), torch.zeros(w * h, dtype=torch.int32, device=dev)
    tot = torch.zeros(5, dtype=torch.int64, device=dev)
    nd, ni, nv, nm = len(s["draws"]), len(s["indices"]), len(s["vertices"]), len(s["materials"])

    def call(r=rec, width=w, height=h, d=db, i=ib, v=vb, m=mb, a=att, b0=g0, b1=g1, t=tot, glob=g, nmat=nm):
        ctx.visibility_attributes_indexed(glob, r, width, height, d, nd, i, ni, v, nv, m, nmat, a, b0, b1, t)
    other = g.copy()
    other["screenWidth"] = w + 1
    for kw in (dict(r=None), dict(d=None), dict(i=None), dict(v=None), dict(width=0), dict(height=16385), dict(glob=other), dict(m=None),
               dict(m=None, nmat=0), dict(r=rec[8:]), dict(a=att[8:]), dict(d=db.view(torch.uint8)[8:]), dict(v=vb.view(torch.uint8)[8:]),
               dict(m=mb.view(torch.uint8)[8:]), dict(t=tot.view(torch.uint8)[4:]), dict(i=ib.view(torch.uint8)[2:]),
               dict(b0=g0.view(torch.uint8)[2:])):
        with pytest.raises(NvError, match="NV_EINVAL"):
            call(**kw)
    call(m=None, nmat=0, b0=None, b1=None)  # without a table: no G-buffer
    call()
    ctx.status()


# ---- 5. the two paths show the same image

def _cluster_chain(ctx, s, cd, g, w, h):
    """every draw of the scene through nv_rasterdepth with stable ids -> nv_visibility_resolve -> nv_visibility_attributes: (depth, host dict)"""
    import torch
    import test_visattr_gpu as TA
    from niagara_amd import pipeline as P
    dev = ctx.device
    draws = s["draws"].copy()
    oracle.assign_visibility_offsets(draws, s["meshes"])
    cmds, ids = [], []
    for d in range(len(draws)):
        lod = s["meshes"]["lods"][int(draws[d]["meshIndex"]), 0]
        for k in range(0, int(lod["meshletCount"]), 64):
            n = min(64, int(lod["meshletCount"]) - k)
            ids += [len(cmds) | j << 24 for j in range(n)]
            cmds.append((d, int(lod["meshletOffset"]) + k, n, 1, int(draws[d]["meshletVisibilityOffset"]) + k))
    commands = np.array(cmds, dtype=L.TASKCMD)
    cc4 = np.array([len(ids), 0, 0, 0], np.uint32)
    cib = np.concatenate([np.array(ids, np.uint32), np.zeros(512, np.uint32)])
    oracle.clustersubmit(cc4, cib)
    t = [P.to_device(a, dev) for a in (commands, draws, s["meshlets"], s["data"], s["vertices"], cib, cc4)]
    mb, mat = P.to_device(s["meshes"], dev), P.to_device(s["materials"], dev)
    n = w * h
    depth = torch.zeros((h, w), dtype=torch.float32, device=dev)
    vis = torch.zeros((h, w), dtype=torch.int64, device=dev)
    rec = torch.full((n * 16,), 0x5A, dtype=torch.uint8, device=dev)
    out = dict(attributes=torch.full((n * 64,), 0x5A, dtype=torch.uint8, device=dev), gbuffer0=torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=dev),
               gbuffer1=torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=dev), totals=torch.zeros(4, dtype=torch.int64, device=dev))
    ctx.set_option(P.NV_OPT_RASTER_VISIBILITY_ID, 1)
    try:
        ctx.rasterdepth(g, *t, depth, w, h, vis)
    finally:
        ctx.set_option(P.NV_OPT_RASTER_VISIBILITY_ID, 0)
    ctx.visibility_resolve(cd, vis, w, h, t[1], len(draws), mb, len(s["meshes"]), rec)
    ctx.visibility_attributes(g, rec, w, h, t[1], len(draws), t[2], len(s["meshlets"]), t[3], len(s["data"]), t[4], len(s["vertices"]), mat,
                              len(s["materials"]), out["attributes"], out["gbuffer0"], out["gbuffer1"], out["totals"])
    ctx.status()
    return depth.cpu().numpy(), P.from_device(rec, L.VISRECORD), TA._host(out)


@pytest.mark.gpu
def test_the_classic_chain_shows_what_the_cluster_chain_shows(ctx, viref):
    """occluder_scene_indexed at 320 x 192, all draws through either path: NvPixelAttributes, gbuffer0 and gbuffer1 bit-identical at EVERY
    pixel.  It holds because the two ids are order-isomorphic there (TC.order_condition: one LOD, no skipped triangle, (draw, meshlet,
    triangle) increasing on both sides) and both rasters write the same depth bits, so ties fall on the same triangle."""
    s = TC.occluder_with_attributes()
    starts = TC.order_condition(s)
    w, h = s["viewport"]
    assert (w, h) == (320, 192)
    vis, res, offsets, commands, count = TC.classic_records(s, viref)
    cd = s["cull"].copy()
    cd["cullingEnabled"] = 0
    g = RR.globals_for(cd, (w, h), 0)
    depth_c, rec_c, attr_c = _cluster_chain(ctx, s, cd, g, w, h)
    depth_i, vis_i, _ = _raster(ctx, g, commands, count, s["draws"], s["indices"], s["vertices"], w, h, offsets)
    assert depth_c.tobytes() == depth_i.tobytes() and (depth_i != 0).sum() > w * h // 4  # the condition's second half, on the device
    rec_i = _resolve(ctx, cd, vis_i, w, h, s["draws"], s["meshes"], offsets)["records"]
    assert TC.meshlet_records(s, rec_i, starts).tobytes() == rec_c.tobytes()  # the same triangle at every pixel
    attr_i = _attributes(ctx, g, rec_i, w, h, s["draws"], s["indices"], s["vertices"], s["materials"])
    for k in ("attributes", "gbuffer0", "gbuffer1"):
        assert attr_i[k].tobytes() == attr_c[k].tobytes(), k
    assert attr_i["totals"].tolist() == attr_c["totals"].tolist() and attr_i["totals"][0] > w * h // 4


# ---- 6. frames

class _FrameRaster:
    """RI.IndexedRef.raster's signature with the frame's visibility target kept inside (the restated word): a call without `depth` (the early
    pass) clears it, the others load it.  history[k] = the target after the k-th call"""

    def __init__(self, viref, offsets):
        self.viref, self.offsets, self.vis, self.history = viref, offsets, None, []

    def raster(self, g, commands, count, draws, indices, vertices, width, height, depth=None, **kw):
        d, self.vis, tot = self.viref.raster(g, commands, count, draws, indices, vertices, width, height, self.offsets, depth=depth,
                                             vis=None if depth is None else self.vis, **kw)
        self.history.append(self.vis.copy())
        return d, tot


def _pipe_kw(s):
    return dict(task_capacity=4096, cluster_capacity=4096 * 64, vertices=s["vertices"], indices=s["indices"], meshlet_data=s["data"], stable_ids=True)


@pytest.mark.gpu
@pytest.mark.parametrize("post_pass", [False, True])
def test_classic_frames_with_a_visibility_target_equal_the_oracle_chain(post_pass, viref, iaref, sref):
    """frame(task=False, visibility=) over 3 frames: depth and the visibility target phase by phase against the oracle's classic chain with
    the restated word; then resolve(classic=True) and attributes(classic=True) of the last frame against their restatements, and shade()
    behind them within one 8-bit code of tests/shade_ref.c on the RESTATED G-buffers and the oracle chain's depth"""
    import raster_indexed_ref as RI
    from niagara_amd import pipeline as P
    s = TC.occluder_with_attributes()
    w, h = s["viewport"]
    offsets = host.assign_triangle_offsets(s["draws"], s["meshes"])
    fr = _FrameRaster(viref, offsets)
    want = RI.oracle_frames_classic(s, 3, post_pass=post_pass, iref=fr)
    names = ["early", "late"] + (["post"] if post_pass else [])
    pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], **_pipe_kw(s))
    try:
        vis = pipe.new_visibility()
        vis.fill_(-1)  # the early raster clears it
        k = 0
        for f in range(3):
            got = {}
            pipe.frame(s["cull"], post_pass=post_pass, task=False, visibility=vis,
                       on_phase=lambda name: got.__setitem__(name, (pipe.depth.cpu().numpy().copy(), vis.cpu().numpy().view(np.uint64).copy())))
            for name in names:
                assert got[name][0].tobytes() == want[f][name]["depth"].tobytes(), (f, name)
                assert got[name][1].tobytes() == fr.history[k].tobytes(), (f, name)
                k += 1
        cd = s["cull"].copy()
        cd["clusterOcclusionEnabled"] = 0
        res = pipe.resolve(s["cull"], vis, classic=True)
        ref = viref.resolve(cd, fr.history[-1], s["draws"], s["meshes"], offsets)
        rec = P.from_device(res["records"], L.VISINDEXEDRECORD)
        assert rec.tobytes() == ref["records"].tobytes() and res["meshlet_seen"] is None
        assert res["draw_pixels"].cpu().numpy().view(np.uint32)[:len(s["draws"])].tolist() == ref["draw_pixels"].tolist()
        assert res["totals"].cpu().numpy().tolist() == ref["totals"].tolist() and ref["totals"][1] == 0 and ref["totals"][0] > w * h // 4
        import test_visattr_gpu as TA
        out = pipe.attributes(s["cull"], res["records"], materials=s["materials"], classic=True)
        g = synth.make_globals(s["cull"], (w, h))
        want_att = iaref.attributes(g, rec, w, h, s["draws"], s["indices"], s["vertices"], s["materials"])
        _same_attributes(TA._host(out), want_att)
        import shade_ref as SR
        import test_shade_gpu as TS
        camera, sun = (0.0, 0.0, 0.0), np.array([0.35, 0.6, 0.72]) / np.linalg.norm([0.35, 0.6, 0.72])
        color = pipe.shade(s["cull"], out["gbuffer0"], out["gbuffer1"], camera, sun, shadow=None)
        pipe.ctx.status()
        sd = host.build_shade_data(g, camera, sun, 0, w, h)
        depth = want[-1][names[-1]]["depth"]
        shaded = sref.shade(sd, want_att["gbuffer0"].reshape(h, w), want_att["gbuffer1"].reshape(h, w), depth, znear=float(s["cull"]["znear"][0]),
                            shadow=None)
        got = SR.channels(color.cpu().numpy().view(np.uint32))
        TS._close("shade behind the classic frame", got, SR.channels(shaded), alpha=True)
        assert (got[..., :3][depth == 0] == 0).all() and (got[..., :3][depth > 0] > 0).any()
        pipe.ctx.status()
    finally:
        pipe.ctx.close()


@pytest.mark.gpu
def test_two_local_shards_stitch_to_the_unsharded_classic_frame(viref):
    from niagara_amd import pipeline as P
    s = TC.occluder_with_attributes()
    w, h = s["viewport"]
    pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], **_pipe_kw(s))
    try:
        vis = pipe.new_visibility()
        for _ in range(2):
            pipe.frame(s["cull"], post_pass=True, task=False, visibility=vis)
        res = pipe.resolve(s["cull"], vis, classic=True)
        out = pipe.attributes(s["cull"], res["records"], materials=s["materials"], classic=True)
        want = [t.cpu().numpy().tobytes() for t in (pipe.depth, vis, res["records"], res["draw_pixels"], out["attributes"], out["gbuffer0"], out["gbuffer1"])]
        pipe.ctx.status()
    finally:
        pipe.ctx.close()
    assert np.frombuffer(want[1], np.uint64).any()
    shards = P.ShardedVisibilityPipeline.local_shards(s["meshes"], s["meshlets"], s["draws"], s["viewport"], 2, **_pipe_kw(s))
    try:
        assert shards.ranges[1][0] > 0
        targets = shards.new_visibility()
        for _ in range(2):
            shards.frame(s["cull"], post_pass=True, task=False, visibility=targets)
        for p, v in zip(shards.pipes, targets):  # every shard holds the unsharded target and resolves it with the scene's draw ids
            res = p.resolve(s["cull"], v, classic=True)
            out = p.attributes(s["cull"], res["records"], materials=s["materials"], classic=True)
            got = [t.cpu().numpy().tobytes() for t in (p.depth, v, res["records"], res["draw_pixels"], out["attributes"], out["gbuffer0"], out["gbuffer1"])]
            assert got == want
        shards.status()
    finally:
        shards.close()


@pytest.mark.gpu
def test_the_refusals_that_remain_still_raise():
    from niagara_amd import pipeline as P
    from niagara_amd._lib import NvError
    s = TC.occluder_with_attributes()
    kw = dict(_pipe_kw(s), stable_ids=False)
    pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], **kw)
    try:
        vis = pipe.new_visibility()
        for task in (True, False):
            with pytest.raises(NvError):
                pipe.frame(s["cull"], task=task, visibility=vis)
        pipe.cull(s["cull"], late=False, task=False)
        with pytest.raises(NvError):
            pipe.render_draws(s["cull"], late=False, visibility=vis)
        with pytest.raises(NvError):
            pipe.resolve(s["cull"], vis, classic=True)
        with pytest.raises(NvError):
            pipe.frame(s["cull"], task=False, textures=True)
    finally:
        pipe.ctx.close()
    kw = dict(_pipe_kw(s))
    del kw["indices"]  # stable ids without an index buffer: the classic forms have nothing to read
    pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], **kw)
    try:
        vis = pipe.new_visibility()
        with pytest.raises(NvError):
            pipe.frame(s["cull"], task=False, visibility=vis)
        with pytest.raises(NvError):
            pipe.resolve(s["cull"], vis, classic=True)
        with pytest.raises(NvError):
            pipe.attributes(s["cull"], vis, classic=True)
    finally:
        pipe.ctx.close()
    shards = P.ShardedVisibilityPipeline.local_shards(s["meshes"], s["meshlets"], s["draws"], s["viewport"], 2, **dict(_pipe_kw(s), stable_ids=False))
    try:
        with pytest.raises(NvError):
            shards.frame(s["cull"], task=False, visibility=shards.new_visibility())
    finally:
        shards.close()
