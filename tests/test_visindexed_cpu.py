"""The visibility buffer of the indexed draws on the CPU: the ABI, nv_assign_triangle_offsets, the restated raster
(tests/visindexed_ref.c) against the depth-only references, and the restated resolve as the inverse of the restated raster under the
oracle's draw-level cull (its LOD select writes the commands the names are checked against)."""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
import raster_clip_ref as RC
import raster_indexed_ref as RI
import raster_ref as RR
import visindexed_ref as VI
from niagara_amd import host, synth
from niagara_amd import layouts as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 63, 64, 65, 200]


@pytest.fixture(scope="session")
def viref(tmp_path_factory):
    return VI.load(tmp_path_factory.mktemp("visindexed_ref"))


@pytest.fixture(scope="session")
def cref(tmp_path_factory):
    return RC.load(tmp_path_factory.mktemp("raster_clip_ref_vi"))


# ---- 1. the ABI

def test_abi_has_the_symbols_and_the_record(tmp_path):
    from niagara_amd import _lib
    header = open(os.path.join(ROOT, "include", "niagara_vis.h")).read()
    for name in ("nv_assign_triangle_offsets", "nv_rasterdepth_indexed_visibility", "nv_visibility_resolve_indexed",
                 "nv_visibility_attributes_indexed"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)
    src = tmp_path / "c.c"
    src.write_text('#include <stddef.h>\n#include "niagara_vis.h"\nint main(void){NvVisIndexedRecord r; return sizeof(r)==16 && offsetof(NvVisIndexedRecord,'
                   'drawId)==0 && offsetof(NvVisIndexedRecord,indexPosition)==4 && offsetof(NvVisIndexedRecord,vertexOffset)==8 && '
                   'offsetof(NvVisIndexedRecord,depthBits)==12?0:1;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "c")])
    subprocess.check_call([str(tmp_path / "c")])
    assert L.VISINDEXEDRECORD.itemsize == 16 and L.VISINDEXEDRECORD.names == ("drawId", "indexPosition", "vertexOffset", "depthBits")
    assert [L.VISINDEXEDRECORD.fields[n][1] for n in L.VISINDEXEDRECORD.names] == [0, 4, 8, 12]


# ---- 2. the names

def _meshes(index_counts):
    """one mesh per list of per-LOD index counts"""
    m = np.zeros(len(index_counts), dtype=L.MESH)
    for i, lods in enumerate(index_counts):
        m[i]["lodCount"] = len(lods)
        for l, k in enumerate(lods[:8]):
            m[i]["lods"]["indexCount"][l] = k
    return m


def _draws_of(mesh_indices):
    d = np.zeros(len(mesh_indices), dtype=L.MESHDRAW)
    d["meshIndex"], d["scale"], d["orientation"] = mesh_indices, 1.0, (0, 0, 0, 1)
    return d


def test_offsets_are_the_prefix_of_the_widest_lods():
    meshes = _meshes([[30, 62, 9], [3], [0], [5, 4]])  # LOD 1 the widest (20 triangles, remainder dropped); 1; 0; 1
    off = host.assign_triangle_offsets(_draws_of([0, 1, 0, 2, 3, 1]), meshes)
    assert off.dtype == np.uint64 and off.tolist() == [0, 20, 21, 41, 41, 42, 43]
    # lodCount above NV_MAX_LODS reads 8 LODs; a LOD at or past lodCount is not read
    meshes = _meshes([[3] * 8, [3, 300]])
    meshes[0]["lodCount"], meshes[1]["lodCount"] = 200, 1
    assert host.assign_triangle_offsets(_draws_of([0, 1]), meshes).tolist() == [0, 1, 2]


def test_offsets_a_bad_mesh_index_spans_nothing_and_no_draws_give_one_zero():
    meshes = _meshes([[30], [60]])
    assert host.assign_triangle_offsets(_draws_of([1, 2, 0xFFFFFFFF, 0]), meshes).tolist() == [0, 20, 20, 20, 30]
    assert host.assign_triangle_offsets(_draws_of([]), meshes).tolist() == [0]
    assert host.assign_triangle_offsets(_draws_of([0, 0]), meshes[:0]).tolist() == [0, 0, 0]


def test_offsets_refuse_more_than_2_pow_34_minus_2_triangles():
    from niagara_amd._lib import NvError
    widest = 0xFFFFFFFF // 3  # 1431655765 triangles: the most one LOD can hold
    room = (1 << 34) - 2 - 12 * widest
    assert 0 < room < widest
    meshes = _meshes([[0xFFFFFFFF], [3 * room], [3 * room + 3]])  # fabricated counts: no buffers behind them
    off = host.assign_triangle_offsets(_draws_of([0] * 12 + [1]), meshes)
    assert int(off[-1]) == (1 << 34) - 2  # the last name is 2^34 - 3, its id 2^34 - 2: below the id field's all-ones
    with pytest.raises(NvError, match="NV_EINVAL"):
        host.assign_triangle_offsets(_draws_of([0] * 12 + [2]), meshes)
    with pytest.raises(NvError, match="NV_EINVAL"):
        host.assign_triangle_offsets(_draws_of([0] * 13), meshes)


def test_word_order_is_depth_then_id_and_decode_inverts_encode():
    lo, hi = int(np.float32(0.25).view(np.uint32)), int(np.float32(0.5).view(np.uint32))
    assert VI.encode(hi, 0) > VI.encode(lo, VI.TRI34_END - 1)  # the nearer sample wins whatever the ids
    assert VI.encode(lo, 8) > VI.encode(lo, 7)                 # a tie in depth goes to the larger id
    assert VI.encode(0, 0) == 1                                # a sample at the far plane is still a sample
    for bits, tri in ((0, 0), (0x3F800000, VI.TRI34_END - 1), (lo, 1 << 33)):
        assert VI.decode(VI.encode(bits, tri)) == (bits, tri)


# ---- 3. the restated raster

def _soup(seed, viewport=(64, 48)):
    s = VI.triangle_soup(SIZES, seed)
    cd = host.build_cull_data(viewport=viewport, draw_count=len(SIZES))
    assert host.assign_triangle_offsets(s["draws"], s["meshes"]).tolist() == s["offsets"].tolist()
    return dict(s, cull=cd, viewport=viewport)


def _ix(s):
    return s["commands"], s["count"], s["draws"], s["indices"], s["vertices"]


@pytest.mark.parametrize("post_pass", [0, 1])
def test_restated_raster_keeps_the_depth_and_names_every_sample(post_pass, viref, cref):
    s = _soup(11)
    w, h = s["viewport"]
    g = RR.globals_for(s["cull"], (w, h), post_pass)
    for near_clip in (0, 1):
        d, v, tot = viref.raster(g, *_ix(s), w, h, s["offsets"], near_clip=near_clip)
        dr, tr = cref.indexed(near_clip).raster(g, *_ix(s), w, h)
        assert d.view(np.uint32).tobytes() == dr.view(np.uint32).tobytes() and tot.tolist() == tr.tolist()
        assert ((v >> np.uint64(34)).astype(np.uint32) == d.view(np.uint32))[v != 0].all()  # the word's depth is the depth
        ids = (v[v != 0] & np.uint64(VI.ID_MASK)) - np.uint64(1)
        assert len(ids) > w * h // 4 and ids.max() < s["offsets"][-1]
        seen = set(np.searchsorted(s["offsets"], ids, side="right") - 1)
        assert len(seen) >= 3  # several commands reach the target


def test_restated_raster_short_span_and_sliced_offsets(viref):
    s = _soup(12)
    w, h = s["viewport"]
    g = RR.globals_for(s["cull"], (w, h), 1)
    d, v, _ = viref.raster(g, *_ix(s), w, h, s["offsets"])
    # draw 4's span cut to 10 triangles: its other triangles write depth and no word; nothing else changes
    short = s["offsets"].copy()
    short[5] = short[4] + np.uint64(10)
    d2, v2, _ = viref.raster(g, *_ix(s), w, h, short)
    assert d2.tobytes() == d.tobytes()
    ids2 = (v2[v2 != 0] & np.uint64(VI.ID_MASK)) - np.uint64(1)
    assert ids2.max() < short[5] and (v2 != v).any()
    # a shard of draws [2, 5): rank-local drawIds, the offsets sliced at 2, the same words as the unsharded pass over those draws
    part = s["commands"][2:].copy()
    full = s["commands"].copy()
    full["instanceCount"][:2] = 0
    part["drawId"] -= 2
    da, va, _ = viref.raster(g, full, 5, s["draws"], s["indices"], s["vertices"], w, h, s["offsets"])
    db, vb, _ = viref.raster(g, part, 3, s["draws"][2:], s["indices"], s["vertices"], w, h, s["offsets"][2:])
    assert da.tobytes() == db.tobytes() and va.tobytes() == vb.tobytes() and (va != 0).any()


# ---- 4. the restated resolve inverts the restated raster

def _classic_commands(s, cd):
    """the oracle's drawcull (task = 0, the opaque passes) over every draw, everything visible: the commands of the classic path with the
    LODs it selects"""
    draws = s["draws"].copy()
    oracle.assign_visibility_offsets(draws, s["meshes"])
    pd = cd.copy()
    pd["postPass"] = 0
    co, c4 = np.zeros(len(draws) + 1, dtype=L.DRAWCMD), np.zeros(4, np.uint32)
    oracle.drawcull(pd, 0, 0, draws, s["meshes"], co, c4, np.ones(len(draws), np.uint32), None)
    return co[:len(draws)], int(c4[0])


def _check_inverse(viref, s, cd, post_pass):
    w, h = s["viewport"]
    offsets = host.assign_triangle_offsets(s["draws"], s["meshes"])
    commands, count = _classic_commands(s, cd)
    assert count > 0
    g = RR.globals_for(cd, (w, h), post_pass)
    _, vis, _ = viref.raster(g, commands, count, s["draws"], s["indices"], s["vertices"], w, h, offsets)
    out = viref.resolve(cd, vis, s["draws"], s["meshes"], offsets)
    rec, flat = out["records"], vis.reshape(-1)
    covered = flat != 0
    assert covered.sum() > w * h // 8 and out["totals"].tolist() == [int(covered.sum()), 0, 0, 0]
    assert rec[~covered].tobytes() == np.array([VI.NO_SAMPLE] * int((~covered).sum()), np.uint32).tobytes()
    by_draw = {int(c["drawId"]): c for c in commands[:count]}
    tri34 = (flat[covered] & np.uint64(VI.ID_MASK)) - np.uint64(1)
    r = rec[covered]
    d = np.searchsorted(offsets, tri34, side="right") - 1
    assert (r["drawId"] == d).all() and (r["depthBits"] == (flat[covered] >> np.uint64(34))).all()
    first = np.array([by_draw[int(k)]["firstIndex"] for k in d], np.uint64)
    vo = np.array([by_draw[int(k)]["vertexOffset"] for k in d], np.uint32)
    assert (r["indexPosition"] == first + np.uint64(3) * (tri34 - offsets[d])).all() and (r["vertexOffset"] == vo).all()
    assert out["draw_pixels"].tolist() == np.bincount(d, minlength=len(s["draws"])).tolist()
    return commands[:count]


@pytest.mark.parametrize("post_pass", [0, 1])
def test_resolve_inverts_the_raster_on_the_occluder_scene(post_pass, viref):
    s = synth.occluder_scene_indexed(meshlet_bounds=oracle.meshlet_bounds)
    cd = s["cull"].copy()
    cd["cullingEnabled"] = 0
    _check_inverse(viref, s, cd, post_pass)


def two_lod_scene(viewport=(64, 48)):
    """triangle_soup's draws over meshes of two LODs: LOD 1 is every second triangle of LOD 0, in an index range of its own, selected beyond
    a view distance of 9"""
    s = VI.triangle_soup(SIZES, 13)
    cd = host.build_cull_data(viewport=viewport, draw_count=len(SIZES), lodEnabled=1)
    cd["cullingEnabled"] = 0
    ind, extra = s["indices"], []
    at = len(ind)
    for i, k in enumerate(SIZES):
        m = s["meshes"][i]
        first = int(m["lods"]["indexOffset"][0])
        half = ind[first:first + 3 * k].reshape(-1, 3)[::2].reshape(-1)
        m["lodCount"], m["radius"] = 2, 0.0
        m["lods"]["indexOffset"][1], m["lods"]["indexCount"][1], m["lods"]["error"][1] = at, len(half), 9.0 * float(cd["lodTarget"][0])
        extra.append(half)
        at += len(half)
    s["draws"]["position"][:, 2] = [-5.0, -13.0, -6.0, -12.0, -11.0]
    return dict(s, indices=np.concatenate([ind] + extra), cull=cd, viewport=viewport)


@pytest.mark.parametrize("lod_enabled", [0, 1])
def test_resolve_inverts_the_raster_over_two_lods(lod_enabled, viref):
    s = two_lod_scene()
    cd = s["cull"].copy()
    cd["lodEnabled"] = lod_enabled
    commands = _check_inverse(viref, s, cd, 1)
    lod1 = [int(c["firstIndex"]) >= 3 * sum(SIZES) for c in commands]
    assert lod1 == ([False, True, False, True, True] if lod_enabled else [False] * 5)


def test_resolve_reference_marks_hand_made_words_unresolved(viref):
    s = _soup(14)
    off = s["offsets"]
    total = int(off[-1])
    words = np.array([0, VI.encode(5, 0), VI.encode(5, total - 1), VI.encode(5, total), 7 << 34, VI.encode(0, int(off[2]))], np.uint64)
    out = viref.resolve(s["cull"], words, s["draws"], s["meshes"], off)
    r = [tuple(int(x) for x in rec) for rec in out["records"]]
    assert r[0] == VI.NO_SAMPLE and r[1] == (0, 0, 0, 5) and r[2][0] == 4 and r[3] == VI.UNRESOLVED and r[4] == VI.UNRESOLVED
    assert r[5] == (2, 3 * int(off[2]), 0, 0) and out["totals"].tolist() == [5, 2, 0, 0]
    # a mesh index past the table, a LOD shorter than the span, an index position past 32 bits
    draws, meshes = s["draws"].copy(), s["meshes"].copy()
    draws[0]["meshIndex"] = 99
    meshes[1]["lods"]["indexCount"][0] = 3 * 10
    meshes[3]["lods"]["indexOffset"][0] = 0xFFFFFFFF - 3
    words = np.array([VI.encode(1, 0), VI.encode(1, int(off[1]) + 9), VI.encode(1, int(off[1]) + 10), VI.encode(1, int(off[3])),
                      VI.encode(1, int(off[3]) + 1)], np.uint64)
    out = viref.resolve(s["cull"], words, draws, meshes, off)
    r = [tuple(int(x) for x in rec) for rec in out["records"]]
    assert r[0] == VI.UNRESOLVED and r[1][0] == 1 and r[2] == VI.UNRESOLVED and r[3] == (3, 0xFFFFFFFF - 3, 0, 1) and r[4] == VI.UNRESOLVED
    assert out["totals"].tolist() == [5, 3, 0, 0] and out["draw_pixels"].tolist() == [0, 1, 0, 1, 0]


# ---- 5. the attribute restatement

@pytest.fixture(scope="session")
def aref(tmp_path_factory):
    import visattr_ref as VA
    return VA.load(tmp_path_factory.mktemp("visattr_ref_vi"))


@pytest.fixture(scope="session")
def iaref(tmp_path_factory):
    import visattr_indexed_ref as VAI
    return VAI.load(tmp_path_factory.mktemp("visattr_indexed_ref"))


def occluder_with_attributes():
    import visattr_ref as VA
    return VA.with_attributes(synth.occluder_scene_indexed(meshlet_bounds=oracle.meshlet_bounds))


def order_condition(s):
    """The condition under which the cluster path's ids and the indexed path's are order-isomorphic on a scene: every mesh has one LOD and
    indexed_geometry skipped none of its meshlets' triangles, so triangle t of a draw is the t-th triangle of its meshlets in order and
    (draw, meshlet, triangle) increases with both ids.  Returns per mesh the running triangle count at each of its meshlets (the map)."""
    meshes, meshlets = s["meshes"], s["meshlets"]
    starts = []
    for m in meshes:
        assert int(m["lodCount"]) == 1
        first, count = int(m["lods"]["meshletOffset"][0]), int(m["lods"]["meshletCount"][0])
        tc = np.minimum(meshlets["triangleCount"][first:first + count].astype(np.int64), 96)
        run = np.concatenate([[0], np.cumsum(tc)])
        assert int(run[-1]) == int(m["lods"]["indexCount"][0]) // 3 and (tc > 0).all()  # no skipped triangle, no empty meshlet
        starts.append(run)
    draws = s["draws"].copy()
    oracle.assign_visibility_offsets(draws, meshes)
    off = host.assign_triangle_offsets(draws, meshes)
    assert (np.diff(draws["meshletVisibilityOffset"].astype(np.int64)) > 0).all() and (np.diff(off.astype(np.int64)) > 0).all()
    return starts


def meshlet_records(s, records, starts):
    """the NvVisRecords that name the triangles `records` (VISINDEXEDRECORD) name: the map is the running triangle count"""
    out = np.zeros(len(records), dtype=L.VISRECORD)
    out["drawId"], out["depthBits"] = records["drawId"], records["depthBits"]
    for i in np.nonzero(records["drawId"] != 0xFFFFFFFF)[0]:
        mesh = int(s["draws"][int(records[i]["drawId"])]["meshIndex"])
        m = s["meshes"][mesh]
        t = (int(records[i]["indexPosition"]) - int(m["lods"]["indexOffset"][0])) // 3
        k = int(np.searchsorted(starts[mesh], t, side="right")) - 1
        out[i]["meshletIndex"], out[i]["triangle"] = int(m["lods"]["meshletOffset"][0]) + k, t - int(starts[mesh][k])
    return out


def classic_records(s, viref, post_pass=0):
    """the restated chain over every draw of the scene (culling off): (visibility, resolve dict, offsets, commands, count)"""
    cd = s["cull"].copy()
    cd["cullingEnabled"] = 0
    w, h = s["viewport"]
    offsets = host.assign_triangle_offsets(s["draws"], s["meshes"])
    commands, count = _classic_commands(s, cd)
    g = RR.globals_for(cd, (w, h), post_pass)
    _, vis, _ = viref.raster(g, commands, count, s["draws"], s["indices"], s["vertices"], w, h, offsets)
    return vis, viref.resolve(cd, vis, s["draws"], s["meshes"], offsets), offsets, commands, count


def all_clusters(s):
    """every meshlet of every draw of a one-LOD scene as the cluster path's inputs: (draws with their offsets, task commands, cib, cc4)"""
    draws = s["draws"].copy()
    oracle.assign_visibility_offsets(draws, s["meshes"])
    cmds, ids = [], []
    for d in range(len(draws)):
        lod = s["meshes"]["lods"][int(draws[d]["meshIndex"]), 0]
        for k in range(0, int(lod["meshletCount"]), 64):
            n = min(64, int(lod["meshletCount"]) - k)
            ids += [len(cmds) | j << 24 for j in range(n)]
            cmds.append((d, int(lod["meshletOffset"]) + k, n, 1, int(draws[d]["meshletVisibilityOffset"]) + k))
    cc4 = np.array([len(ids), 0, 0, 0], np.uint32)
    cib = np.concatenate([np.array(ids, np.uint32), np.zeros(512, np.uint32)])
    oracle.clustersubmit(cc4, cib)
    return draws, np.array(cmds, dtype=L.TASKCMD), cib, cc4


@pytest.mark.parametrize("post_pass", [0, 1])
def test_order_condition_holds_on_the_two_restatements(post_pass, viref, tmp_path_factory):
    """occluder_scene_indexed: the structural half (order_condition), and on the two restated rasters over all draws the same depth bits
    and, through the map, the same triangle at every pixel — so ties fall on the same triangle and the two chains can be compared bit for bit"""
    import visbuffer_ref as VB
    vref = VB.load(tmp_path_factory.mktemp("visbuffer_ref_vi"))
    s = occluder_with_attributes()
    starts = order_condition(s)
    w, h = s["viewport"]
    cd = s["cull"].copy()
    cd["cullingEnabled"] = 0
    g = RR.globals_for(cd, (w, h), post_pass)
    offsets = host.assign_triangle_offsets(s["draws"], s["meshes"])
    commands, count = _classic_commands(s, cd)
    di, vi, ti = viref.raster(g, commands, count, s["draws"], s["indices"], s["vertices"], w, h, offsets)
    draws, tasks, cib, cc4 = all_clusters(s)
    dc, vc, tc = vref.raster(g, tasks, draws, s["meshlets"], s["data"], s["vertices"], cib, cc4, w, h)
    assert di.view(np.uint32).tobytes() == dc.view(np.uint32).tobytes() and ti[2:].tolist() == tc[2:].tolist() and (di != 0).sum() > w * h // 4
    ri = viref.resolve(cd, vi, s["draws"], s["meshes"], offsets)["records"]
    mvb_words = (int(draws["meshletVisibilityOffset"][-1]) + 4096 + 31) // 32
    rc = vref.resolve(cd, vc, draws, s["meshes"], mvb_words)["records"]
    assert meshlet_records(s, ri, starts).tobytes() == rc.tobytes()


def test_indexed_attributes_equal_the_meshlet_attributes_of_the_same_triangles(viref, aref, iaref):
    s = occluder_with_attributes()
    starts = order_condition(s)
    w, h = s["viewport"]
    rec = classic_records(s, viref)[1]["records"]
    g = RR.globals_for(s["cull"], (w, h))
    for mats in (s["materials"], None):
        for real in ("f32", "f64"):
            a = iaref.attributes(g, rec, w, h, s["draws"], s["indices"], s["vertices"], mats, real=real)
            b = aref.attributes(g, meshlet_records(s, rec, starts), w, h, s["draws"], s["meshlets"], s["data"], s["vertices"], mats, real=real)
            for k in ("vals", "ids", "gbuffer0", "gbuffer1", "totals", "flags", "chan"):
                assert a[k].tobytes() == b[k].tobytes(), (k, real)
    assert a["totals"][0] > w * h // 4 and a["totals"][1] == 0


def test_indexed_attribute_reference_counts_invalid_records(iaref):
    s = occluder_with_attributes()
    w, h = 8, 1
    g = RR.globals_for(host.build_cull_data(viewport=(w, h)), (w, h))
    ni, nv, nd = len(s["indices"]), len(s["vertices"]), len(s["draws"])
    rec = np.zeros(8, dtype=L.VISINDEXEDRECORD)
    rec["drawId"] = [0, nd, 0, 0, 0, 0xFFFFFFFF, 0xFFFFFFFF, 1]
    rec["indexPosition"] = [0, 0, ni - 3, ni - 2, 0xFFFFFFFE, 0, 0xFFFFFFFF, 3]
    rec["vertexOffset"] = [0, 0, 0, 0, 0, 0, 0xFFFFFFFF, nv]  # the last one: every corner past the vertices
    rec["depthBits"][6] = 0xFFFFFFFF
    out = iaref.attributes(g, rec, w, h, s["draws"], s["indices"], s["vertices"], s["materials"])
    assert out["totals"][:2].tolist() == [2, 4] and out["flags"].tolist()[:2] == [out["flags"][0], 2]
    assert [int(f) & 3 for f in out["flags"]] == [1, 2, 1, 2, 2, 0, 0, 2]
    draws = s["draws"].copy()
    draws["materialIndex"][0] = len(s["materials"])
    out = iaref.attributes(g, rec, w, h, draws, s["indices"], s["vertices"], s["materials"])
    assert [int(f) & 3 for f in out["flags"]] == [2, 2, 2, 2, 2, 0, 0, 2]
    out = iaref.attributes(g, rec, w, h, draws, s["indices"], s["vertices"], None)  # no table: the material index is not checked
    assert [int(f) & 3 for f in out["flags"]] == [1, 2, 1, 2, 2, 0, 0, 2]
