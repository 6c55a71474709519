"""The frame-stable visibility buffer on the CPU: the ABI, the word's order and round trip, list independence of the
stable form (false for the slot form), the resolve reference against a decode that never evaluates a LOD, and the composite of two gloo
ranks through shard.composite_visibility."""
import ctypes as C
import os
import pickle
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import niagara_amd as N
import oracle
import raster_ref as RR
import sharded_ref as SR
import visbuffer_ref as VB
from niagara_amd import host, shard, synth
from niagara_amd import layouts as L
from scenes import make_scene, make_triangle_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="session")
def vref(tmp_path_factory):
    return VB.load(tmp_path_factory.mktemp("visbuffer_ref"))


@pytest.fixture(scope="session")
def rref(tmp_path_factory):
    return RR.load(tmp_path_factory.mktemp("raster_ref_vis"))


# ---- 1. ABI

def test_abi_has_the_symbols_the_option_and_the_record(tmp_path):
    import subprocess
    from niagara_amd import pipeline as P
    for name in ("nv_visibility_resolve", "nv_visibility_merge", "nv_rasterdepth"):
        assert name in N.EXPORTS and hasattr(N.lib, name)
    header = open(os.path.join(ROOT, "include", "niagara_vis.h")).read()
    assert re.search(r"^#define NV_OPT_RASTER_VISIBILITY_ID 11$", header, flags=re.M) and P.NV_OPT_RASTER_VISIBILITY_ID == 11
    src = tmp_path / "t.c"
    src.write_text('#include "niagara_vis.h"\nint main(void){NvVisRecord r; return sizeof(r)==16 && sizeof(r.drawId)==4 && NV_OPT_RASTER_VISIBILITY_ID==11?0:1;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "c")])
    subprocess.check_call([str(tmp_path / "c")])
    assert L.VISRECORD.itemsize == 16 and L.VISRECORD.names == ("drawId", "meshletIndex", "triangle", "depthBits")


# ---- 2. the word

def _bits(z):
    return int(np.float32(z).view(np.uint32))


def test_word_order_is_depth_then_id_and_decode_inverts_encode():
    rng = np.random.default_rng(1)
    special = [0.0, 1.0, 1e-45, 1e-40, 1.1754942e-38, 1.17549435e-38, 0.5, np.nextafter(np.float32(1.0), np.float32(0.0))]
    zs = [_bits(z) for z in special] + [_bits(z) for z in rng.random(200).astype(np.float32)]
    assert VB.encode(_bits(1.0), VB.MVI_END - 1, 127) < 1 << 64 and _bits(1.0) == 0x3F800000 and _bits(1.0) < 1 << 30
    assert VB.encode(_bits(1.0), 0, 0) >> 63 == 1  # bit 63 can be set: the composite must be unsigned
    assert VB.encode(0, 0, 0) == 1  # 0 stays "no sample"
    for _ in range(4000):
        a = (int(rng.choice(zs)), int(rng.choice([0, 1, 5, 1 << 20, VB.MVI_END - 1, int(rng.integers(0, VB.MVI_END))])), int(rng.integers(0, 128)))
        b = (int(rng.choice(zs)), int(rng.choice([0, 1, 5, 1 << 20, VB.MVI_END - 1, int(rng.integers(0, VB.MVI_END))])), int(rng.integers(0, 128)))
        wa, wb = VB.encode(*a), VB.encode(*b)
        assert (wa < wb) == (a < b) and (wa == wb) == (a == b)  # tuple order: depth bits, then mvi, then triangle
        assert VB.decode(wa) == a and 0 < wa < 1 << 64
    # the order of positive floats is the order of their bits, denormals included
    fl = np.sort(np.array(special, np.float32))
    assert (np.diff(fl.view(np.uint32).astype(np.int64)) > 0).all()


def _split_lists(s, cib, cc4, rng):
    """the cluster list cut into two disjoint lists (random halves), each padded by clustersubmit"""
    ids = cib[:int(cc4[0])]
    pick = rng.random(len(ids)) < 0.5
    out = []
    for part in (ids[pick], ids[~pick]):
        c4 = np.array([len(part), 0, 0, 0], np.uint32)
        cb = np.concatenate([part, np.zeros(512, np.uint32)])
        oracle.clustersubmit(c4, cb)
        out.append((cb, c4))
    return out


def _cluster_list(s):
    cd = s["cull"].copy()
    cd["clusterBackfaceEnabled"], cd["cullingEnabled"] = 0, 1
    cib, cc4 = np.zeros(s["n"] * 64 + 256, np.uint32), np.zeros(4, np.uint32)
    oracle.clustercull(cd, 0, s["commands"], s["count4"], s["draws"], s["meshlets"], None, None, cib, cc4)
    oracle.clustersubmit(cc4, cib)
    return cib, cc4


@pytest.mark.parametrize("near_clip", [0, 1])
def test_stable_words_do_not_depend_on_the_list_and_slot_words_do(vref, rref, near_clip):
    s = make_triangle_scene(seed=41, n_draws=200, commands_per_draw=3, scene_radius=6.0, viewport=(333, 207))
    cib, cc4 = _cluster_list(s)
    w, h = s["viewport"]
    common = (s["globals"], s["commands"], s["draws"], s["meshlets"], s["data"], s["vertices"])
    d1, v1, t1 = vref.raster(*common, cib, cc4, w, h, near_clip=near_clip)
    (ca, c4a), (cb, c4b) = _split_lists(s, cib, cc4, np.random.default_rng(2))
    d2, v2, ta = vref.raster(*common, ca, c4a, w, h, near_clip=near_clip)
    d2, v2, tb = vref.raster(*common, cb, c4b, w, h, depth=d2, vis=v2, near_clip=near_clip)
    assert v1.tobytes() == v2.tobytes() and d1.tobytes() == d2.tobytes() and (ta + tb).tolist() == t1.tolist()
    assert (v1 != 0).sum() > 1000
    # the depth does not depend on the form, and the word carries it
    if near_clip == 0:
        ds, vs, ts = rref.raster(*common, cib, cc4, w, h, visibility=True)
        assert ds.tobytes() == d1.tobytes() and ts.tolist() == t1.tolist()
        assert ((vs >> np.uint64(32)) == (v1 >> np.uint64(VB.SHIFT))).all()
        # the slot form of the same two lists into one target is NOT the one-list target: its ids are positions in the list
        _, sa, _ = rref.raster(*common, ca, c4a, w, h, visibility=True)
        _, sb, _ = rref.raster(*common, cb, c4b, w, h, visibility=True)
        assert np.maximum(sa, sb).tobytes() != vs.tobytes()
    assert ((v1[v1 != 0] >> np.uint64(VB.SHIFT)).astype(np.uint32) == d1.view(np.uint32)[v1 != 0]).all()


def test_a_cluster_past_the_id_range_writes_depth_and_no_word(vref):
    s = make_triangle_scene(seed=42, n_draws=20, commands_per_draw=1, scene_radius=6.0, viewport=(160, 120))
    cib, cc4 = _cluster_list(s)
    co = s["commands"].copy()
    co["meshletVisibilityOffset"][::2] = VB.MVI_END - 3  # lanes 0-2 still fit, lanes >= 3 do not
    common = (s["globals"], co, s["draws"], s["meshlets"], s["data"], s["vertices"])
    d, v, _ = vref.raster(*common, cib, cc4, 160, 120)
    d0, v0, _ = vref.raster(s["globals"], s["commands"], *common[2:], cib, cc4, 160, 120)
    assert d.tobytes() == d0.tobytes() and (v != 0).sum() < (v0 != 0).sum()
    mvi = ((v[v != 0] & np.uint64(VB.ID_MASK)).astype(np.int64) - 1) >> 7
    assert mvi.max() == VB.MVI_END - 1 and (mvi < VB.MVI_END).all()


# ---- 3. the resolve reference against the frame's own command lists

def _lod_scene():
    """tests/test_raster_gpu.py's make_scene frame (four LODs, several of them in view) plus draws of a mesh without meshlets"""
    sc = make_scene(seed=5, n_draws=300, viewport=(256, 192))
    meshes = np.concatenate([sc["meshes"], np.zeros(1, L.MESH)])
    meshes[-1]["lodCount"], meshes[-1]["radius"] = 1, 1.0
    draws = sc["draws"].copy()
    draws["meshIndex"][[3, 4, 50, 51, 52, 299]] = len(meshes) - 1
    host.assign_visibility_offsets(draws, meshes)
    data, vertices = synth.make_geometry(sc["meshlets"], seed=6)
    cd = sc["cull"].copy()
    cd["occlusionEnabled"], cd["clusterOcclusionEnabled"], cd["clusterBackfaceEnabled"] = 1, 1, 1
    return dict(meshes=meshes, meshlets=sc["meshlets"], draws=draws, data=data, vertices=vertices, cull=cd, viewport=sc["viewport"])


SCENES = {"lods": (_lod_scene, 0), "occluder": (lambda: synth.occluder_scene(meshlet_bounds=oracle.meshlet_bounds), 0),
          "interior": (lambda: synth.interior_scene(meshlet_bounds=oracle.meshlet_bounds), 1)}


def _mvb_words(draws, meshes):
    slots, _ = oracle.assign_visibility_offsets(draws.copy(), meshes)
    return max(1, (slots + 31) // 32 + 2)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_resolve_reference_equals_the_decode_by_command_lists(vref, name):
    make, near_clip = SCENES[name]
    s = make()
    frames = VB.oracle_frames(s, 2, True, vref, near_clip)
    for rec in frames:
        vis, draws = rec["visibility"], rec["draws"]
        got = vref.resolve(s["cull"], vis, draws, s["meshes"], _mvb_words(draws, s["meshes"]))
        want = VB.decode_by_commands(vis, VB.frame_commands(rec, True))
        assert got["records"].tobytes() == want.tobytes()
        covered = int((vis != 0).sum())
        assert got["totals"].tolist() == [covered, 0, 0, 0] and covered > vis.size // 20  # unresolved = 0: a condition of the GPU test
        assert ((vis[vis != 0] >> np.uint64(VB.SHIFT)).astype(np.uint32) == rec["post"]["depth"].view(np.uint32)[vis != 0]).all()
        mvi = ((vis[vis != 0] & np.uint64(VB.ID_MASK)).astype(np.int64) - 1) >> 7
        assert mvi.max() < VB.MVI_END // 1000  # far below 2^27
        # d_meshletSeen names rasterised clusters only; d_drawPixels counts the records
        seen = {int(w) * 32 + b for w in np.nonzero(got["seen"])[0] for b in range(32) if got["seen"][w] >> b & 1}
        assert seen == set(np.unique(mvi).tolist()) and seen <= VB.rasterised_clusters(rec, True)
        r = got["records"].reshape(-1)
        ok = r["drawId"] != 0xFFFFFFFF
        assert np.bincount(r["drawId"][ok], minlength=len(draws)).tolist() == got["draw_pixels"].tolist()
    if name == "lods":
        m = s["meshes"][frames[0]["draws"]["meshIndex"][r["drawId"][ok]]]
        rel = r["meshletIndex"][ok][:, None] - m["lods"]["meshletOffset"]
        lod = ((rel >= 0) & (rel < m["lods"]["meshletCount"])).argmax(axis=1)
        assert len(np.unique(lod)) >= 2, "one LOD only in view"
    if name == "occluder":  # the wall's pixels resolve to the wall
        wall = s["wall"] if isinstance(s["wall"], (list, tuple)) else [s["wall"]]
        assert np.isin(r["drawId"][ok], wall).sum() > ok.sum() // 2


def test_resolve_reference_marks_hand_made_words_unresolved(vref):
    s = _lod_scene()
    draws, meshes = s["draws"], s["meshes"]
    words_all = _mvb_words(draws, meshes)
    far = np.linalg.norm(draws["position"], axis=1)
    far[draws["meshIndex"] == len(meshes) - 1] = 0
    d = int(far.argmax())  # far from the camera: its LOD threshold is not 0
    off, mesh = int(draws["meshletVisibilityOffset"][d]), meshes[draws["meshIndex"][d]]
    cd = s["cull"].copy()
    cd["lodEnabled"] = 0
    n0 = int(mesh["lods"][0]["meshletCount"])
    last = len(draws) - 1  # draw 299 has no meshlets: an mvi at or past its offset names nothing
    bad_mesh = draws.copy()
    vis = np.array([0,
                    VB.encode(5, off, 0), VB.encode(5, off + n0 - 1, 95),           # resolved
                    VB.encode(5, off, 96), VB.encode(5, off, 127),                  # triangle >= 96
                    VB.encode(5, int(draws["meshletVisibilityOffset"][last]), 0),   # past the last meshlet of the scene
                    VB.encode(5, VB.MVI_END - 1, 0),
                    5 << VB.SHIFT,                                                   # depth without an id
                    VB.encode(0x3F800000, off + 1, 3)], np.uint64)
    got = vref.resolve(cd, vis, draws, meshes, words_all)
    r = got["records"]
    assert tuple(r[0]) == VB.NO_SAMPLE
    assert tuple(r[1]) == (d, int(mesh["lods"][0]["meshletOffset"]), 0, 5) and tuple(r[2]) == (d, int(mesh["lods"][0]["meshletOffset"]) + n0 - 1, 95, 5)
    assert all(tuple(r[k]) == VB.UNRESOLVED for k in (3, 4, 5, 6, 7))
    assert tuple(r[8]) == (d, int(mesh["lods"][0]["meshletOffset"]) + 1, 3, 0x3F800000)
    assert got["totals"].tolist() == [8, 5, 0, 0] and got["draw_pixels"][d] == 3 and got["draw_pixels"].sum() == 3
    # a LOD with fewer meshlets than the index, and a mesh index past the table
    cd1 = s["cull"].copy()
    cd1["lodEnabled"], cd1["lodTarget"] = 1, 1e9  # every error is below the threshold: the last LOD
    lastlod = int(mesh["lodCount"]) - 1
    nl = int(mesh["lods"][lastlod]["meshletCount"])
    assert nl < n0
    g2 = vref.resolve(cd1, np.array([VB.encode(5, off + nl, 0), VB.encode(5, off + nl - 1, 0)], np.uint64), draws, meshes, words_all)
    assert tuple(g2["records"][0]) == VB.UNRESOLVED and tuple(g2["records"][1]) == (d, int(mesh["lods"][lastlod]["meshletOffset"]) + nl - 1, 0, 5)
    bad_mesh["meshIndex"][d] = len(meshes)
    g3 = vref.resolve(cd, vis[1:2], bad_mesh, meshes, words_all)
    assert tuple(g3["records"][0]) == VB.UNRESOLVED and g3["totals"].tolist() == [1, 1, 0, 0]
    g4 = vref.resolve(cd, vis[1:2], draws[:0], meshes, words_all)
    assert tuple(g4["records"][0]) == VB.UNRESOLVED


# ---- 4. two gloo ranks

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    s = synth.occluder_scene(meshlet_bounds=oracle.meshlet_bounds)
    draws = s["draws"].copy()
    oracle.assign_visibility_offsets(draws, s["meshes"])
    b, e = shard.draw_ranges(draws, s["meshes"], world, "draws")[rank]
    fr = VB.load(out_dir).frame_raster(0)
    me = SR.OracleRank(s, b, e, fr)
    out = []
    for _ in range(2):
        for name in SR.phase_names(True):
            me.phase(name)
            shard.composite_depth(torch.from_numpy(me.depth), True)
            shard.composite_visibility(torch.from_numpy(fr.vis.view(np.int64)), True)  # in place: the frame's target on every rank
        out.append(fr.vis.copy())
    # a word with bit 63 set against one without: the unsigned maximum keeps it
    t = torch.from_numpy(np.array([VB.encode(0x3F800000, 3, 1) if rank == 0 else VB.encode(0x3F7FFFFF, 9, 2), 0, rank + 1], np.uint64).view(np.int64))
    shard.composite_visibility(t, True)
    with open(os.path.join(out_dir, "rank_%d.pkl" % rank), "wb") as f:
        pickle.dump((out, t.numpy().view(np.uint64)), f)
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_composite_to_the_unsharded_buffer(tmp_path, vref):
    world = 2
    VB.load(tmp_path)  # compiled once, before the ranks load it
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    s = synth.occluder_scene(meshlet_bounds=oracle.meshlet_bounds)
    want = VB.oracle_frames(s, 2, True, vref, 0)
    for r in range(world):
        got, words = pickle.load(open(tmp_path / ("rank_%d.pkl" % r), "rb"))
        for f in range(2):
            assert got[f].tobytes() == want[f]["visibility"].tobytes(), (r, f)
        assert words.tolist() == [VB.encode(0x3F800000, 3, 1), 0, 2] and int(words[0]) >> 63 == 1
    assert (want[1]["visibility"] != 0).sum() > 1000
    ranges = shard.draw_ranges(want[0]["draws"], s["meshes"], world, "draws")
    ids = vref.resolve(s["cull"], want[1]["visibility"], want[1]["draws"], s["meshes"], _mvb_words(want[1]["draws"], s["meshes"]))["records"]["drawId"]
    ids = ids[ids != 0xFFFFFFFF]
    assert all(((ids >= b) & (ids < e)).any() for b, e in ranges), "one rank owns every visible pixel"


def test_composite_visibility_without_a_group_is_a_no_op():
    v = torch.from_numpy(np.array([VB.encode(0x3F800000, 1, 1), 0], np.uint64).view(np.int64))
    assert shard.composite_visibility(v.clone()).equal(v)
