"""The frame sharded by draw ranges on the CPU: world size 2 over gloo, the oracle's passes and the reference raster
standing in for the device on each rank's range, the depth composite through shard.composite_depth (all_reduce MAX), the outputs stitched
with shard's helpers and compared with the oracle's unsharded frame; plus the unit tests of draw_ranges and the rebase helpers."""
import os
import pickle
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import oracle
import raster_clip_ref as RC
import raster_ref as RR
import sharded_ref as SR
from niagara_amd import host, shard, synth
from niagara_amd import layouts as L

FRAMES = 2


@pytest.fixture(scope="session")
def rref(tmp_path_factory):
    return RR.load(tmp_path_factory.mktemp("raster_ref_sharded"))


def _scene():
    return synth.occluder_scene(meshlet_bounds=oracle.meshlet_bounds)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, out_dir, post_pass, weight):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    s = _scene()
    draws = s["draws"].copy()
    oracle.assign_visibility_offsets(draws, s["meshes"])
    b, e = shard.draw_ranges(draws, s["meshes"], world, weight)[rank]
    me = SR.OracleRank(s, b, e, RR.load(out_dir))
    out = []
    for _ in range(FRAMES):
        rec = {}
        for name in SR.phase_names(post_pass):
            rec[name] = me.phase(name)
            shard.composite_depth(torch.from_numpy(me.depth), True)  # in place: the rank's target becomes the frame's
            counts = torch.tensor([int(rec[name]["count4"][0]), int(rec[name]["count4"][1]), int(rec[name]["cc4"][0])], dtype=torch.int64)
            rec[name]["counts"] = shard.allreduce_counts(counts).numpy()
            rec[name]["depth"] = me.depth.copy()
        rec["pyramid"] = me.pyr.data.copy()
        out.append(rec)
    with open(os.path.join(out_dir, "rank_%d.pkl" % rank), "wb") as f:
        pickle.dump(out, f)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("weight", ["draws", "meshlets"])
def test_two_gloo_ranks_stitch_to_the_unsharded_oracle_frame(tmp_path, rref, weight):
    """both cull phases (and the post phase) of two consecutive frames: frame 2's early pass consumes frame 1's visibility state, its late
    pass the composite of both ranks' depth"""
    world, post_pass = 2, True
    RR.load(tmp_path)  # compiled once, before the ranks load it
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), post_pass, weight), nprocs=world, join=True)
    s = _scene()
    want = RR.oracle_frames(s, FRAMES, post_pass=post_pass, rref=rref)
    ranges = shard.draw_ranges(want[0]["draws"], s["meshes"], world, weight)
    got = [pickle.load(open(tmp_path / ("rank_%d.pkl" % r), "rb")) for r in range(world)]
    for f in range(FRAMES):
        for r in range(world):
            assert got[r][f]["pyramid"].tobytes() == want[f]["pyramid"].tobytes(), (f, r)
        for name in SR.phase_names(post_pass):
            parts = [got[r][f][name] for r in range(world)]
            st = SR.stitched(parts, ranges)
            for r in range(world):  # after the composite every rank holds the unsharded target
                SR.same_phase(dict(st, depth=parts[r]["depth"]), want[f][name])
                assert parts[r]["counts"].tolist() == [int(want[f][name]["count4"][0]), sum(int(p["count4"][1]) for p in parts), int(want[f][name]["cc4"][0])]
    SR.assert_not_vacuous(s, ranges, want, [got[r][1]["early"]["samples"] for r in range(world)])


@pytest.fixture(scope="session")
def clip_rref(tmp_path_factory):
    return RC.load(tmp_path_factory.mktemp("raster_clip_ref_sharded")).cluster(1)


@pytest.mark.parametrize("weight", ["draws", "meshlets"])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("name", ["occluder", "interior"])
def test_lockstep_shards_equal_the_unsharded_oracle_frame(rref, clip_rref, name, world, weight):
    """the scenes and world sizes of the GPU test, checked on the CPU: equality, and the conditions that make it mean something (the
    interior scene with the near-plane clipping reference: its surfaces occlude only when clipped)"""
    s = _scene() if name == "occluder" else synth.interior_scene(meshlet_bounds=oracle.meshlet_bounds)
    rref = rref if name == "occluder" else clip_rref
    want = RR.oracle_frames(s, FRAMES, post_pass=True, rref=rref)
    ranges = shard.draw_ranges(want[0]["draws"], s["meshes"], world, weight)
    got = SR.lockstep_frames(s, ranges, FRAMES, True, rref)
    for f in range(FRAMES):
        for name in SR.phase_names(True):
            SR.same_phase(got[f][name], want[f][name])
        for p in got[f]["pyramids"]:
            assert p.tobytes() == want[f]["pyramid"].tobytes()
    rejected = SR.assert_not_vacuous(s, ranges, want, got[1]["early"]["samples"])
    assert set(rejected) == set(s["hidden"])  # the README's 8 hidden boxes; the interior scene's 4 below + 4 behind


def test_a_frame_without_the_composite_differs(rref):
    """the negative control: with every rank keeping its own depth the boxes behind the wall stay visible on the ranks that do not own it"""
    s = _scene()
    want = RR.oracle_frames(s, FRAMES, post_pass=False, rref=rref)
    ranges = shard.draw_ranges(want[0]["draws"], s["meshes"], 2, "draws")
    got = SR.lockstep_frames(s, ranges, FRAMES, False, rref, composite=False)
    assert got[1]["late"]["dvb"].tobytes() != want[1]["late"]["dvb"].tobytes()
    with pytest.raises(AssertionError):
        SR.same_phase(got[1]["late"], want[1]["late"])


# ---- draw_ranges

def _random_scene(n_draws, n_meshes, seed):
    rng = np.random.default_rng(seed)
    meshes = np.zeros(n_meshes, dtype=L.MESH)
    meshes["lodCount"] = rng.integers(1, 4, n_meshes)
    meshes["lods"]["meshletCount"] = rng.integers(1, 400, meshes["lods"]["meshletCount"].shape)
    draws = np.zeros(n_draws, dtype=L.MESHDRAW)
    draws["meshIndex"] = rng.integers(0, n_meshes, n_draws)
    return draws, meshes


@pytest.mark.parametrize("weight", ["draws", "meshlets"])
def test_draw_ranges_are_contiguous_and_cover(weight):
    for n, world, seed in [(0, 1, 1), (1, 1, 2), (13, 2, 3), (13, 8, 4), (1000, 3, 5), (1000, 8, 6), (5, 8, 7), (64, 64, 8)]:
        draws, meshes = _random_scene(n, 5, seed)
        r = shard.draw_ranges(draws, meshes, world, weight)
        assert len(r) == world and r[0][0] == 0 and r[-1][1] == n
        assert all(r[k][1] == r[k + 1][0] for k in range(world - 1)) and all(b <= e for b, e in r)
        if n >= world:
            assert all(e > b for b, e in r)
        else:  # world > draws: every draw still has exactly one owner, the other ranks are idle
            assert sum(e - b for b, e in r) == n and sum(1 for b, e in r if e > b) <= n


def test_draw_ranges_by_draws_are_nv_shard_range():
    draws, meshes = _random_scene(1001, 4, 9)
    assert shard.draw_ranges(draws, meshes, 8) == [tuple(host.shard_range(1001, r, 8)) for r in range(8)]


def test_draw_ranges_by_meshlets_are_within_one_draw_of_the_ideal_split():
    for seed, world in [(10, 2), (11, 3), (12, 8)]:
        draws, meshes = _random_scene(2000, 6, seed)
        w = shard.draw_weights(draws, meshes)
        valid = np.arange(meshes["lods"]["meshletCount"].shape[1])[None, :] < meshes["lodCount"][:, None]
        assert (w == np.where(valid, meshes["lods"]["meshletCount"], 0).max(axis=1)[draws["meshIndex"]]).all()
        prefix = np.concatenate([[0], np.cumsum(w)])
        r = shard.draw_ranges(draws, meshes, world, "meshlets")
        for k in range(1, world):
            assert abs(int(prefix[r[k][0]]) - prefix[-1] * k / world) <= w.max()
        # and equal draw counts do not achieve that here: one mesh far heavier than the rest, all of its draws first
    meshes = np.zeros(2, dtype=L.MESH)
    meshes["lodCount"] = 1
    meshes["lods"]["meshletCount"][:, 0] = (1000, 1)
    draws = np.zeros(100, dtype=L.MESHDRAW)
    draws["meshIndex"][10:] = 1
    (b0, e0), (b1, e1) = shard.draw_ranges(draws, meshes, 2, "meshlets")
    assert (b0, e0, b1, e1) == (0, 5, 5, 100)
    with pytest.raises(ValueError):
        shard.draw_ranges(draws, meshes, 2, "triangles")


# ---- rebase and stitch helpers

def test_draw_ids_are_rebased_in_a_copy_for_both_command_kinds():
    for dt in (L.TASKCMD, L.DRAWCMD):
        c = np.zeros(3, dtype=dt)
        c["drawId"] = (0, 1, 5)
        out = shard.to_global_draw_ids(c, 100)
        assert out["drawId"].tolist() == [100, 101, 105] and c["drawId"].tolist() == [0, 1, 5]
        c2 = c.copy()
        c2["drawId"] = 0
        assert out.tobytes() != c.tobytes() and shard.to_global_draw_ids(c[:0], 7).size == 0
    with pytest.raises(ValueError):
        shard.to_global_draw_ids(c, (1 << 32) - 3)


def test_stitched_cluster_ids_rebase_by_the_earlier_ranks_commands():
    a = np.array([0 | (3 << 24), 1 | (63 << 24), 0xffffffff, 0xffffffff], np.uint32)  # rank 0: 2 commands, with clustersubmit's padding
    b = np.array([0 | (1 << 24), 4 | (2 << 24)], np.uint32)                             # rank 1: 5 commands
    c = np.array([2], np.uint32)
    out = shard.stitch_cluster_ids([a, b, c], [2, 5, 3])
    assert out.tolist() == [0 | (3 << 24), 1 | (63 << 24), 2 | (1 << 24), 6 | (2 << 24), 9]
    # padding entries stay ~0 through the rebase itself, and the 24-bit command field must not overflow
    assert shard.to_global_ids(a, 10).tolist() == [10 | (3 << 24), 11 | (63 << 24), 0xffffffff, 0xffffffff]
    with pytest.raises(ValueError):
        shard.stitch_cluster_ids([a, b], [(1 << 24) - 3, 5])
    assert shard.stitch_cluster_ids([a[2:], b], [(1 << 24) - 5, 5]).tolist() == [((1 << 24) - 5) | (1 << 24), ((1 << 24) - 1) | (2 << 24)]


def test_stitched_visibility_is_concatenation_and_or():
    dvb, mvb = shard.stitch_visibility([np.array([1, 0], np.uint32), np.array([1], np.uint32)],
                                       [np.array([0x0000ffff, 0, 0], np.uint32), np.array([0x00ff0000, 7, 0], np.uint32)])
    assert dvb.tolist() == [1, 0, 1] and mvb.tolist() == [0x00ffffff, 7, 0]


def test_composite_depth_without_a_group_is_a_no_op():
    d = torch.rand(4, 5)
    assert shard.composite_depth(d.clone()).equal(d)
