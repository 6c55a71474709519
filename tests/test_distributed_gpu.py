"""The N > 1 path executed with the HIP kernels.  A gpurun box has ONE GPU, so both ranks share
cuda:0 and the process group is gloo; what runs is exactly bench.py's N > 1 code and niagara_amd/shard.py — command
ranges, nv_set_counts_sink rows written by the scatter launch, the batched asynchronous all-reduce, ID rebasing — only
the transport differs from the 8-GPU run (RCCL over xGMI), which is the driver's to launch."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize("batch, streams, total", [(8, 2, 0), (1, 2, 0), (3, 2, 0), (8, 1, 0), (3, 3, 0), (8, 1, 3_000_000 + 64 * 7)])
def test_bench_two_ranks_on_one_device(batch, streams, total):
    """python -m torch.distributed.run --nproc-per-node 2 bench.py --gpus 2 --backend gloo --shared-device: rc 0, one JSON
    line, and the all-reduced visible count of the last pass = the sum of what the oracle sees in the two shards.  total > 0:
    the strong-scaling mode (--total-meshlets), with a shard boundary in the middle of a draw's commands."""
    import argparse
    import oracle
    sys.path.insert(0, ROOT)
    import bench
    from niagara_amd import synth
    draws_per_rank, cpd, steps = 3000, 10, 16
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = None
    for attempt in range(2):  # (a rendezvous that never completes — seen once on the GPU box — gets one more try on a fresh port)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
               str(_free_port()), os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--backend", "gloo", "--shared-device", "--steps", str(steps), "--warmup", "3",
               "--counts-batch", str(batch), "--streams", str(streams), "--draws", str(draws_per_rank)] + (["--total-meshlets", str(total), "--cpu-seconds", "0.2"] if total else ["--no-cpu-baseline"])
        try:
            out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=180, cwd=ROOT)
            break
        except subprocess.TimeoutExpired:
            if attempt == 1:
                raise
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["steps"] == steps and rec["scaling"] == ("strong" if total else "weak") and rec["config"]["streams"] == streams
    assert rec["config"]["meshlets_total"] == (total if total else 2 * draws_per_rank * cpd * 64)
    assert "collective_wait_ms" in rec and rec["throughput_overlapped"] is None
    assert len(set(rec["config"]["visible_per_stream"])) == 1  # every stream's last pass saw the same scene
    want = []
    args = argparse.Namespace(draws=draws_per_rank, commands_per_draw=cpd, total_meshlets=total)
    for rank in range(2):
        draws, meshlets, cd, (b, e), _ = bench.make_inputs(args, rank, 2)
        commands = bench.make_commands(b, e, cpd)
        cib, cc4 = np.zeros(len(commands) * 64, np.uint32), np.zeros(4, np.uint32)
        oracle.clustercull(cd, 0, commands, synth.count4_for(e - b), draws, meshlets, None, None, cib, cc4, threads=oracle.max_threads())
        want.append(int(cc4[0]))
    if total:
        assert (total // 64 // 2) % cpd != 0  # the boundary splits a draw's commands
    assert rec["config"]["visible_rank0"] == want[0]
    assert rec["config"]["visible_total"] == want[0] + want[1] and want[1] > 0
    if total:  #  the N > 1 line is gradeable: parity on every rank's shard and a CPU baseline
        assert rec["parity"] == "bit-identical" and "2 of 2 ranks" in rec["parity_checked"] and rec["cpu_baseline"]["value"] > 0


@pytest.mark.parametrize("batch, streams, launcher", [(1, 1, "run"), (3, 1, "run"), (8, 1, "run"), (8, 2, "run"), (3, 2, "run"), (8, 1, "alone")])
def test_bench_forced_sharded_over_rccl(batch, streams, launcher):
    """the sharded Python path over RCCL before the driver's 8-GPU run.  `torch.distributed.run --nproc-per-node 1
    bench.py --gpus 1 --force-sharded` (backend nccl = RCCL) takes every N > 1 branch with one rank: process group + warm-up
    all-reduce, CountsReducer's asynchronous batched all-reduce on the device rows the scatter launch writes (its stream ordering and
    waits — under gloo those collectives are host-synchronous), barrier, MAX over the ranks, per-rank oracle check + flag all-reduce.
    The reduced counts must be the pass's own and the visible-ID list the oracle's.  launcher "alone": plain `python bench.py
    --force-sharded` (the rendezvous variables default to this host)."""
    import argparse
    import oracle
    sys.path.insert(0, ROOT)
    import bench
    from niagara_amd import synth
    draws, cpd, steps = 3000, 10, 19  # (19: a partial last batch for every batch size but 1)
    tail = [os.path.join(ROOT, "bench.py"), "--full", "--gpus", "1", "--force-sharded", "--backend", "nccl", "--steps", str(steps), "--warmup", "3", "--counts-batch", str(batch),
            "--streams", str(streams), "--draws", str(draws), "--cpu-seconds", "0.2"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    if launcher == "run":
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port", str(_free_port())] + tail
    else:
        cmd = [sys.executable] + tail
        for k in ("MASTER_ADDR", "MASTER_PORT", "RANK", "WORLD_SIZE", "LOCAL_RANK"):
            env.pop(k, None)
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    cfg = rec["config"]
    assert rec["n_gpus"] == 1 and cfg["force_sharded"] is True and cfg["backend"] == "nccl" and cfg["streams"] == streams
    assert "async all-reduce" in cfg["counts_allreduce"] and rec["throughput_overlapped"] is None and "collective_wait_ms" in rec
    args = argparse.Namespace(draws=draws, commands_per_draw=cpd, total_meshlets=0)
    d, meshlets, cd, (b, e), _ = bench.make_inputs(args, 0, 1)
    commands = bench.make_commands(b, e, cpd)
    cib, cc4 = np.zeros(len(commands) * 64, np.uint32), np.zeros(4, np.uint32)
    oracle.clustercull(cd, 0, commands, synth.count4_for(e - b), d, meshlets, None, None, cib, cc4, threads=oracle.max_threads())
    # the all-reduced count (one rank: the sum is the pass's own) = what the pass left in its count word = the oracle's
    assert cfg["visible_total"] == cfg["visible_rank0"] == int(cc4[0]) > 0 and len(set(cfg["visible_per_stream"])) == 1
    assert rec["parity"] == "bit-identical" and "1 of 1 ranks" in rec["parity_checked"] and rec["cpu_baseline"]["value"] > 0


def test_config5_eight_ranks_100m_meshlets(tmp_path):
    """BASELINE config 5 end to end with the HIP kernels: `python bench.py --gpus 8 --total-meshlets 100000000` — bench.py launching its own ranks
    under torch.distributed.run (gloo, the eight ranks sharing the box's one device — on an 8-GPU node the same command with the default backend is the
    RCCL run).  The line must carry `parity` (every rank against the oracle on its shard, inside bench.py) and `cpu_baseline`; and the
    eight ranks' rebased ID lists, concatenated in rank order, must be the oracle's list over the UNSHARDED 100 M-meshlet pool."""
    import argparse
    import oracle
    sys.path.insert(0, ROOT)
    import bench
    from niagara_amd import host, synth
    world, total, cpd = 8, 100_000_000, 10
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    # (no launcher in front — bench.py starts its own eight ranks, as the driver's `python3 bench.py --gpus N ...` needs)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", str(world), "--backend", "gloo", "--shared-device", "--steps", "3", "--warmup", "2",
           "--total-meshlets", str(total), "--copies", "2", "--cpu-seconds", "0.5", "--dump-ids", str(tmp_path)]
    env = {k: v for k, v in env.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert rec["n_gpus"] == world and rec["scaling"] == "strong" and rec["config"]["meshlets_total"] == total // 64 * 64
    assert rec["parity"] == "bit-identical" and "8 of 8 ranks" in rec["parity_checked"]
    assert rec["cpu_baseline"]["value"] > 0 and rec["cpu_baseline"]["kind"] == "port" and "1 / 8" in rec["cpu_baseline"]["sample"]
    # the unsharded pool: rank r's meshlets are its own seeded stream, packed in rank order; one oracle pass over all of it
    args = argparse.Namespace(draws=0, commands_per_draw=cpd, total_meshlets=total)
    total_cmd = total // 64
    pool = []
    for rank in range(world):
        _, meshlets, cd, (b, e), tc = bench.make_inputs(args, rank, world)
        assert tc == total_cmd and len(meshlets) == (e - b) * 64
        pool.append(meshlets)
    pool = np.concatenate(pool)
    draws = host.synth_draws((total_cmd + cpd - 1) // cpd, 1, 300.0)
    commands = bench.make_commands(0, total_cmd, cpd)
    cib, cc4 = np.zeros(total_cmd * 64, np.uint32), np.zeros(4, np.uint32)
    oracle.clustercull(cd, 0, commands, synth.count4_for(total_cmd), draws, pool, None, None, cib, cc4, threads=oracle.max_threads())
    ids = np.concatenate([np.load(tmp_path / ("ids_%d.npy" % r)) for r in range(world)])
    assert rec["config"]["visible_total"] == int(cc4[0]) == len(ids) and len(ids) > 1_000_000
    assert (ids == cib[:len(ids)]).all()


def test_bench_launches_its_own_ranks():
    """VERDICT r5 item 1, the exact command of its `Done`: `python3 bench.py --gpus 2 --backend gloo --shared-device --steps 5 --warmup 2` with NO launcher
    and no rendezvous variables in the environment: rc 0, one JSON line for two ranks, parity on both shards"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--backend", "gloo", "--shared-device", "--steps", "5", "--warmup", "2"],
                         env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["steps"] == 5 and rec["warmup"] == 2 and rec["scaling"] == "weak"
    assert rec["config"]["meshlets_total"] == 2 * 10_000_000 and rec["value"] > 0
    assert rec["parity"] == "bit-identical" and "2 of 2 ranks" in rec["parity_checked"] and rec["cpu_baseline"]["value"] > 0


def test_bench_driver_command_carries_frame_and_contract_rooflines():
    """the driver's N = 1 command with --full: the line carries the headline's roofline + cpu_baseline, `contract_chain` with its own roofline
     and the dependent `frame` at BASELINE scale with its HBM fraction, per-launch times and parity (item 6a)"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "1", "--steps", "20", "--warmup", "5"], capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["parity"] == "bit-identical" and "TIMED loop" in rec["parity_checked"]
    assert 0 < rec["roofline"]["frac"] < 1 and rec["cpu_baseline"]["value"] > 0
    cc = rec["contract_chain"]
    assert cc["parity"] == "bit-identical" and 0 < cc["roofline"]["frac"] < 1
    assert cc["roofline"]["algorithmic_bytes"] == sum(cc["roofline"]["per_pass_bytes"].values())
    assert cc["roofline"]["per_pass_bytes"]["drawcull"] == 52 * cc["draws"] + 20 * cc["task_commands"]
    assert cc["roofline"]["per_pass_bytes"]["cluster"] == 12 * cc["meshlets_tested"] + 68 * cc["task_commands"] + 4 * cc["visible"] + 4
    fr = rec["frame"]
    assert fr["parity"] == "bit-identical" and 0 < fr["frac"] < 1 and fr["frame_us"] > 0
    assert set(fr["launch_us"]) >= {"early_drawcull", "early_cluster_cull", "early_cluster_scatter", "pyramid", "late_drawcull", "late_cluster_cull", "late_cluster_hiz", "late_cluster_scatter"}
    assert sum(fr["launch_us"].values()) < fr["frame_us"] * 1.5 and fr["early"]["meshlets_tested"] > 5_000_000 and fr["late"]["meshlets_tested"] > 5_000_000


def test_bench_single_gpu_line_is_one_regime():
    """the default line's value / ms_per_step are one pass after the other on one stream, the dominant kernel's
    event time fits inside a step, and the several-passes-in-flight figure is a side field"""
    sys.path.insert(0, ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "30", "--warmup", "5", "--draws", "6000", "--cpu-seconds", "0.2", "--no-frame"],
                         capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert rec["config"]["streams"] == 1 and "note" not in rec
    assert rec["roofline"]["kernel_avg_us"] * 1e-3 <= rec["ms_per_step"] * 1.02
    assert abs(rec["roofline"]["ms_per_pass_single_stream"] - rec["ms_per_step"]) < 1e-9
    assert rec["throughput_overlapped"]["streams"] == 3 and rec["throughput_overlapped"]["value"] > 0
    assert rec["cpu_baseline"]["visible_list"].startswith("bit-identical") and rec["config"]["visible_total"] == rec["config"]["visible_rank0"]
    assert rec["parity"] == "bit-identical"


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """a plain run (no --full): exactly `--steps` timed passes, the headline fields and none of the side fields, and --dump-outputs writes the last timed
    pass's visible-ID list and count words as float64 — the list is the CPU oracle's for the same seeded inputs"""
    import argparse
    import oracle
    sys.path.insert(0, ROOT)
    import bench
    from niagara_amd import synth
    draws, cpd, steps = 6000, 10, 7
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2", "--draws", str(draws),
                          "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["metric"] == "meshlets culled+compacted /sec" and rec["unit"] == "meshlets/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
    assert rec["steps"] == steps and rec["warmup"] == 2 and rec["ms_per_step"] > 0
    assert abs(rec["value"] - rec["config"]["meshlets_total"] / (rec["ms_per_step"] * 1e-3)) < 1e-6 * rec["value"]
    assert not set(rec) & {"roofline", "throughput_overlapped", "cpu_baseline", "parity", "contract_chain", "frame"}
    ids, count = np.load(tmp_path / "out" / "visible_ids.npy"), np.load(tmp_path / "out" / "count.npy")
    assert ids.dtype == np.float64 and count.dtype == np.float64 and count.shape == (4,)
    assert int(count[0]) == len(ids) == rec["config"]["visible_rank0"] > 0
    args = argparse.Namespace(draws=draws, commands_per_draw=cpd, total_meshlets=0)
    d, meshlets, cd, (b, e), _ = bench.make_inputs(args, 0, 1)
    commands = bench.make_commands(b, e, cpd)
    cib, cc4 = np.zeros(len(commands) * 64, np.uint32), np.zeros(4, np.uint32)
    oracle.clustercull(cd, 0, commands, synth.count4_for(e - b), d, meshlets, None, None, cib, cc4, threads=oracle.max_threads())
    assert int(cc4[0]) == len(ids) and (ids == cib[:len(ids)].astype(np.float64)).all()


def _worker(rank, world, port, out_dir):
    import torch
    import torch.distributed as dist
    from niagara_amd import host, shard, synth
    from niagara_amd import pipeline as P
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    ctx = P.Context(0)
    dev = ctx.device
    draws, meshlets, commands, n = synth.cluster_scene(2500, 7, seed=5)
    cd = host.build_cull_data(draw_count=len(draws), cullingEnabled=1, clusterBackfaceEnabled=1)
    b, e = shard.command_range(n, rank, world)
    local, ln = shard.local_commands(commands, b, e)
    db, mlb, dcb = P.to_device(draws, dev), P.to_device(meshlets, dev), P.to_device(local, dev)
    ctx.upload_meshlets(mlb, len(meshlets))
    dccb = torch.from_numpy(synth.count4_for(ln).view(np.int32).copy()).to(dev)
    cib = torch.zeros(len(local) * 64 + 256, dtype=torch.int32, device=dev)
    ccb = torch.zeros(4, dtype=torch.int32, device=dev)
    red = shard.CountsReducer(ctx, dev, batch=2)
    for i in range(5):
        ccb.zero_()
        red.before_pass(i)
        ctx.clustercull(cd, 0, dcb, dccb, db, mlb, None, None, cib, ccb)
        ctx.clustersubmit(ccb, cib)
        red.after_pass(i)
    red.drain(5)
    ctx.status()
    total = int(ccb[0].item())
    padded = (total + 255) // 256 * 256
    ids = shard.to_global_ids(cib[:padded].cpu().numpy().view(np.uint32), b)
    np.save(os.path.join(out_dir, "ids_%d.npy" % rank), ids[:total])
    np.save(os.path.join(out_dir, "pad_%d.npy" % rank), ids[total:])
    np.save(os.path.join(out_dir, "counts_%d.npy" % rank), red.last(5).cpu().numpy())
    dist.barrier()
    ctx.close()
    dist.destroy_process_group()


def test_two_ranks_run_the_hip_pass_on_their_shards(tmp_path):
    """each rank culls ITS command range with nv_clustercull (not the oracle), rebases its IDs; concatenated they are the
    unsharded oracle list, the padding entries stay ~0, and every rank holds the global sums"""
    import torch.multiprocessing as mp
    import oracle
    from niagara_amd import host, synth
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    draws, meshlets, commands, n = synth.cluster_scene(2500, 7, seed=5)
    cd = host.build_cull_data(draw_count=len(draws), cullingEnabled=1, clusterBackfaceEnabled=1)
    cib, cc4 = np.zeros(len(commands) * 64 + 256, np.uint32), np.zeros(4, np.uint32)
    oracle.clustercull(cd, 0, commands, synth.count4_for(n), draws, meshlets, None, None, cib, cc4)
    ids = np.concatenate([np.load(tmp_path / ("ids_%d.npy" % r)) for r in range(world)])
    assert cc4[0] > 1000 and (ids == cib[:cc4[0]]).all()
    for r in range(world):
        assert (np.load(tmp_path / ("pad_%d.npy" % r)) == 0xffffffff).all()
        c = np.load(tmp_path / ("counts_%d.npy" % r))
        assert c[1] == n and c[2] == cc4[0]
