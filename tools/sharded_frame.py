#!/usr/bin/env python3
"""The closed-loop frame sharded over ranks by draw ranges (niagara_amd.pipeline.ShardedVisibilityPipeline).

    python3 tools/sharded_frame.py --gpus 8 --frames 20                       # one rank per GPU, RCCL
    python3 tools/sharded_frame.py --gpus 2 --backend gloo --shared-device    # a one-GPU box: every rank on cuda:0, gloo
    python3 tools/sharded_frame.py --gpus 1 --force-collective                # one rank, the composite's all_reduce(MAX) over RCCL anyway
    python3 tools/sharded_frame.py --local-shards 8                           # 8 shards in ONE process, composite = nv_depth_merge
    python3 tools/sharded_frame.py --as-rank 0/8                              # one rank's share alone (no exchange): the per-rank frame cost
    python3 tools/sharded_frame.py --local-shards 4 --visibility              # + the stable-ID visibility buffer, composited and resolved
    python3 tools/sharded_frame.py --local-shards 2 --scene occluder_indexed --visibility --attributes   # the classic path's

Like bench.py --gpus N it starts its own ranks under torch.distributed.run when no launcher did.  Prints ONE JSON line (rank 0): the
per-phase counts of the last frame summed over the ranks, the frame time (MAX over the ranks; the shortest of three timed loops of
--frames frames) and the time of one depth composite.  --dump DIR writes rank_<r>.npz per rank: for every frame f and phase p the
commands, cluster ids, dvb (the rank's draws), mvb, counts and depth, and the pyramid per frame (the frames start from cleared
visibility; nothing is timed then).  --visibility runs the frame with stable ids (on an indexed scene: the classic path, its triangle names and indexed records) and a visibility target per rank,
composited with the depth; the JSON line gains the resolve totals of the last frame and the dump "f<f>_visibility" and "f<f>_records".
--attributes (with --visibility) runs the attribute pass on every rank after the last frame (a fixed four-entry material table; the
vertices' packed fields as the scene has them): the JSON line gains its totals and one digest of the outputs per rank of this process
(equal digests: every rank shades the same frame), the dump attributes_<r>.npz."""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gpus", type=int, default=1, help="ranks (one process each)")
    ap.add_argument("--backend", choices=("nccl", "gloo"), default="nccl")
    ap.add_argument("--shared-device", action="store_true", help="functional runs on a one-GPU box: all ranks use cuda:0 (needs --backend gloo)")
    ap.add_argument("--force-collective", action="store_true", help="create the process group and issue the composite's all-reduce with one rank too")
    ap.add_argument("--local-shards", type=int, default=0, help="K shards inside this one process (no process group): composite by nv_depth_merge")
    ap.add_argument("--as-rank", default="", help="R/K: run rank R of K alone, without any exchange")
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scene", choices=("occluder", "occluder_indexed", "interior"), default="occluder")
    ap.add_argument("--hidden", type=int, default=8, help="occluder scenes: boxes behind the wall")
    ap.add_argument("--beside", type=int, default=4, help="occluder scenes: boxes beside the wall")
    ap.add_argument("--viewport", default="320x192")
    ap.add_argument("--weight", choices=("draws", "meshlets"), default="draws")
    ap.add_argument("--post", action="store_true", help="run the post phase too")
    ap.add_argument("--unfused", action="store_true", help="the reference's dispatch sequence one to one (default: fused resets / submits)")
    ap.add_argument("--skip-last-composite", action="store_true")
    ap.add_argument("--dump", default="", help="directory for rank_<r>.npz")
    ap.add_argument("--visibility", action="store_true", help="stable-ID visibility buffer: composited with the depth, resolved after the frame")
    ap.add_argument("--attributes", action="store_true", help="with --visibility: the attribute pass (nv_visibility_attributes) on every rank after the last frame")
    return ap.parse_args(argv)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def self_launch_command(gpus, argv, port=None):
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus), "--master-addr", "127.0.0.1", "--master-port",
            str(port or _free_port()), os.path.abspath(__file__)] + list(argv)


def make_scene(args):
    """(scene dict, task, near_clip) with the meshlet bounds computed on the current device (nv_meshlet_bounds)"""
    import numpy as np
    from niagara_amd import layouts as L
    from niagara_amd import pipeline as P
    from niagara_amd import synth
    vp = tuple(int(x) for x in args.viewport.split("x"))

    def bounds(vertices, data, meshlets):
        ctx = P.Context()
        try:
            mlb = P.to_device(meshlets, ctx.device)
            ctx.meshlet_bounds(P.to_device(vertices, ctx.device), P.to_device(data, ctx.device), mlb, len(meshlets))
            ctx.status()
            meshlets[:] = P.from_device(mlb, L.MESHLET)
        finally:
            ctx.close()
    if args.scene == "interior":
        return synth.interior_scene(viewport=vp, meshlet_bounds=bounds), True, True
    kw = dict(viewport=vp, hidden=args.hidden, beside=args.beside, meshlet_bounds=bounds)
    if args.scene == "occluder_indexed":
        return synth.occluder_scene_indexed(**kw), False, False
    return synth.occluder_scene(**kw), True, False


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL across processes needs it on this driver
        raise SystemExit(subprocess.call(self_launch_command(args.gpus, sys.argv[1:]), env=env))
    import numpy as np
    import torch
    import torch.distributed as dist

    from niagara_amd import shard
    from niagara_amd import layouts as L
    from niagara_amd import pipeline as P

    world, rank, local_rank = (int(os.environ.get(k, d)) for k, d in (("WORLD_SIZE", "1"), ("RANK", "0"), ("LOCAL_RANK", "0")))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if args.shared_device:
        if args.backend != "gloo" and world > 1:
            raise SystemExit("--shared-device needs --backend gloo: RCCL wants one device per rank")
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    grouped = world > 1 or args.force_collective
    if grouped:
        if "MASTER_ADDR" not in os.environ:
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), RANK="0", WORLD_SIZE="1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(args.backend)
        dist.all_reduce(torch.zeros(1, dtype=torch.int32, device=dev), op=dist.ReduceOp.MAX)  # communicator set-up is not part of a frame
        torch.cuda.synchronize()

    s, task, near_clip = make_scene(args)
    geometry = dict(vertices=s["vertices"], meshlet_data=s["data"]) if task else dict(vertices=s["vertices"], indices=s["indices"])
    classic = not task  # an indexed scene: the classic path's visibility buffer, resolve and attribute pass
    if args.attributes and not args.visibility:
        raise SystemExit("--attributes reads the resolved visibility buffer: add --visibility")
    kw = dict(task_capacity=4096 if len(s["draws"]) < 256 else None, cluster_capacity=4096 * 64 if len(s["draws"]) < 256 else None,
              fused=not args.unfused, near_clip=near_clip, weight=args.weight, stable_ids=args.visibility, **geometry)
    shards = None
    if args.local_shards:
        shards = P.ShardedVisibilityPipeline.local_shards(s["meshes"], s["meshlets"], s["draws"], s["viewport"], args.local_shards, **kw)
        pipes, n_ranks = shards.pipes, args.local_shards
        runner = shards
    else:
        r, k = (int(x) for x in args.as_rank.split("/")) if args.as_rank else (rank, world)
        pipes = [P.ShardedVisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], rank=r, world=k, group=True if grouped else None, **kw)]
        runner, n_ranks = pipes[0], k
    w, h = s["viewport"]
    names = ["early", "late"] + (["post"] if args.post else [])
    frame_kw = dict(post_pass=args.post, task=task, composite_last=not args.skip_last_composite)
    vis = None
    if args.visibility:
        vis = shards.new_visibility() if shards else pipes[0].new_visibility()
        frame_kw["visibility"] = vis
    vis_of = (lambda k: vis[k]) if shards else (lambda k: vis)

    def counts_now():
        c = torch.stack([p.phase_counts(task) for p in pipes]).sum(0)
        return shard.allreduce_counts(c.cpu() if grouped and args.backend == "gloo" else c).cpu().numpy()

    result = dict(metric="sharded_frame", scene=args.scene, draws=len(s["draws"]), viewport=[w, h], ranks=n_ranks, processes=world,
                  deployment="local_shards" if shards else ("as_rank" if args.as_rank else "process_per_rank"), backend=args.backend if grouped else None,
                  weight=args.weight, ranges=[[p.begin, p.end] for p in pipes] if shards or world == 1 else None, frames=args.frames, phases=names,
                  composite_payload_bytes=w * h * 4, composites_per_frame=len(names) - int(args.skip_last_composite))
    last_counts = {}
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
        dumps = [dict(begin=p.begin, end=p.end, frames=args.frames) for p in pipes]
        for f in range(args.frames):
            def grab(name, f=f):
                c = counts_now()
                last_counts[name] = c
                for p, d in zip(pipes, dumps):
                    c4, cc4 = p.dccb.cpu().numpy().view(np.uint32), p.ccb.cpu().numpy().view(np.uint32)
                    key = "f%d_%s_" % (f, name)
                    d[key + "count4"], d[key + "cc4"], d[key + "counts"] = c4.copy(), cc4.copy(), c
                    d[key + "commands"] = P.from_device(p.dcb, L.TASKCMD if task else L.DRAWCMD)[:int(c4[0])].copy()
                    d[key + "cib"] = p.cib.cpu().numpy().view(np.uint32)[:int(cc4[0]) if task else 0].copy()
                    d[key + "dvb"] = p.dvb.cpu().numpy().view(np.uint32).copy()
                    d[key + "mvb"] = p.mvb.cpu().numpy().view(np.uint32).copy()
                    d[key + "depth"] = p.depth.cpu().numpy().copy()
            runner.frame(s["cull"], on_phase=grab, **frame_kw)
            for k, (p, d) in enumerate(zip(pipes, dumps)):
                d["f%d_pyramid" % f] = p.pyramid.data.cpu().numpy().copy()
                if vis is not None:
                    d["f%d_visibility" % f] = vis_of(k).cpu().numpy().view(np.uint64).copy()
                    d["f%d_records" % f] = P.from_device(p.resolve(s["cull"], vis_of(k), classic=classic)["records"],
                                                          L.VISINDEXEDRECORD if classic else L.VISRECORD).copy()
        for p, d in zip(pipes, dumps):
            np.savez(os.path.join(args.dump, "rank_%d.npz" % (p.rank if shards or args.as_rank else rank)), **d)
        result.update(frame_ms=None, composite_ms=None, timed=False)
    else:
        for _ in range(args.warmup):
            runner.frame(s["cull"], **frame_kw)
        best = float("inf")
        for _ in range(3):  # the shortest of three timed loops
            torch.cuda.synchronize()
            if grouped:
                dist.barrier()
            t0 = time.perf_counter()
            for _ in range(args.frames):
                runner.frame(s["cull"], **frame_kw)
            torch.cuda.synchronize()
            best = min(best, (time.perf_counter() - t0) * 1e3 / args.frames)
        comp = float("inf")
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                runner.composite()
            torch.cuda.synchronize()
            comp = min(comp, (time.perf_counter() - t0) * 1e3 / 20)
        t = torch.tensor([best, comp], dtype=torch.float64, device="cpu" if args.backend == "gloo" else dev)
        if grouped:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        runner.frame(s["cull"], on_phase=lambda name: last_counts.__setitem__(name, counts_now()), **frame_kw)
        result.update(frame_ms=float(t[0]), composite_ms=float(t[1]), timed=True)
    if vis is not None:  # every rank holds the frame's buffer after the composite: rank 0's resolve is the frame's
        tot = pipes[0].resolve(s["cull"], vis_of(0), records=False, classic=classic)["totals"].cpu().numpy()
        result.update(visibility=True, covered_pixels=int(tot[0]), unresolved_pixels=int(tot[1]), visibility_payload_bytes=w * h * 8)
    if args.attributes:  # the records are global after the composite: every rank shades the whole frame, and all of them the same bytes
        import hashlib
        mats = np.zeros(4, L.MATERIAL)
        mats["diffuseFactor"], mats["specularFactor"] = (0.8, 0.6, 0.4, 1.0), (0.5, 0.5, 0.5, 0.25)
        mats["diffuseFactor"][:, 0] = np.linspace(0.2, 1.0, 4)
        digests, tot = [], None
        for k, p in enumerate(pipes):
            out = p.attributes(s["cull"], p.resolve(s["cull"], vis_of(k), classic=classic)["records"], mats, classic=classic)
            tot = out["totals"].cpu().numpy()
            hsh = hashlib.sha256()
            for name in ("attributes", "gbuffer0", "gbuffer1"):
                hsh.update(out[name].cpu().numpy().tobytes())
            digests.append(hsh.hexdigest()[:16])
            if args.dump:
                np.savez(os.path.join(args.dump, "attributes_%d.npz" % (p.rank if shards or args.as_rank else rank)),
                         attributes=P.from_device(out["attributes"], L.PIXELATTR), gbuffer0=out["gbuffer0"].cpu().numpy().view(np.uint32),
                         gbuffer1=out["gbuffer1"].cpu().numpy().view(np.uint32))
        result.update(attributes=True, shaded_pixels=int(tot[0]), invalid_records=int(tot[1]), degenerate_pixels=int(tot[2]), attribute_digests=digests,
                      attribute_payload_bytes=w * h * (L.PIXELATTR.itemsize + 8))
    for p in pipes:
        p.ctx.status()
    result["counts"] = {n: [int(x) for x in last_counts[n]] for n in names}
    result["counts_fields"] = ["visible draws or task commands", "task groups", "visible meshlets"]
    if grouped:
        dist.barrier()
        dist.destroy_process_group()
    for p in pipes:
        p.ctx.close()
    if rank == 0:
        print(json.dumps(result))


if __name__ == "__main__":
    main()
