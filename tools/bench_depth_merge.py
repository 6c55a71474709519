#!/usr/bin/env python3
"""nv_depth_merge against the bytes it must move and against K torch.maximum calls (profiles/r09_sharded_frame.md).

    python3 tools/bench_depth_merge.py                                   # event-timed, the shortest of three loops per case
    rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/bench_depth_merge.py --iters 20     # the kernels' own durations

Prints one JSON line per case: size, sources, microseconds per call, the traffic (sources + 2) * 4 * width * height bytes, the
bandwidth that time means, and the time of the torch.maximum chain that does the same work."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, iters):
    import torch
    best = float("inf")
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / iters)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    import torch
    from niagara_amd import pipeline as P
    ctx = P.Context()
    dev = ctx.device
    for w, h in ((1920, 1080), (4096, 4096)):
        for k in (1, 2, 8):
            dst = torch.rand((h, w), device=dev)
            srcs = [torch.rand((h, w), device=dev) for _ in range(k)]
            views = [s.view(torch.int32) for s in srcs]
            dv = dst.view(torch.int32)

            def merge():
                ctx.depth_merge(dst, srcs, w, h)

            def chain():
                for v in views:
                    torch.maximum(dv, v, out=dv)
            merge(), chain()
            t_merge, t_chain = timed(merge, args.iters), timed(chain, args.iters)
            traffic = (k + 2) * 4 * w * h
            print(json.dumps(dict(width=w, height=h, sources=k, depth_merge_us=round(t_merge, 2), bytes=traffic,
                                  depth_merge_TBps=round(traffic / t_merge / 1e6, 3), floor_us_at_8TBps=round(traffic / 8e6, 2),
                                  torch_maximum_chain_us=round(t_chain, 2), chain_bytes=3 * k * 4 * w * h)))
    ctx.status()
    ctx.close()


if __name__ == "__main__":
    main()
