#!/usr/bin/env python3
"""Timings of the frame-stable visibility buffer on one GPU, one JSON line per measurement.

    python3 tools/bench_visibility.py                      # product library
    NV_LIBRARY_PATH=niagara_amd/libniagara_vis_exp.so NV_RESOLVE_PER_PIXEL=1 python3 tools/bench_visibility.py --only resolve

Every figure is the median over --repeats batches of device-event time around --batch back-to-back launches, divided by the batch
(launch gaps included: an upper bound of the kernel time).  The frame rasterised is synth.occluder_scene at the given viewport."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, batch, repeats):
    import torch
    for _ in range(3):
        fn()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(batch):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / batch)
    return dict(us_median=round(statistics.median(out), 2), us_min=round(min(out), 2), us_max=round(max(out), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    import numpy as np
    import torch

    from niagara_amd import layouts as L
    from niagara_amd import pipeline as P
    from niagara_amd import synth

    def bounds(vertices, data, meshlets):
        ctx = P.Context()
        mlb = P.to_device(meshlets, ctx.device)
        ctx.meshlet_bounds(P.to_device(vertices, ctx.device), P.to_device(data, ctx.device), mlb, len(meshlets))
        ctx.status()
        meshlets[:] = P.from_device(mlb, L.MESHLET)
        ctx.close()

    say = lambda **kw: print(json.dumps(kw), flush=True)
    per_pixel = os.environ.get("NV_RESOLVE_PER_PIXEL", "0") != "0"
    for w, h in ((1920, 1080), (4096, 4096)):
        s = synth.occluder_scene(viewport=(w, h), meshlet_bounds=bounds)
        kw = dict(task_capacity=4096, cluster_capacity=4096 * 64, fused=True, vertices=s["vertices"], meshlet_data=s["data"])
        pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], stable_ids=True, **kw)
        plain = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], stable_ids=False, **kw)
        vis = pipe.new_visibility()
        for _ in range(3):
            pipe.frame(s["cull"], post_pass=True, visibility=vis)
            plain.frame(s["cull"], post_pass=True)
        dev = pipe.ctx.device
        if args.only in ("", "frame"):  # (d) the closed loop with and without the target
            say(what="frame", viewport=[w, h], visibility=False, **timed(lambda: plain.frame(s["cull"], post_pass=True), 5, args.repeats))
            say(what="frame", viewport=[w, h], visibility=True, **timed(lambda: pipe.frame(s["cull"], post_pass=True, visibility=vis), 5, args.repeats))
        if args.only in ("", "raster"):  # (a) the last pass's list again: depth only, slot words, stable words
            slotvis = plain.new_visibility()
            say(what="rasterdepth", viewport=[w, h], words="none", **timed(lambda: plain.render_depth(s["cull"], late=True, post_pass=1), args.batch, args.repeats))
            say(what="rasterdepth", viewport=[w, h], words="slot", **timed(lambda: plain.render_depth(s["cull"], late=True, post_pass=1, visibility=slotvis), args.batch, args.repeats))
            say(what="rasterdepth", viewport=[w, h], words="stable", **timed(lambda: pipe.render_depth(s["cull"], late=True, post_pass=1, visibility=vis), args.batch, args.repeats))
        pipe.frame(s["cull"], post_pass=True, visibility=vis)
        if args.only in ("", "resolve"):  # (b)
            rec = torch.zeros(w * h * 16, dtype=torch.uint8, device=dev)
            seen, dp, tot = torch.zeros_like(pipe.mvb), torch.zeros(len(s["draws"]), dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
            c = pipe.ctx
            full = lambda: c.visibility_resolve(s["cull"], vis, w, h, pipe.db, pipe.draw_count, pipe.mb, pipe.mesh_count, rec, seen, dp, tot)
            recs = lambda: c.visibility_resolve(s["cull"], vis, w, h, pipe.db, pipe.draw_count, pipe.mb, pipe.mesh_count, rec)
            floor_us = w * h * 24 / 8e12 * 1e6
            covered = int((vis != 0).sum().item())
            say(what="resolve", viewport=[w, h], outputs="all", per_pixel=per_pixel, covered=covered, bytes=w * h * 24, us_at_8TBps=round(floor_us, 2),
                **timed(full, args.batch, args.repeats))
            say(what="resolve", viewport=[w, h], outputs="records", per_pixel=per_pixel, **timed(recs, args.batch, args.repeats))
        if args.only in ("", "merge"):  # (c) next to nv_depth_merge
            for k in (1, 2, 8):
                vs = [torch.randint(0, 1 << 62, (h, w), dtype=torch.int64, device=dev) for _ in range(k + 1)]
                ds = [torch.rand((h, w), dtype=torch.float32, device=dev) for _ in range(k + 1)]
                say(what="visibility_merge", viewport=[w, h], sources=k, bytes=(k + 2) * w * h * 8,
                    **timed(lambda: pipe.ctx.visibility_merge(vs[0], vs[1:], w, h), args.batch, args.repeats))
                say(what="depth_merge", viewport=[w, h], sources=k, bytes=(k + 2) * w * h * 4,
                    **timed(lambda: pipe.ctx.depth_merge(ds[0], ds[1:], w, h), args.batch, args.repeats))
        pipe.ctx.status()
        pipe.ctx.close()
        plain.ctx.close()


if __name__ == "__main__":
    main()
