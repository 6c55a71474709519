#!/usr/bin/env python3
"""The numbers of the device TLAS rebuild (profiles/r16_tlas_build.md); prints one JSON line.

    python3 tools/bench_tlas.py [--repeats 15] [--draws 125000,1000000] [--viewport 1920x1080]

rebuild: nv_rt_tlas_build by HIP events around the whole call (its two memset nodes and all launches: launch gaps included), cache-cold (a
512 MiB buffer is rewritten before every run) and back to back, on the occluder scene's own draws and on nv_synth_draws sets over the same two
meshes; next to it the only path the library had before for moved draws, nv_rt_scene_build + nv_rt_scene_upload, as wall time in this
process.  The device result is compared with the host twin's bytes before anything is timed.  Per-launch times come from a kernel trace of
this tool (rocprofv3 --kernel-trace --stats -- python3 tools/bench_tlas.py): the entry point exposes no events between its launches.
trace: nv_shadow_trace on the occluder scene at --viewport over the depth target its own frames leave, walking the host's median-split TLAS
and the rebuilt radix-tree TLAS alternately (the same draws, the same mask), cache-cold; with the trees' surface-area cost (the sum of the
inner boxes' areas over the root's: the expected number of inner-node visits of a random line that meets the root)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _stats(us):
    t = sorted(us)
    return dict(us_median=round(t[len(t) // 2], 2), us_min=round(t[0], 2), us_max=round(t[-1], 2))


def _area_cost(blob):
    import numpy as np
    h = blob[:64].view(np.uint32)
    n, off = int(h[4]), int(h[9])
    if n == 0:
        return 0.0
    nodes = blob[off:off + 32 * n].view(np.float32).reshape(n, 8).astype(np.float64)
    leaf = blob[off:off + 32 * n].view(np.uint32).reshape(n, 8)[:, 7]
    e = np.maximum(nodes[:, 4:7] - nodes[:, 0:3], 0.0)
    area = e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2] + e[:, 2] * e[:, 0]
    return round(float(area[leaf == 0].sum() / area[0]), 3) if np.isfinite(area[0]) and area[0] > 0 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--draws", default="125000,1000000")
    ap.add_argument("--viewport", default="1920x1080")
    args = ap.parse_args()
    import numpy as np
    import torch

    from niagara_amd import host, synth
    from niagara_amd import layouts as L
    from niagara_amd import pipeline as P

    def bounds(vertices, data, meshlets):
        c = P.Context()
        mlb = P.to_device(meshlets, c.device)
        c.meshlet_bounds(P.to_device(vertices, c.device), P.to_device(data, c.device), mlb, len(meshlets))
        c.status()
        meshlets[:] = P.from_device(mlb, L.MESHLET)
        c.close()
    w, h = (int(v) for v in args.viewport.split("x"))
    s = synth.occluder_scene_indexed(meshlet_bounds=bounds, viewport=(w, h))
    pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], (w, h), fused=True, vertices=s["vertices"], meshlet_data=s["data"], stable_ids=True)
    vis = pipe.new_visibility()
    for _ in range(2):
        pipe.frame(s["cull"], post_pass=True, visibility=vis)
    ctx, dev = pipe.ctx, pipe.ctx.device
    flush = torch.zeros(512 << 20, dtype=torch.uint8, device=dev)
    line = dict(repeats=args.repeats)

    def events(fn, cold):
        if cold:
            flush.add_(1)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3

    # ---- rebuild time
    sets = [("occluder", s["draws"])] + [("synth_%d" % int(n), host.synth_draws(int(n), len(s["meshes"]))) for n in args.draws.split(",") if n]
    static = host.rt_scene_build(s["meshes"], s["indices"], s["vertices"], s["draws"])
    for name, draws in sets:
        n = len(draws)
        t0 = time.perf_counter()
        blob = host.rt_scene_build(s["meshes"], s["indices"], s["vertices"], draws)
        t1 = time.perf_counter()
        ctx.rt_scene_upload(blob)
        t2 = time.perf_counter()
        ctx.rt_scene_upload(static)
        ctx.rt_scene_reserve_dynamic(n)
        db = P.to_device(draws, dev)
        ctx.rt_tlas_build(db, n)
        got = ctx.rt_scene_download()
        t3 = time.perf_counter()
        want = host.rt_tlas_build_host(static, draws)
        t4 = time.perf_counter()
        run = lambda: ctx.rt_tlas_build(db, n)
        cold = [events(run, True) for _ in range(args.repeats)]
        warm = [events(run, False) for _ in range(args.repeats)]
        st = host.rt_scene_stats(got)
        line["rebuild_" + name] = dict(draws=n, instances=st["instances"], equals_host_twin=bool(got.tobytes() == want.tobytes()), cold=_stats(cold), warm=_stats(warm),
                                       host_build_ms=round((t1 - t0) * 1e3, 2), host_upload_ms=round((t2 - t1) * 1e3, 2),
                                       host_build_plus_upload_ms=round((t2 - t0) * 1e3, 2), host_twin_ms=round((t4 - t3) * 1e3, 2),
                                       area_cost_median_split=_area_cost(blob), area_cost_radix=_area_cost(got))
        del db

    # ---- trace time: the two TLAS over the occluder scene's own draws, alternately
    sun = np.array([2.0, 0.3, 1.0]) / np.linalg.norm([2.0, 0.3, 1.0])
    g = synth.make_globals(s["cull"], (w, h))
    mask = torch.zeros((h, w), dtype=torch.uint8, device=dev)
    db = P.to_device(s["draws"], dev)
    median, radix = P.Context(), ctx
    median.rt_scene_upload(static)
    radix.rt_scene_upload(static)
    radix.rt_scene_reserve_dynamic(len(s["draws"]))
    radix.rt_tlas_build(db, len(s["draws"]))
    for quality, checkerboard in ((1, 0), (0, 1)):
        sd = host.build_shadow_data(g, sun, 1e-2, checkerboard, w, h)
        masks, times = {}, dict(median_split=[], radix=[])
        for name, c in (("median_split", median), ("radix", radix)):
            mask.zero_()
            c.shadow_trace(sd, pipe.depth, mask, w, h, quality)  # warm-up
            masks[name] = mask.cpu().numpy().copy()
        for _ in range(args.repeats):
            for name, c in (("median_split", median), ("radix", radix)):
                times[name].append(events(lambda: c.shadow_trace(sd, pipe.depth, mask, w, h, quality), True))
        line["trace_q%d_cb%d" % (quality, checkerboard)] = dict(size="%dx%d" % (w, h), masks_equal=bool((masks["median_split"] == masks["radix"]).all()),
                                                              occluded=int((masks["radix"] == 0).sum()), median_split=_stats(times["median_split"]),
                                                              radix=_stats(times["radix"]))
    median.status()
    radix.status()
    median.close()
    print(json.dumps(line), flush=True)
    pipe.ctx.close()


if __name__ == "__main__":
    main()
