"""nv_rasterdepth measurements: the raster over the 131 k-cluster list nv_trianglecull is timed on (bench_configs
config_n4: every meshlet of a 2048-draw pool once, 1920 x 1080) at several NV_OPT_RASTER_SMALL_LIMIT values, by HIP events around each
launch, with its totals and the split of the rasterised triangles between the lane and the wave path; and the closed-loop frame of
synth.occluder_scene (VisibilityPipeline.frame) against the same frame reduced from synthetic depth (synth.make_depth).

    python tools/bench_raster.py [--iters N] [--only raster|loop] [--limits 0,16,...]
Kernel-trace times: rocprofv3 --kernel-trace --stats -d OUT -o raster -- python tools/bench_raster.py --only raster
Prints one JSON object."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import oracle  # noqa: E402
from niagara_amd import host, synth  # noqa: E402
from niagara_amd import layouts as L  # noqa: E402
from niagara_amd import pipeline as P  # noqa: E402

INT_MAX = 2 ** 31 - 1


def path_split(g, commands, draws, meshlets, data, vertices, cib, cc4, w, h, limits):
    """rasterised triangles per path for each limit: the setup rules of DESIGN.md §4.10 in numpy over the reference's vertex stage (the
    near-plane rule read as z <= 1 on the quotient: a statistic, not a parity check)"""
    import raster_ref as RR
    import tempfile
    rr = RR.load(tempfile.mkdtemp(prefix="raster_ref"))
    vx = rr.vertices(g, commands, draws, meshlets, data, vertices, cib, cc4)  # (slots, 64, {sx, sy, w, z})
    d8 = data.view(np.uint8)
    sizes = []
    for k in range(len(vx)):
        ci = int(cib[k])
        if ci == 0xffffffff:
            continue
        m = meshlets[int(commands[ci & 0xffffff]["taskOffset"]) + (ci >> 24)]
        ve, te = min(int(m["vertexCount"]), 64), min(int(m["triangleCount"]), 96)
        io = (int(m["dataOffset"]) + ((int(m["vertexCount"]) + 1) // 2 if m["shortRefs"] == 1 else int(m["vertexCount"]))) * 4
        idx = d8[io:io + 3 * te].reshape(-1, 3).astype(np.int64)
        v = vx[k]
        with np.errstate(invalid="ignore"):
            bad = ~((v[:, 2] > 0) & (v[:, 3] <= 1.0)) | ~(np.abs(v[:, 0]) < 2 ** 21) | ~(np.abs(v[:, 1]) < 2 ** 21)
        X = np.where(bad, 0, np.rint(v[:, 0] * 256)).astype(np.int64)
        Y = np.where(bad, 0, h * 256 - np.rint(v[:, 1] * 256)).astype(np.int64)
        ok = (idx < ve).all(axis=1)
        idx = np.where(idx < 64, idx, 0)
        ok &= ~bad[idx].any(axis=1)
        a, b, c = idx[:, 0], idx[:, 1], idx[:, 2]
        A = (X[b] - X[a]) * (Y[c] - Y[a]) - (Y[b] - Y[a]) * (X[c] - X[a])
        ok &= A < 0  # postPass 0: front faces only
        xs, ys = X[idx], Y[idx]
        x0 = np.maximum((xs.min(1) - 128 + 255) >> 8, 0)
        x1 = np.minimum((xs.max(1) - 128) >> 8, w - 1)
        y0 = np.maximum((ys.min(1) - 128 + 255) >> 8, 0)
        y1 = np.minimum((ys.max(1) - 128) >> 8, h - 1)
        n = np.where((x1 >= x0) & (y1 >= y0), (x1 - x0 + 1) * (y1 - y0 + 1), 0)
        sizes.append(n[ok])
    n = np.concatenate(sizes) if sizes else np.zeros(0, np.int64)
    return {str(lim): dict(lane=int(((n > 0) & (n <= lim)).sum()), wave=int((n > lim).sum())) for lim in limits}, \
        dict(box_pixels_p50=float(np.percentile(n, 50)) if len(n) else 0.0, box_pixels_p90=float(np.percentile(n, 90)) if len(n) else 0.0,
             box_pixels_max=int(n.max()) if len(n) else 0, empty_boxes=int((n == 0).sum()))


def bench_raster(ctx, iters, limits, split=True):
    dev = ctx.device
    w, h = 1920, 1080
    draws, meshlets, commands, n = synth.cluster_scene(2048, 1, seed=9, scene_radius=60.0)
    data, vertices = synth.make_geometry(meshlets, seed=11)
    cd = host.build_cull_data(draw_count=2048, viewport=(w, h), cullingEnabled=1)
    g = synth.make_globals(cd, (w, h))
    m = n * 64
    ids = (np.arange(m, dtype=np.uint32) // 64) | ((np.arange(m, dtype=np.uint32) % 64) << 24)
    cib_h = np.concatenate([ids, np.zeros(512, np.uint32)])
    cc4_h = np.array([m, 0, 0, 0], np.uint32)
    oracle.clustersubmit(cc4_h, cib_h)
    db, mlb, dcb = P.to_device(draws, dev), P.to_device(meshlets, dev), P.to_device(commands, dev)
    dd, vb, cib, ccb = P.to_device(data, dev), P.to_device(vertices, dev), P.to_device(cib_h, dev), P.to_device(cc4_h, dev)
    depth = torch.zeros((h, w), dtype=torch.float32, device=dev)
    totals = torch.zeros(4, dtype=torch.int64, device=dev)
    out = dict(clusters=m, viewport=[w, h], limits={})
    for lim in limits:
        ctx.set_option(P.NV_OPT_RASTER_SMALL_LIMIT, lim)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        for i in range(3):
            depth.zero_()
            ctx.rasterdepth(g, dcb, db, mlb, dd, vb, cib, ccb, depth, w, h)
        for e0, e1 in ev:
            depth.zero_()  # every launch starts from a cleared target (an early pass)
            e0.record()
            ctx.rasterdepth(g, dcb, db, mlb, dd, vb, cib, ccb, depth, w, h)
            e1.record()
        torch.cuda.synchronize()
        us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
        totals.zero_()
        ctx.rasterdepth(g, dcb, db, mlb, dd, vb, cib, ccb, depth, w, h, None, totals)
        t = [int(x) for x in totals.cpu().numpy()]
        med = us[len(us) // 2]
        out["limits"][str(lim)] = dict(us_median=med, us_min=us[0], clusters_per_s=t[0] / (med * 1e-6), triangles_per_s=t[1] / (med * 1e-6),
                                       samples_per_s=t[3] / (med * 1e-6))
        out["totals"] = dict(clusters=t[0], triangles=t[1], rasterised=t[2], samples=t[3])
    ctx.set_option(P.NV_OPT_RASTER_SMALL_LIMIT, 16)
    if split:
        out["path_split"], out["boxes"] = path_split(g, commands, draws, meshlets, data, vertices, cib_h, cc4_h, w, h, limits)
    return out


def _lists(pipe):
    cc4 = pipe.ccb.cpu().numpy().view(np.uint32)
    c4 = pipe.dccb.cpu().numpy().view(np.uint32)
    return int(c4[0]), int(cc4[0])


def bench_loop(iters):
    s = synth.occluder_scene(meshlet_bounds=oracle.meshlet_bounds)
    cd = s["cull"]
    w, h = s["viewport"]
    out = {}
    for mode in ("raster", "synthetic"):
        pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], task_capacity=4096, cluster_capacity=4096 * 64, fused=True,
                                    meshlet_data=s["data"], vertices=s["vertices"])
        synth_depth = torch.from_numpy(synth.make_depth(w, h)).to(pipe.ctx.device)

        def frame():
            if mode == "raster":
                pipe.frame(cd)
            else:  # the same frame with the pyramid reduced from a fixed synthetic target
                pipe.cull(cd, late=False)
                pipe.render_clusters(cd, late=False)
                pipe.build_pyramid(synth_depth)
                pipe.cull(cd, late=True)
                pipe.render_clusters(cd, late=True)

        for _ in range(4):  # past the first frames: steady state
            frame()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            frame()
        torch.cuda.synchronize()
        us = (time.perf_counter() - t0) / iters * 1e6
        # one more frame, phase by phase, for the counts
        pipe.cull(cd, late=False)
        pipe.render_clusters(cd, late=False)
        early = _lists(pipe)
        if mode == "raster":
            pipe.render_depth(cd, late=False)
            pipe.build_pyramid(pipe.depth)
        else:
            pipe.build_pyramid(synth_depth)
        pipe.cull(cd, late=True)
        pipe.render_clusters(cd, late=True)
        late = _lists(pipe)
        visible = int(pipe.dvb.cpu().numpy().sum())
        out[mode] = dict(frame_us=us, draws=len(s["draws"]), meshlets=len(s["meshlets"]), early_commands=early[0], early_meshlets=early[1],
                         late_commands=late[0], late_meshlets=late[1], visible_draws_after_late=visible,
                         draws_rejected=len(s["draws"]) - visible, hidden_boxes_visible=int(pipe.dvb.cpu().numpy()[s["hidden"]].sum()))
        pipe.ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--only", choices=("raster", "loop"), default=None)
    ap.add_argument("--limits", default="0,4,9,16,32,64,%d" % INT_MAX)
    ap.add_argument("--no-split", action="store_true")
    a = ap.parse_args()
    res = {}
    if a.only in (None, "raster"):
        ctx = P.Context()
        res["raster"] = bench_raster(ctx, a.iters, [int(x) for x in a.limits.split(",")], split=not a.no_split)
        ctx.close()
    if a.only in (None, "loop"):
        res["loop"] = bench_loop(a.iters)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
