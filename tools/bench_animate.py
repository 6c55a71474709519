#!/usr/bin/env python3
"""The numbers of the device keyframe evaluation (profiles/r21_animation.md); prints one JSON line.

    python3 tools/bench_animate.py [--repeats 15] [--draws 13,125000,1000000] [--keyframes 4]

Every draw of an nv_synth_draws set over the occluder scene's two meshes is animated (synth.orbit_animations).  By HIP events around the
calls (launch gaps included), cache-cold (a 512 MiB buffer is rewritten before every run), the alternatives alternated in one process:
  fused       nv_animate_draws on the registered draw buffer: records and cull mirror in one launch (the shipped form)
  unfused     nv_animate_draws of a context with nothing registered (the instantiation without the mirror), then nv_update_draws over the
              whole range: the pair the fused form has to match
  fused_tlas  fused, then nv_rt_tlas_build: what VisibilityPipeline.animate enqueues with a dynamic ray-tracing scene
  host_path   what the library offered before: the host twin's evaluation (wall time), then the records copied to the device,
              nv_update_draws over all of them and nv_rt_tlas_build (wall time around a synchronise: move_draws(0, all records))
Before anything is timed the two device forms are compared byte for byte (records) and by an early drawcull's output (mirror)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BYTES_PER_ANIMATION = 24 + 4 * 16 + 2 * 16 + 16 + 16 + 24  # record, two keyframes (four 16-byte words), the draw's two stores, its ids word, the Mesh's sphere, the mirror's two stores


def _stats(us):
    t = sorted(us)
    return dict(us_median=round(t[len(t) // 2], 2), us_min=round(t[0], 2), us_max=round(t[-1], 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--draws", default="13,125000,1000000")
    ap.add_argument("--keyframes", type=int, default=4)
    args = ap.parse_args()
    import numpy as np
    import torch

    from niagara_amd import host, synth
    from niagara_amd import layouts as L
    from niagara_amd import pipeline as P

    s = synth.occluder_scene_indexed()
    meshes = s["meshes"]
    static = host.rt_scene_build(meshes, s["indices"], s["vertices"], s["draws"])
    ctx, bare = P.Context(), P.Context()  # `bare` registers nothing: its nv_animate_draws is the instantiation without the mirror
    dev = ctx.device
    flush = torch.zeros(512 << 20, dtype=torch.uint8, device=dev)
    mb = P.to_device(meshes, dev)
    ctx.upload_meshes(mb, len(meshes))
    line = dict(repeats=args.repeats, keyframes_per_animation=args.keyframes, bytes_per_animation=BYTES_PER_ANIMATION)

    def events(fn, cold=True):
        if cold:
            flush.add_(1)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3

    for n in (int(v) for v in args.draws.split(",") if v):
        draws = host.synth_draws(n, len(meshes))
        host.assign_visibility_offsets(draws, meshes)
        anims, keys = synth.orbit_animations(draws, np.arange(n), args.keyframes, seed=7)
        db = P.to_device(draws, dev)
        ctx.reserve(n)
        ctx.upload_draws(db, n, mb)
        ctx.rt_scene_upload(static)
        ctx.rt_scene_reserve_dynamic(n)
        ctx.upload_animations(anims, keys, n)
        bare.upload_animations(anims, keys, n)
        cd = host.build_cull_data(draw_count=n, draw_distance=200.0, cullingEnabled=1, lodEnabled=1)
        dcb = torch.zeros((n + 64) * L.DRAWCMD.itemsize, dtype=torch.uint8, device=dev)
        dccb, dvb = torch.zeros(4, dtype=torch.int32, device=dev), torch.ones(n, dtype=torch.int32, device=dev)

        def cull():
            dccb.zero_()
            ctx.drawcull(cd, 0, 0, db, mb, dcb, dccb, dvb, None)
            k = int(dccb[0].item())
            return k, dcb[:k * L.DRAWCMD.itemsize].cpu().numpy().tobytes()
        fused = lambda t=1.3: ctx.animate_draws(t, db, n)

        def unfused(t=1.3):
            bare.animate_draws(t, db, n)
            ctx.update_draws(db, 0, n)

        def fused_tlas(t=1.3):
            ctx.animate_draws(t, db, n)
            ctx.rt_tlas_build(db, n)
        # ---- the two forms give the same records and the same mirror
        fused()
        rec_f, cull_f = db.cpu().numpy().tobytes(), cull()
        db.copy_(P.to_device(draws, dev))
        ctx.update_draws(db, 0, n)
        unfused()
        rec_u, cull_u = db.cpu().numpy().tobytes(), cull()
        twin = draws.copy()
        t0 = time.perf_counter()
        host.animate_draws_host(1.3, anims, keys, twin)
        host_eval_ms = (time.perf_counter() - t0) * 1e3
        got = np.frombuffer(rec_f, L.MESHDRAW)
        checks = dict(records_equal=bool(rec_f == rec_u), drawcull_equal=bool(cull_f == cull_u), commands=cull_f[0],
                      positions_equal_host_twin=bool(got["position"].tobytes() == twin["position"].tobytes()),
                      orientation_max_abs_diff_host_twin=float(np.abs(got["orientation"].astype(np.float64) - twin["orientation"]).max()))
        times = dict(fused=[], unfused=[], fused_tlas=[])
        for r in range(args.repeats):
            t = 0.37 * (r + 1)
            for name, fn in (("fused", fused), ("unfused", unfused), ("fused_tlas", fused_tlas)):
                times[name].append(events(lambda: fn(t)))
        host_path = []
        size = L.MESHDRAW.itemsize
        for r in range(min(args.repeats, 5)):
            rec = draws.copy()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host.animate_draws_host(0.37 * (r + 1), anims, keys, rec)
            t1 = time.perf_counter()
            db.view(torch.uint8).reshape(-1)[:n * size].copy_(P.to_device(rec, dev).view(torch.uint8).reshape(-1))
            ctx.update_draws(db, 0, n)
            ctx.rt_tlas_build(db, n)
            torch.cuda.synchronize()
            host_path.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
        f = _stats(times["fused"])
        line["draws_%d" % n] = dict(animations=n, checks=checks, fused=f, unfused=_stats(times["unfused"]), fused_tlas=_stats(times["fused_tlas"]),
                                    fused_gb_per_s=round(n * BYTES_PER_ANIMATION / (f["us_median"] * 1e-6) / 1e9, 1),
                                    host_eval_ms=round(sorted(h[0] for h in host_path)[len(host_path) // 2], 3),
                                    host_copy_update_tlas_ms=round(sorted(h[1] for h in host_path)[len(host_path) // 2], 3),
                                    host_eval_first_ms=round(host_eval_ms, 3))
        ctx.status()
        bare.status()
        del db, dcb, dvb
    print(json.dumps(line), flush=True)
    ctx.close()
    bare.close()


if __name__ == "__main__":
    main()
