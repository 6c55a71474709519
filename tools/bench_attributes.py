#!/usr/bin/env python3
"""Timings of the visibility buffer's attribute pass (nv_visibility_attributes) on one GPU, one JSON line per scene and size.

    python3 tools/bench_attributes.py                      # product library: the per-run form
    NV_LIBRARY_PATH=niagara_amd/libniagara_vis_exp.so NV_ATTRIBUTES_PER_PIXEL=1 python3 tools/bench_attributes.py    # the per-pixel form

Every figure is the median over --repeats batches of device-event time around --batch back-to-back launches, divided by the batch
(launch gaps included: an upper bound of the kernel time; profiles/r12_visattr.md has the kernel trace).  The records are those of the
closed-loop frame of synth.occluder_scene / synth.interior_scene at the given viewport; the vertices' packed normals, tangents and
texcoords and the material table are random bits (they cost what real ones cost).  --once runs one launch per configuration and no
timing loop: the run to put under a kernel trace."""
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
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--sizes", default="1920x1080,4096x4096")
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

    rng = np.random.default_rng(3)
    per_pixel = os.environ.get("NV_ATTRIBUTES_PER_PIXEL", "0") != "0"
    for size in args.sizes.split(","):
        w, h = (int(x) for x in size.split("x"))
        for name in ("occluder", "interior"):
            s = synth.occluder_scene(viewport=(w, h), meshlet_bounds=bounds) if name == "occluder" else synth.interior_scene(viewport=(w, h), meshlet_bounds=bounds)
            v = s["vertices"].copy()
            v["np"], v["tp"] = rng.integers(0, 1 << 31, len(v)), rng.integers(0, 1 << 16, len(v))
            v["tu"], v["tv"] = (rng.random(len(v)).astype(np.float16).view(np.uint16) for _ in range(2))
            draws = s["draws"].copy()
            draws["materialIndex"] = np.arange(len(draws)) % 5
            mats = np.zeros(5, L.MATERIAL)
            mats["diffuseFactor"], mats["specularFactor"], mats["emissiveFactor"] = rng.random((5, 4)), rng.random((5, 4)), rng.random((5, 3))
            pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], draws, s["viewport"], task_capacity=4096, cluster_capacity=4096 * 64, fused=True,
                                        vertices=v, meshlet_data=s["data"], stable_ids=True, near_clip=name == "interior")
            vis = pipe.new_visibility()
            for _ in range(2):
                pipe.frame(s["cull"], post_pass=True, visibility=vis)
            records = pipe.resolve(s["cull"], vis)["records"]
            dev = pipe.ctx.device
            mat = P.to_device(mats, dev)
            g = synth.make_globals(s["cull"], (w, h))
            attr = torch.zeros(w * h * 64, dtype=torch.uint8, device=dev)
            g0, g1 = (torch.zeros(w * h, dtype=torch.int32, device=dev) for _ in range(2))
            tot = torch.zeros(4, dtype=torch.int64, device=dev)
            c = pipe.ctx

            def launch(attributes, gbuffers):
                c.visibility_attributes(g, records, w, h, pipe.db, pipe.draw_count, pipe.mlb, pipe.meshlet_count, pipe.mdb, pipe.mdb.numel() // 4, pipe.vb,
                                        pipe.vertex_count, mat, len(mats), attr if attributes else None, g0 if gbuffers else None, g1 if gbuffers else None, tot)
            launch(True, True)
            c.status()
            shaded = int(tot[0].item())
            for outputs, a_, g_ in (("all", True, True), ("gbuffers", False, True), ("attributes", True, False)):
                nbytes = w * h * (16 + (64 if a_ else 0) + (8 if g_ else 0))
                rec = dict(what="attributes", scene=name, viewport=[w, h], outputs=outputs, per_pixel=per_pixel, shaded=shaded, bytes=nbytes,
                           us_at_8TBps=round(nbytes / 8e12 * 1e6, 2))
                if args.once:
                    launch(a_, g_)
                    c.status()
                else:
                    t = timed(lambda: launch(a_, g_), args.batch, args.repeats)
                    rec.update(t, fraction_of_8TBps=round(nbytes / 8e12 * 1e6 / t["us_median"], 3))
                print(json.dumps(rec), flush=True)
            c.status()
            c.close()


if __name__ == "__main__":
    main()
