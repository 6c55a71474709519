#!/usr/bin/env python3
"""Timings of the classic path's textured entry points on one GPU at 1920 x 1080, one JSON line per case.

    python3 tools/bench_classic_textures.py [--repeats 15] [--rounds 3]

Every sample is ONE call of an entry point between two HIP events (launch gaps included: an upper bound of the kernel time), cache-cold: a
512 MiB buffer, larger than the last-level cache, is overwritten before it.  The entry points of a case alternate sample by sample
(a, b, c, a, b, c, ...), so a drift of the machine falls on all of them; a figure is the median over --repeats samples, per round.

  attributes   nv_visibility_attributes_indexed (factors only), nv_visibility_attributes_indexed_textured, ..._indexed_blocks, and
               nv_visibility_attributes_textured over the cluster path's records of the same image (the cut-out occluder scene's frame);
  raster       the post launch: nv_rasterdepth_indexed_visibility, nv_rasterdepth_indexed_textured, ..._indexed_blocks, and
               nv_rasterdepth_textured over the same draws' clusters — the cut-out wall alone (64- and 1024-texel sets) and the 512 distant
               walls of profiles/r19_alpha_coverage.md at NV_OPT_RASTER_SMALL_LIMIT 16 and 0; targets cleared before every sample."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import oracle  # noqa: E402
from niagara_amd import host, synth  # noqa: E402
from niagara_amd import layouts as L  # noqa: E402
from niagara_amd import pipeline as P  # noqa: E402

W, H = 1920, 1080


def alternated(fns, repeats, rounds, flush, reset=None):
    """{name: [median us of each round]} and {name: min us}: the entry points in turn, each sample cache-cold"""
    for fn in fns.values():
        fn()
    med, low = {k: [] for k in fns}, {k: float("inf") for k in fns}
    for _ in range(rounds):
        us = {k: [] for k in fns}
        for r in range(repeats):
            for k, fn in fns.items():
                if reset:
                    reset()
                flush.fill_(r)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                us[k].append(a.elapsed_time(b) * 1e3)
        for k in fns:
            med[k].append(round(statistics.median(us[k]), 1))
            low[k] = round(min(low[k], min(us[k])), 1)
    return med, low


def commands_of(s, meshes, draw_ids):
    c = np.zeros(len(draw_ids), L.DRAWCMD)
    for k, d in enumerate(draw_ids):
        mesh = meshes[int(s["draws"][d]["meshIndex"])]
        c[k]["drawId"], c[k]["instanceCount"], c[k]["vertexOffset"] = d, 1, mesh["vertexOffset"]
        c[k]["firstIndex"], c[k]["indexCount"] = mesh["lods"][0]["indexOffset"], mesh["lods"][0]["indexCount"]
    return c


def bench_raster(args, flush):
    import raster_alpha_ref as RA
    ctx = P.Context()
    dev = ctx.device
    ctx.set_option(P.NV_OPT_RASTER_VISIBILITY_ID, 1)

    def case(name, s, list_draws, size, limit):
        t = synth.with_textures(s, size=size, cutout=True)
        draws = t["draws"].copy()
        draws["postPass"][list_draws] = 1
        draws["materialIndex"][list_draws] = 0
        t["draws"] = draws
        indices, meshes = synth.indexed_geometry(t["meshes"], t["meshlets"], t["data"])
        offsets = host.assign_triangle_offsets(draws, meshes)
        icmd = commands_of(t, meshes, list_draws)
        commands, cib_h, cc4_h = RA.draw_list(t, list_draws)
        cd = t["cull"].copy()
        cd["postPass"] = 1
        g = synth.make_globals(cd, (W, H))
        descs, texels = ctx.texture_decode(t["textures"])
        bdescs, bbuf = ctx.texture_blocks(t["textures"])
        mat = P.to_device(t["materials"], dev)
        tex = dict(materials=mat, material_count=len(t["materials"]), textures=P.to_device(descs, dev), texture_count=len(descs), texels=texels,
                   texel_words=texels.numel())
        btex = dict(materials=mat, material_count=len(t["materials"]), textures=P.to_device(bdescs, dev), texture_count=len(bdescs), blocks=bbuf,
                    units16=bbuf.numel() // 16)
        cl = [P.to_device(a, dev) for a in (commands, draws, t["meshlets"], t["data"], t["vertices"], cib_h, cc4_h)]
        ix = (P.to_device(icmd, dev), P.to_device(np.array([len(icmd), 0, 0, 0], np.uint32), dev), cl[1], len(draws), P.to_device(indices, dev), len(indices),
              cl[4], len(t["vertices"]))
        ob = P.to_device(offsets, dev)
        ctx.reserve(len(draws))
        depth = torch.zeros((H, W), dtype=torch.float32, device=dev)
        vis = torch.zeros((H, W), dtype=torch.int64, device=dev)
        tot, alpha = torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
        fns = dict(indexed_visibility=lambda: ctx.rasterdepth_indexed_visibility(g, *ix, depth, W, H, ob, vis),
                   indexed_textured=lambda: ctx.rasterdepth_indexed_textured(g, *ix, depth, W, H, ob, vis, **tex),
                   indexed_blocks=lambda: ctx.rasterdepth_indexed_blocks(g, *ix, depth, W, H, ob, vis, **btex),
                   cluster_textured=lambda: ctx.rasterdepth_textured(g, *cl, depth, W, H, vis, **tex))

        def reset():
            depth.zero_()
            vis.zero_()
        ctx.set_option(P.NV_OPT_RASTER_SMALL_LIMIT, limit)
        med, low = alternated(fns, args.repeats, args.rounds, flush, reset)
        reset()
        ctx.rasterdepth_indexed_textured(g, *ix, depth, W, H, ob, vis, tot, alpha_totals2=alpha, **tex)
        k, a2 = [int(x) for x in tot.cpu().numpy()], [int(x) for x in alpha.cpu().numpy()]
        want = depth.cpu().numpy().tobytes()
        reset()
        ctx.rasterdepth_textured(g, *cl, depth, W, H, vis, **tex)
        same = want == depth.cpu().numpy().tobytes()
        ctx.status()
        ctx.set_option(P.NV_OPT_RASTER_SMALL_LIMIT, 16)
        print(json.dumps(dict(what="raster", case=name, texture_side=size, small_limit=limit, commands=k[0], triangles=k[1], rasterised=k[2], kept=k[3],
                              dropped=a2[0], unevaluated=a2[1], us_median=med, us_min=low, depth_equals_cluster_path=same)), flush=True)

    wall = synth.occluder_scene(viewport=(W, H), box_scale=3.0, meshlet_bounds=oracle.meshlet_bounds)
    case("wall_1080p_64", wall, [int(d) for d in wall["wall"]], 64, 16)
    case("wall_1080p_1024", wall, [int(d) for d in wall["wall"]], 1024, 16)
    far = dict(wall)
    rng = np.random.default_rng(5)
    d = np.zeros(512, L.MESHDRAW)
    d["orientation"], d["scale"], d["meshIndex"] = (0.0, 0.0, 0.0, 1.0), wall["draws"]["scale"][0], 0
    dist = rng.uniform(200.0, 300.0, 512)
    d["position"] = np.stack([rng.uniform(-1.2, 1.2, 512) * dist, rng.uniform(-0.7, 0.7, 512) * dist, -dist], 1)
    far["draws"] = d
    host.assign_visibility_offsets(far["draws"], far["meshes"])
    for limit in (16, 0):
        case("far_walls_limit_%d" % limit, far, list(range(512)), 256, limit)
    ctx.close()


def bench_attributes(args, flush):
    s = synth.with_textures(synth.occluder_scene_indexed(viewport=(W, H), box_scale=3.0, meshlet_bounds=oracle.meshlet_bounds), size=args.texture_size,
                            cutout=True)
    s["draws"] = s["draws"].copy()
    s["draws"]["postPass"][s["wall"]] = 1
    rng = np.random.default_rng(3)
    v = s["vertices"].copy()
    v["np"], v["tp"] = rng.integers(0, 1 << 31, len(v)), rng.integers(0, 1 << 16, len(v))
    s["vertices"] = v
    kw = dict(task_capacity=4096, cluster_capacity=4096 * 64, vertices=v, indices=s["indices"], meshlet_data=s["data"], stable_ids=True)
    g = synth.make_globals(s["cull"], (W, H))
    n = W * H
    for resident in ("decoded",):
        pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], fused=True, **kw)
        pipe.set_textures(s["textures"])
        dev, c = pipe.ctx.device, pipe.ctx
        records = {}
        for task in (True, False):
            vis = pipe.new_visibility()
            for _ in range(2):
                pipe.frame(s["cull"], post_pass=True, visibility=vis, task=task, textures=True, materials=s["materials"])
            records[task] = pipe.resolve(s["cull"], vis, classic=not task)["records"]
        mat = P.to_device(s["materials"], dev)
        nm = len(s["materials"])
        bdescs, bbuf = c.texture_blocks(s["textures"])
        btable = P.to_device(bdescs, dev)
        _, tset = pipe._texture_set()
        attr = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
        g0, g1 = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2))
        tot = torch.zeros(4, dtype=torch.int64, device=dev)
        ix = (pipe.db, pipe.draw_count, pipe.ib, pipe.index_count, pipe.vb, pipe.vertex_count, mat, nm, attr, g0, g1)
        fns = dict(indexed=lambda: c.visibility_attributes_indexed(g, records[False], W, H, *ix),
                   indexed_textured=lambda: c.visibility_attributes_indexed_textured(g, records[False], W, H, *ix, None, *tset),
                   indexed_blocks=lambda: c.visibility_attributes_indexed_blocks(g, records[False], W, H, *ix, None, btable, len(bdescs), bbuf, bbuf.numel() // 16),
                   cluster_textured=lambda: c.visibility_attributes_textured(g, records[True], W, H, pipe.db, pipe.draw_count, pipe.mlb, pipe.meshlet_count, pipe.mdb,
                                                                             pipe.mdb.numel() * pipe.mdb.element_size() // 4, pipe.vb, pipe.vertex_count, mat, nm,
                                                                             attr, g0, g1, None, *tset))
        med, low = alternated(fns, args.repeats, args.rounds, flush)
        c.visibility_attributes_indexed_textured(g, records[False], W, H, *ix, tot, *tset)
        a = (attr.cpu().numpy().tobytes(), g0.cpu().numpy().tobytes(), g1.cpu().numpy().tobytes())
        fns["cluster_textured"]()
        same = a == (attr.cpu().numpy().tobytes(), g0.cpu().numpy().tobytes(), g1.cpu().numpy().tobytes())
        c.status()
        print(json.dumps(dict(what="attributes", viewport=[W, H], texture_side=args.texture_size, shaded=int(tot[0].item()), not_sampled=int(tot[3].item()),
                              us_median=med, us_min=low, outputs_equal_cluster_path=same)), flush=True)
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--texture-size", type=int, default=1024)
    ap.add_argument("--only", choices=("attributes", "raster"), default=None)
    args = ap.parse_args()
    flush = torch.zeros(512 << 20, dtype=torch.uint8, device="cuda")
    if args.only in (None, "attributes"):
        bench_attributes(args, flush)
    if args.only in (None, "raster"):
        bench_raster(args, flush)


if __name__ == "__main__":
    main()
