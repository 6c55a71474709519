#!/usr/bin/env python3
"""Timings of the visibility buffer's attribute pass (nv_visibility_attributes) on one GPU, one JSON line per scene and size.

    python3 tools/bench_attributes.py                      # product library: the per-run form
    NV_LIBRARY_PATH=niagara_amd/libniagara_vis_exp.so NV_ATTRIBUTES_PER_PIXEL=1 python3 tools/bench_attributes.py    # the per-pixel form

Every figure is the median over --repeats batches of device-event time around --batch back-to-back launches, divided by the batch
(launch gaps included: an upper bound of the kernel time; profiles/r12_visattr.md has the kernel trace).  The records are those of the
closed-loop frame of synth.occluder_scene / synth.interior_scene at the given viewport; the vertices' packed normals, tangents and
texcoords and the material table are random bits (they cost what real ones cost).  --once runs one launch per configuration and no
timing loop: the run to put under a kernel trace.

    python3 tools/bench_attributes.py --textures --sizes 1920x1080

--textures gives the occluder scene synth.with_textures' four 1024 x 1024 BC1 textures (--texture-size) and times, on the same records,
nv_visibility_attributes (outputs "all") and nv_visibility_attributes_textured, cache-cold: a buffer larger than the last-level cache is
overwritten between the timed launches (one launch per sample, not a batch), as the untextured rows of this mode are too.  It then times
nv_texture_decode per format on a 2048 x 2048 chain and prints GB/s of RGBA8 written.

    python3 tools/bench_attributes.py --textures --blocks --sizes 1920x1080 [--random-format 7]

--blocks adds nv_visibility_attributes_blocks over the block-resident form of the same set: its samples alternate with the decoded entry
point's (decoded, blocks, decoded, ...; each cache-cold), the outputs of the two are compared byte for byte, and the resident bytes of both
forms are printed.  --random-format fills the four maps with random blocks of one format (BC7: every mode), to time that format's decode."""
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
    ap.add_argument("--textures", action="store_true")
    ap.add_argument("--texture-size", type=int, default=1024)
    ap.add_argument("--blocks", action="store_true", help="with --textures: also time nv_visibility_attributes_blocks, alternating with the decoded entry point")
    ap.add_argument("--random-format", type=int, default=0, choices=(0, 1, 2, 3, 7),
                    help="with --textures: replace the four maps by random blocks of this NV_FORMAT_* (0: keep synth.with_textures' BC1 images)")
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

    if args.textures:
        return textures_mode(args, bounds)
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


def timed_cold(fn, repeats, flush):
    """one launch per sample behind a write of `flush` (larger than the last-level cache): the launch starts cache-cold"""
    import torch
    fn()
    out = []
    for k in range(repeats):
        flush.fill_(k)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return dict(us_median=round(statistics.median(out), 2), us_min=round(min(out), 2), us_max=round(max(out), 2))


def alternated_cold(fns, names, repeats, flush):
    """timed_cold for several launches whose samples alternate (a, b, a, b, ...): a drift of the machine lands on all of them alike"""
    import torch
    for fn in fns:
        fn()
    out = {n: [] for n in names}
    for k in range(repeats):
        for n, fn in zip(names, fns):
            flush.fill_(k)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            out[n].append(a.elapsed_time(b) * 1e3)
    return {n + "_us": dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2)) for n, v in out.items()}


def textures_mode(args, bounds):
    import ctypes as C

    import numpy as np
    import torch

    from niagara_amd import host
    from niagara_amd import layouts as L
    from niagara_amd import pipeline as P
    from niagara_amd import synth
    from niagara_amd._lib import TextureDesc, check, lib
    rng = np.random.default_rng(3)
    for size in args.sizes.split(","):
        w, h = (int(x) for x in size.split("x"))
        s = synth.occluder_scene(viewport=(w, h), meshlet_bounds=bounds)
        v = s["vertices"].copy()
        v["np"], v["tp"] = rng.integers(0, 1 << 31, len(v)), rng.integers(0, 1 << 16, len(v))
        v["tu"], v["tv"] = ((rng.random(len(v)) * 4).astype(np.float16).view(np.uint16) for _ in range(2))
        s["vertices"] = v
        s = synth.with_textures(s, size=args.texture_size)
        if args.random_format:
            fmt = args.random_format
            side, levels = args.texture_size, args.texture_size.bit_length()
            code = {1: 71, 2: 74, 3: 77, 7: 98}[fmt]
            files = []
            for _ in range(4):
                head = np.zeros(37, np.uint32)
                head[0], head[1], head[3], head[4], head[7], head[19], head[20], head[21] = 0x20534444, 124, side, side, levels, 32, 4, 0x30315844
                head[32], head[33], head[35] = code, 3, 1
                nbytes = sum(((max(1, side >> l) + 3) // 4) ** 2 for l in range(levels)) * (8 if fmt == 1 else 16)
                payload = rng.integers(0, 256, nbytes, dtype=np.uint8)
                if fmt == 7:
                    payload[0::16] |= 1 << 7  # a mode bit in every first byte: modes 0..7 by the lowest set bit, none reserved
                files.append(head.tobytes() + payload.tobytes())
            s["textures"] = files
        mats = s["materials"]
        pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], task_capacity=4096, cluster_capacity=4096 * 64, fused=True,
                                    vertices=v, meshlet_data=s["data"], stable_ids=True)
        vis = pipe.new_visibility()
        for _ in range(2):
            pipe.frame(s["cull"], post_pass=True, visibility=vis)
        records = pipe.resolve(s["cull"], vis)["records"]
        c, dev = pipe.ctx, pipe.ctx.device
        mat = P.to_device(mats, dev)
        g = synth.make_globals(s["cull"], (w, h))
        attr = torch.zeros(w * h * 64, dtype=torch.uint8, device=dev)
        g0, g1 = (torch.zeros(w * h, dtype=torch.int32, device=dev) for _ in range(2))
        tot = torch.zeros(4, dtype=torch.int64, device=dev)
        flush = torch.zeros(512 << 20, dtype=torch.uint8, device=dev)
        args_ = (g, records, w, h, pipe.db, pipe.draw_count, pipe.mlb, pipe.meshlet_count, pipe.mdb, pipe.mdb.numel() // 4, pipe.vb, pipe.vertex_count, mat,
                 len(mats), attr, g0, g1, tot)
        rows = [("nv_visibility_attributes", lambda: c.visibility_attributes(*args_))]
        descs, texels = c.texture_decode(s["textures"])
        table = P.to_device(descs, dev)
        rows.append(("nv_visibility_attributes_textured", lambda: c.visibility_attributes_textured(*args_, table, len(descs), texels, texels.numel())))
        for name, fn in rows:
            tot.zero_()
            fn()
            c.status()
            t = tot.cpu().numpy()
            rec = dict(what=name, scene="occluder, textured", viewport=[w, h], shaded=int(t[0]), unsampled=int(t[3]), texture_size=args.texture_size, cold=True)
            if not args.once:
                rec.update(timed_cold(fn, args.repeats, flush))
            print(json.dumps(rec), flush=True)
        if args.blocks:
            bdescs, blocks = c.texture_blocks(s["textures"])
            btable = P.to_device(bdescs, dev)
            decoded = rows[1][1]
            block_fn = lambda: c.visibility_attributes_blocks(*args_, btable, len(bdescs), blocks, blocks.numel() // 16)
            outs = []
            for fn in (decoded, block_fn):
                for t_ in (attr, g0, g1, tot):
                    t_.zero_()
                fn()
                c.status()
                outs.append([t_.cpu().numpy().tobytes() for t_ in (attr, g0, g1, tot)])
            rec = dict(what="blocks against decoded", scene="occluder, textured", viewport=[w, h], texture_size=args.texture_size, random_format=args.random_format,
                       outputs_equal=outs[0] == outs[1], decoded_bytes=int(texels.numel()) * 4, block_bytes=int(blocks.numel()), cold=True)
            if not args.once:
                rec.update(alternated_cold([decoded, block_fn], ["decoded", "blocks"], args.repeats, flush))
            print(json.dumps(rec), flush=True)
        if not args.once:
            side, levels = 2048, 12
            for fmt, code in ((L.FORMAT_BC1, 71), (L.FORMAT_BC2, 74), (L.FORMAT_BC3, 77), (L.FORMAT_BC7, 98)):
                head = np.zeros(37, np.uint32)
                head[0], head[1], head[3], head[4], head[7], head[19], head[20], head[21] = 0x20534444, 124, side, side, levels, 32, 4, 0x30315844
                head[32], head[33], head[35] = code, 3, 1
                blocks = sum(((max(1, side >> l) + 3) // 4) ** 2 for l in range(levels)) * (8 if fmt == L.FORMAT_BC1 else 16)
                payload = rng.integers(0, 256, blocks, dtype=np.uint8)
                if fmt == L.FORMAT_BC7:
                    payload[0::16] |= 1 << 6
                data = head.tobytes() + payload.tobytes()
                descs, words, infos = host.texture_set_layout([data])
                out = torch.zeros(words, dtype=torch.int32, device=dev)
                src = P.to_device(payload, dev)
                d = TextureDesc(*[int(descs[1][k]) for k in ("offset", "width", "height", "levels")])
                fn = lambda: check(lib.nv_texture_decode(c.h, P._stream(), P._ptr(src), fmt, side, side, levels, P._ptr(out), C.byref(d)), "nv_texture_decode")
                t = timed_cold(fn, args.repeats, flush)
                print(json.dumps(dict(what="nv_texture_decode", format=fmt, side=side, levels=levels, out_bytes=words * 4, **t,
                                      out_GBps=round(words * 4 / t["us_median"] / 1e3, 1))), flush=True)
        c.status()
        c.close()


if __name__ == "__main__":
    main()
