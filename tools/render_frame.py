#!/usr/bin/env python3
"""A displayable image out of a scene on one GPU: synth.occluder_scene through frame(visibility=) -> resolve -> attributes -> shade
(DESIGN.md §4.12-4.15).  A demonstration, not a test.

    python3 tools/render_frame.py --out frame.ppm                       # the scene at its own viewport, a synthetic shadow mask
    python3 tools/render_frame.py --no-shadow --viewport 1920x1080
    python3 tools/render_frame.py --bloom                               # two materials emit; the bloom chain and final's bloom term
    python3 tools/render_frame.py --traced-shadows                      # the mask is ray traced (nv_shadow_trace)
    python3 tools/render_frame.py --traced-shadows --animate 8          # 8 images, one box on a circle: its shadow follows (§4.17)
    python3 tools/render_frame.py --alpha-shadows                       # the wall is a cut-out in the post pass: its shadow has holes (§4.19)
    python3 tools/render_frame.py --alpha-coverage --alpha-shadows      # and so has the wall: the boxes behind it show through (§4.20)
    python3 tools/render_frame.py --classic [--bloom]                   # the classic path's frame: indexed draws, their visibility buffer (§4.23)
    python3 tools/render_frame.py --classic --alpha-coverage            # the same frame textured, the wall a cut-out in the post pass (§4.24)

Writes a binary PPM (P6, R G B from the R8G8B8A8 colour words) and prints one JSON line with the passes' times by HIP events (one run
each after a warm-up frame: launch gaps included, an upper bound of the kernel time; profiles/r13_shade.md has the kernel trace).
--passes WxH[,WxH...] instead times the three shade passes alone on synthetic images of those sizes, cache-cold (a 512 MiB buffer is
rewritten between the passes): the run to put under a kernel trace.  With --bloom it times the bloom passes instead: pass 0, every level
of passes 1 and 2, the whole chain per level and with the fused tail (NV_OPT_BLOOM_FUSED_TAIL) alternately — the A/B — and final with the
bloom term (profiles/r14_bloom.md).  --traced-shadows --passes shadow_trace times nv_shadow_trace alone on the scene at --viewport over the
depth target its own frames leave, both qualities, with and without checkerboard, cache-cold (profiles/r15_shadowtrace.md)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _timed(events, name, fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    events.append((name, a, b))
    return out


def passes(sizes, repeats, bloom=False):
    """the three shade passes (or, with `bloom`, the bloom passes) on synthetic images, each launch behind a flush of the caches"""
    import numpy as np
    import torch

    from niagara_amd import host, synth
    from niagara_amd import pipeline as P
    ctx = P.Context()
    dev = ctx.device
    flush = torch.zeros(512 << 20, dtype=torch.uint8, device=dev)
    for w, h in sizes:
        rng = np.random.default_rng(w + h)
        x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
        depth = torch.from_numpy((0.1 / (4.0 + x / w + y / h)).astype(np.float32)).to(dev)
        g0 = torch.from_numpy(rng.integers(0, 1 << 31, (h, w), dtype=np.int64).astype(np.int32)).to(dev)
        g1 = torch.from_numpy(rng.integers(0, 1 << 31, (h, w), dtype=np.int64).astype(np.int32)).to(dev)
        shadow = torch.from_numpy(rng.integers(0, 256, (h, w)).astype(np.uint8)).to(dev)
        tmp, color = torch.zeros_like(shadow), torch.zeros((h, w), dtype=torch.int32, device=dev)
        cd = host.build_cull_data(viewport=(w, h), pyramid=(host.previous_pow2(w), host.previous_pow2(h)))
        sd = {k: host.build_shade_data(synth.make_globals(cd, (w, h)), (0, 0, 0), (0.35, 0.6, 0.72), k, w, h) for k in (0, 1)}
        n = w * h
        if bloom:
            # an emissive block in a G-buffer without emission; the passes' cost does not depend on the values
            g0 &= 0x00FFFFFF
            g0[h // 4:h // 2, w // 4:w // 2] |= 0x60000000
            d = host.bloom_desc(w, h)
            target = torch.zeros(d.totalTexels, dtype=torch.int32, device=dev)
            size = lambda i: max(1, d.width >> i) * max(1, d.height >> i)
            runs = dict(bloom_extract=lambda: ctx.bloom_extract(g0, w, h, target, d))
            algorithmic = dict(bloom_extract=n * 4 + size(0) * 4)
            for i in range(1, d.levels):
                runs["bloom_downsample_%d" % i] = lambda i=i: ctx.bloom_downsample(target, d, i)
                algorithmic["bloom_downsample_%d" % i] = (size(i - 1) + size(i)) * 4
            for i in range(d.levels - 2, -1, -1):
                runs["bloom_upsample_%d" % i] = lambda i=i: ctx.bloom_upsample(target, d, i, 2.0)
                algorithmic["bloom_upsample_%d" % i] = (size(i + 1) + 2 * size(i)) * 4
            chain_bytes = sum(algorithmic.values())

            def fused_chain():
                ctx.set_option(P.NV_OPT_BLOOM_FUSED_TAIL, 1)
                try:
                    ctx.bloom(g0, w, h, target, d)
                finally:
                    ctx.set_option(P.NV_OPT_BLOOM_FUSED_TAIL, 0)
            # the A/B of the fused tail: the two forms of the whole chain, measured alternately (ab below)
            runs["bloom_chain"] = lambda: ctx.bloom(g0, w, h, target, d)
            runs["bloom_chain_fused_tail"] = fused_chain
            algorithmic["bloom_chain"] = algorithmic["bloom_chain_fused_tail"] = chain_bytes
            runs["shade_final_bloom"] = lambda: ctx.shade_final_bloom(sd[1], g0, g1, depth, shadow, color, w, h, target, d)
            algorithmic["shade_final_bloom"] = n * 17 + size(0) * 4
            ab = ("bloom_chain", "bloom_chain_fused_tail")
        else:
            runs = dict(shadow_fill=lambda: ctx.shadow_fill(shadow, depth, w, h, 1), shadow_blur_h=lambda: ctx.shadow_blur(tmp, shadow, depth, w, h, 1, 0.1),
                        shadow_blur_v=lambda: ctx.shadow_blur(shadow, tmp, depth, w, h, 0, 0.1),
                        shade_final_shadow=lambda: ctx.shade_final(sd[1], g0, g1, depth, shadow, color, w, h),
                        shade_final=lambda: ctx.shade_final(sd[0], g0, g1, depth, None, color, w, h))
            algorithmic = dict(shadow_fill=(n // 2) * (5 * 4 + 4 + 1), shadow_blur_h=n * (4 + 1 + 1), shadow_blur_v=n * (4 + 1 + 1), shade_final_shadow=n * 17,
                               shade_final=n * 16)
            ab = ()
        line = dict(size="%dx%d" % (w, h))
        def measure(name):
            flush.add_(1)
            ev = []
            _timed(ev, name, runs[name])
            torch.cuda.synchronize()
            return ev[0][1].elapsed_time(ev[0][2]) * 1e3
        times = {name: [] for name in runs}
        for name, fn in runs.items():
            fn()  # warm-up
            if name not in ab:
                times[name] = [measure(name) for _ in range(repeats)]
        for _ in range(repeats):  # the A/B pair: alternating, so that a drift of the box hits both alike
            for name in ab:
                times[name].append(measure(name))
        for name in runs:
            t = sorted(times[name])
            line[name] = dict(us_median=round(t[len(t) // 2], 2), us_min=round(t[0], 2), us_max=round(t[-1], 2), bytes=algorithmic[name],
                              us_at_8TBs=round(algorithmic[name] / 8e12 * 1e6, 2))
        print(json.dumps(line), flush=True)
    ctx.status()
    ctx.close()


def _scene(args, indexed):
    """the occluder scene at the asked viewport with its meshlet bounds computed on the device"""
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
    kw = dict(meshlet_bounds=bounds)
    if args.viewport:
        kw["viewport"] = tuple(int(v) for v in args.viewport.split("x"))
    return synth.occluder_scene_indexed(**kw) if indexed else synth.occluder_scene(**kw)


def trace_passes(args):
    """nv_shadow_trace alone: the scene's own depth target (two closed-loop frames), every launch behind a flush of the caches"""
    import numpy as np
    import torch

    from niagara_amd import host, synth
    from niagara_amd import pipeline as P
    s = _scene(args, True)
    w, h = s["viewport"]
    pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], (w, h), fused=True, vertices=s["vertices"], meshlet_data=s["data"], stable_ids=True)
    vis = pipe.new_visibility()
    for _ in range(2):
        pipe.frame(s["cull"], post_pass=True, visibility=vis)
    if args.alpha_shadows:
        alpha_passes(args, s, pipe)
        return
    blob = pipe.build_rt_scene(s["meshes"], s["indices"], s["vertices"], s["draws"])
    ctx, dev = pipe.ctx, pipe.ctx.device
    flush = torch.zeros(512 << 20, dtype=torch.uint8, device=dev)
    mask = torch.zeros((h, w), dtype=torch.uint8, device=dev)
    sun = np.array([2.0, 0.3, 1.0]) / np.linalg.norm([2.0, 0.3, 1.0])
    g = synth.make_globals(s["cull"], (w, h))
    line = dict(size="%dx%d" % (w, h), covered=int((pipe.depth > 0).sum().item()), scene=host.rt_scene_stats(blob))
    for quality in (0, 1):
        for checkerboard in (0, 1):
            for jitter in (0.0, 1e-2):
                sd = host.build_shadow_data(g, sun, jitter, checkerboard, w, h)
                run = lambda: ctx.shadow_trace(sd, pipe.depth, mask, w, h, quality)
                run()  # warm-up
                times = []
                for _ in range(args.repeats):
                    flush.add_(1)
                    ev = []
                    _timed(ev, "shadow_trace", run)
                    torch.cuda.synchronize()
                    times.append(ev[0][1].elapsed_time(ev[0][2]) * 1e3)
                warm = []  # back to back: the scene and the depth target stay in the caches
                for _ in range(args.repeats):
                    ev = []
                    _timed(ev, "shadow_trace", run)
                    torch.cuda.synchronize()
                    warm.append(ev[0][1].elapsed_time(ev[0][2]) * 1e3)
                t, tw = sorted(times), sorted(warm)
                rays = ((w + 1) // 2 if checkerboard else w) * h
                line["shadow_trace_q%d_cb%d_jitter%g" % (quality, checkerboard, jitter)] = dict(
                    us_median=round(t[len(t) // 2], 2), us_min=round(t[0], 2), us_max=round(t[-1], 2), us_warm_median=round(tw[len(tw) // 2], 2),
                    us_warm_min=round(tw[0], 2), us_warm_max=round(tw[-1], 2), rays=rays, occluded=int((mask == 0).sum().item()))
    print(json.dumps(line), flush=True)
    ctx.status()
    ctx.close()


def alpha_passes(args, s, pipe):
    """--alpha-shadows --passes shadow_trace: nv_shadow_trace_textured against nv_shadow_trace at quality 1 on the same scene blob and depth target,
    the wall a cut-out in the post pass; alternating, every launch behind a flush of the caches"""
    import numpy as np
    import torch

    from niagara_amd import host, synth
    from niagara_amd import pipeline as P
    w, h = s["viewport"]
    t = synth.with_textures(dict(vertices=s["vertices"], draws=s["draws"]), cutout=True)
    draws = t["draws"].copy()
    draws["postPass"][s["wall"]] = 1
    ctx, dev = pipe.ctx, pipe.ctx.device
    pipe.set_textures(t["textures"])
    blob = ctx.rt_scene_build(s["meshes"], s["indices"], t["vertices"], draws, texcoords=True)
    ctx.rt_scene_upload(blob)
    db, mat = P.to_device(draws, dev), P.to_device(t["materials"], dev)
    flush = torch.zeros(512 << 20, dtype=torch.uint8, device=dev)
    mask = torch.zeros((h, w), dtype=torch.uint8, device=dev)
    sun = np.array([2.0, 0.3, 1.0]) / np.linalg.norm([2.0, 0.3, 1.0])
    sd = host.build_shadow_data(synth.make_globals(s["cull"], (w, h)), sun, 0.0, 0, w, h)
    runs = dict(opaque=lambda: ctx.shadow_trace(sd, pipe.depth, mask, w, h, 1),
                alpha=lambda: ctx.shadow_trace_textured(sd, pipe.depth, mask, w, h, 1, db, len(draws), mat, len(t["materials"]), pipe.texture_table,
                                                        len(pipe.texture_descs), pipe.texels, pipe.texels.numel()))
    if args.block_textures:  # the same trace over the block-resident form of the set, in the same alternation
        bdescs, blocks = ctx.texture_blocks(t["textures"])
        btable = P.to_device(bdescs, dev)
        runs["blocks"] = lambda: ctx.shadow_trace_blocks(sd, pipe.depth, mask, w, h, 1, db, len(draws), mat, len(t["materials"]), btable, len(bdescs), blocks,
                                                         blocks.numel() // 16)
    line = dict(size="%dx%d" % (w, h), covered=int((pipe.depth > 0).sum().item()), scene=host.rt_scene_stats(blob))
    times = {name: [] for name in runs}
    for name, run in runs.items():
        run()  # warm-up
        line["occluded_" + name] = int((mask == 0).sum().item())
        line["mask_sum_" + name] = int(mask.sum(dtype=torch.int64).item())
    for _ in range(args.repeats):
        for name, run in runs.items():
            flush.add_(1)
            ev = []
            _timed(ev, name, run)
            torch.cuda.synchronize()
            times[name].append(ev[0][1].elapsed_time(ev[0][2]) * 1e3)
    for name, v in times.items():
        v = sorted(v)
        line["shadow_trace_" + name] = dict(us_median=round(v[len(v) // 2], 2), us_min=round(v[0], 2), us_max=round(v[-1], 2))
    print(json.dumps(line), flush=True)
    ctx.status()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="frame.ppm")
    ap.add_argument("--viewport", default=None, help="WxH (default: the scene's own, 320x192)")
    ap.add_argument("--no-shadow", action="store_true")
    ap.add_argument("--checkerboard", action="store_true")
    ap.add_argument("--bloom", action="store_true", help="two materials emit; run the bloom chain and final's bloom term")
    ap.add_argument("--textures", action="store_true", help="synth.with_textures' checker albedo, bump normal map, specular and emissive maps through "
                    "nv_visibility_attributes_textured (DESIGN.md §4.18)")
    ap.add_argument("--block-textures", action="store_true", help="--textures with the set block-resident (set_textures(resident=\"blocks\"), DESIGN.md §4.21): every "
                    "textured pass decodes its taps from the BC blocks; the image equals the decoded run's byte for byte")
    ap.add_argument("--traced-shadows", action="store_true", help="ray trace the shadow mask (the default stays the synthetic mask)")
    ap.add_argument("--alpha-shadows", action="store_true", help="--traced-shadows --textures with the wall in the post pass and a cut-out albedo: the trace "
                    "runs the alpha test (nv_shadow_trace_textured, DESIGN.md §4.19) and the wall's shadow has the checker's holes")
    ap.add_argument("--alpha-coverage", action="store_true", help="--textures with the wall in the post pass and a cut-out albedo: the post phase's raster runs the "
                    "fragment's alpha test (nv_rasterdepth_textured, DESIGN.md §4.20) and the boxes behind the wall's holes are in the image; alone or "
                    "with --alpha-shadows")
    ap.add_argument("--classic", action="store_true", help="the classic path (no mesh shading): frame(task=False, visibility=) over the indexed draws, "
                    "resolve(classic=True), attributes(classic=True), shade (DESIGN.md §4.23); with --textures / --block-textures the complete fragment "
                    "stage and with --alpha-coverage the alpha-tested indexed raster in the post phase (§4.24)")
    ap.add_argument("--quality", type=int, default=1, help="--traced-shadows: 0 = opaque draws cast, 1 = post-pass draws too")
    ap.add_argument("--animate", type=int, default=0, help="--traced-shadows: write N images (out_000.ppm ...) with one draw displaced along a circle "
                    "per frame through move_draws, which rebuilds the TLAS on the device")
    ap.add_argument("--keyframes", action="store_true", help="--animate: the circle as N keyframes of one animation, evaluated on the device by "
                    "animate(time) (nv_animate_draws, DESIGN.md §4.22) instead of records written on the host")
    ap.add_argument("--passes", default=None, help="WxH[,WxH...], or shadow_trace (with --traced-shadows)")
    ap.add_argument("--repeats", type=int, default=9)
    args = ap.parse_args()
    if args.alpha_shadows:
        args.traced_shadows = args.textures = True
    if args.alpha_coverage or args.block_textures:
        args.textures = True
    cutout = args.alpha_shadows or args.alpha_coverage
    if args.passes == "shadow_trace":
        if not args.traced_shadows:
            ap.error("--passes shadow_trace times the ray-traced pass: give --traced-shadows")
        trace_passes(args)
        return
    if args.passes:
        passes([tuple(int(v) for v in s.split("x")) for s in args.passes.split(",")], args.repeats, args.bloom)
        return
    import numpy as np
    import torch

    from niagara_amd import layouts as L
    from niagara_amd import pipeline as P

    s = _scene(args, args.traced_shadows or args.classic)  # the traced mask and the classic frame need the index buffer of the classic path
    w, h = s["viewport"]
    # attributes for the vertices and a material per draw: unit normals from the positions, colours by draw
    rng = np.random.default_rng(7)
    v = s["vertices"].copy()
    pos = np.stack([v["vx"], v["vy"], v["vz"]], -1).view(np.float16).astype(np.float64)
    nrm = pos / np.maximum(np.linalg.norm(pos, axis=1, keepdims=True), 1e-6)
    nrm[np.abs(pos[:, 2]) < 1e-3] = (0.0, 0.0, 1.0)  # the wall (a grid in z = 0) faces the camera
    q = np.clip(np.rint((nrm + 1.0) * 511.0), 0, 1022).astype(np.uint32)
    v["np"] = q[:, 0] | q[:, 1] << 10 | q[:, 2] << 20
    v["tp"] = 127 | 127 << 8
    draws = s["draws"].copy()
    materials = np.zeros(6, L.MATERIAL)
    materials["diffuseFactor"] = np.concatenate([rng.uniform(0.2, 0.95, (6, 3)), np.ones((6, 1))], 1).astype(np.float32)
    materials["specularFactor"][:, 3] = rng.uniform(0.1, 0.9, 6).astype(np.float32)
    if args.bloom:
        materials["emissiveFactor"][[1, 4]] = ((6.0, 2.5, 0.5), (0.5, 3.0, 8.0))
    draws["materialIndex"] = np.arange(len(draws)) % len(materials)
    textures = None
    if args.textures:
        from niagara_amd import synth
        t = synth.with_textures(dict(vertices=v, draws=draws, materials=materials), cutout=cutout)  # planar texcoords, the four maps, materials that name them
        v, materials, textures = t["vertices"], t["materials"], t["textures"]
    if cutout:
        draws["postPass"][s["wall"]] = 1  # both alpha tests see post-pass draws only (src/scenert.cpp:516, mesh.frag.glsl:88)
    pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], draws, (w, h), fused=True, vertices=v, meshlet_data=s["data"], stable_ids=True,
                                indices=s["indices"] if args.classic else None)
    if textures:
        pipe.set_textures(textures, resident="blocks" if args.block_textures else "decoded")
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    r = np.hypot(x - 0.45 * w, y - 0.5 * h) / (0.3 * h)
    mask = np.clip(np.rint(255.0 * np.clip((r - 0.8) / 0.4, 0.0, 1.0)), 0, 255).astype(np.uint8)
    sun = np.array([0.35, 0.6, 0.72]) / np.linalg.norm([0.35, 0.6, 0.72])
    mat = P.to_device(materials, pipe.ctx.device)
    if args.traced_shadows and not args.no_shadow:
        pipe.build_rt_scene(s["meshes"], s["indices"], v, draws, dynamic=args.animate > 0, texcoords=args.alpha_shadows)

    def frame(events):
        vis = pipe.new_visibility()
        _timed(events, "frame", lambda: pipe.frame(s["cull"], post_pass=True, visibility=vis, textures=args.alpha_coverage, materials=mat,
                                                   task=not args.classic))
        res = _timed(events, "resolve", lambda: pipe.resolve(s["cull"], vis, classic=args.classic))
        att = _timed(events, "attributes", lambda: pipe.attributes(s["cull"], res["records"], mat, attributes=False, textures=args.textures,
                                                                   classic=args.classic))
        shadow = None if args.no_shadow else "trace" if args.traced_shadows else torch.from_numpy(mask.copy()).to(pipe.ctx.device)
        return _timed(events, "shade", lambda: pipe.shade(s["cull"], att["gbuffer0"], att["gbuffer1"], (0.0, 0.0, 0.0), sun, shadow=shadow,
                                                          checkerboard=args.checkerboard, bloom=args.bloom, quality=args.quality,
                                                          textures=args.alpha_shadows and isinstance(shadow, str), materials=mat))
    def write(path, color, events, extra):
        words = color.cpu().numpy().view(np.uint32)
        rgb = np.stack([(words >> np.uint32(8 * k)) & np.uint32(255) for k in range(3)], -1).astype(np.uint8)
        with open(path, "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (w, h))
            f.write(rgb.tobytes())
        print(json.dumps(dict(out=path, viewport=[w, h], shadow=not args.no_shadow, traced=bool(args.traced_shadows and not args.no_shadow), bloom=args.bloom, classic=bool(args.classic),
                              covered=int((pipe.depth > 0).sum().item()), alpha_coverage=bool(args.alpha_coverage), mean_rgb=[round(float(c), 2) for c in rgb.reshape(-1, 3).mean(0)],
                              us={name: round(a.elapsed_time(b) * 1e3, 1) for name, a, b in events}, **extra)))
    frame([])  # warm-up (and the visibility bits of the closed loop)
    if args.animate > 0:
        if not (args.traced_shadows and not args.no_shadow):
            ap.error("--animate moves a draw under the traced shadows: give --traced-shadows")
        which = s["beside"][0]  # a box next to the wall, carried around the wall's edge: its shadow crosses the boxes behind
        home = draws[which:which + 1].copy()
        stem, ext = os.path.splitext(args.out)

        def circle(k):
            a = 2.0 * np.pi * k / args.animate
            rec = home.copy()
            rec["position"][0] = home["position"][0] + np.array([6.0 * np.cos(a) - 6.0, 6.0 * np.sin(a), 0.0], np.float32)
            return rec
        if args.keyframes:  # one keyframe per image, period 1: image k is the keyframe instant `time = k`
            keys = np.zeros(args.animate, L.KEYFRAME)
            for k in range(args.animate):
                keys["translation"][k], keys["scale"][k], keys["rotation"][k] = circle(k)["position"][0], home["scale"][0], home["orientation"][0]
            anim = np.zeros(1, L.ANIMATION)
            anim["drawIndex"], anim["lightIndex"], anim["period"], anim["keyframeCount"] = which, -1, 1.0, args.animate
            pipe.set_animations(anim, keys)
        for k in range(args.animate):
            rec = circle(k)
            events = []
            if args.keyframes:
                _timed(events, "animate", lambda: pipe.animate(float(k)))
            else:
                _timed(events, "move_draws", lambda: pipe.move_draws(which, rec))
            frame(events)  # the closed loop's visibility bits follow the move one frame late, as niagara's do
            color = frame(events)
            torch.cuda.synchronize()
            pipe.ctx.status()
            write("%s_%03d%s" % (stem, k, ext), color, events, dict(moved_draw=int(which), position=[round(float(c), 3) for c in rec["position"][0]],
                                                                     shadowed=int((pipe.shadow_image == 0).sum().item())))
        pipe.ctx.close()
        return
    events = []
    color = frame(events)
    torch.cuda.synchronize()
    pipe.ctx.status()
    write(args.out, color, events, {})
    pipe.ctx.close()


if __name__ == "__main__":
    main()
