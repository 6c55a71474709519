"""nv_rasterdepth measurements: the raster over the 131 k-cluster list nv_trianglecull is timed on (bench_configs
config_n4: every meshlet of a 2048-draw pool once, 1920 x 1080) at several NV_OPT_RASTER_SMALL_LIMIT values, by HIP events around each
launch, with its totals and the split of the rasterised triangles between the lane and the wave path; and the closed-loop frame of
synth.occluder_scene (VisibilityPipeline.frame) against the same frame reduced from synthetic depth (synth.make_depth).
--only indexed: nv_rasterdepth_indexed on the kitten x 1024 draws at 1024 x 768, the same kitten geometry meshletised
(tests/meshlet_builder.py) through nv_rasterdepth on the same context, one 120 k-triangle draw, and the classic closed-loop frame
(VisibilityPipeline.frame(task=False)) on synth.occluder_scene_indexed.
--near-clip: the same workloads with NV_OPT_RASTER_NEAR_CLIP 1 (triangles crossing the near plane are clipped, not dropped).  --only loop also
times synth.interior_scene (the camera inside the geometry) with and without clipping, whatever the switch.

--only alpha: nv_rasterdepth_textured against nv_rasterdepth, alternated on one context: the post-phase launch of the cut-out
occluder scene at 1920 x 1080 (the wall alone: large triangles, the wave path) with a 64-texel set (magnified) and a 1024-texel set (minified,
two levels blended), and 512 distant instances of the wall (triangles of a few pixels) at NV_OPT_RASTER_SMALL_LIMIT 16 (a lane walks its own
triangle: divergent taps) and 0 (every triangle through the wave path).

    python tools/bench_raster.py [--iters N] [--only raster|loop|indexed|alpha] [--limits 0,16,...] [--near-clip]
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


def bench_interior(iters):
    """the closed-loop frame of synth.interior_scene with and without near-plane clipping, task and classic path: frame time, and what the late
    pass rejects"""
    s = synth.interior_scene_indexed(meshlet_bounds=oracle.meshlet_bounds)
    out = {}
    for task in (True, False):
        for near_clip in (False, True):
            pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], task_capacity=4096, cluster_capacity=4096 * 64, fused=True,
                                        meshlet_data=s["data"], vertices=s["vertices"], indices=s["indices"], near_clip=near_clip)
            for _ in range(4):
                pipe.frame(s["cull"], task=task)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                pipe.frame(s["cull"], task=task)
            torch.cuda.synchronize()
            us = (time.perf_counter() - t0) / iters * 1e6
            dvb = pipe.dvb.cpu().numpy()
            late = _lists(pipe)
            out["%s_%s" % ("cluster" if task else "classic", "clip" if near_clip else "noclip")] = dict(
                frame_us=us, draws=len(s["draws"]), draws_rejected=len(s["draws"]) - int(dvb.sum()), hidden_boxes_visible=int(dvb[s["hidden"]].sum()),
                late_commands=late[0], late_meshlets=late[1] if task else None, depth_covered=float((pipe.depth > 0).float().mean().item()))
            pipe.ctx.close()
    return out


def bench_loop(iters, near_clip=False):
    s = synth.occluder_scene(meshlet_bounds=oracle.meshlet_bounds)
    cd = s["cull"]
    w, h = s["viewport"]
    out = {}
    for mode in ("raster", "synthetic"):
        pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], task_capacity=4096, cluster_capacity=4096 * 64, fused=True,
                                    meshlet_data=s["data"], vertices=s["vertices"], near_clip=near_clip)
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
    out["interior"] = bench_interior(iters)
    return out


def _time(fn, iters, reset=None):
    """median / min microseconds per call by HIP events (reset() before each call, outside the events)"""
    for _ in range(3):
        if reset:
            reset()
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in ev:
        if reset:
            reset()
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
    return us[len(us) // 2], us[0]


def _rates(med, tot):
    return dict(us_median=med, triangles_per_s=tot[1] / (med * 1e-6), rasterised_per_s=tot[2] / (med * 1e-6), samples_per_s=tot[3] / (med * 1e-6),
                totals=dict(first=tot[0], triangles=tot[1], rasterised=tot[2], samples=tot[3]))


def bench_indexed(iters, near_clip=False):
    import meshlet_builder
    import raster_indexed_ref as RI
    ctx = P.Context()
    ctx.set_option(P.NV_OPT_RASTER_NEAR_CLIP, int(near_clip))
    dev = ctx.device
    out = {}
    # kitten x 1024 (BASELINE config 1's draws), every draw one command
    w, h = 1024, 768
    vertices, indices, positions = RI.kitten_geometry()
    n = 1024
    draws = host.synth_draws(n, 1, 300.0)
    cd = host.build_cull_data(draw_count=n, viewport=(w, h), cullingEnabled=1)
    g = synth.make_globals(cd, (w, h))
    cmds = RI.commands_for([(0, len(indices))] * n)
    dcb, db, ib, vb = P.to_device(cmds, dev), P.to_device(draws, dev), P.to_device(indices, dev), P.to_device(vertices, dev)
    dccb = P.to_device(np.array([n, 0, 0, 0], np.uint32), dev)
    depth = torch.zeros((h, w), dtype=torch.float32, device=dev)
    totals = torch.zeros(4, dtype=torch.int64, device=dev)

    def indexed():
        ctx.rasterdepth_indexed(g, dcb, dccb, db, n, ib, len(indices), vb, len(vertices), depth, w, h)

    med, mn = _time(indexed, iters, depth.zero_)
    depth.zero_()
    ctx.rasterdepth_indexed(g, dcb, dccb, db, n, ib, len(indices), vb, len(vertices), depth, w, h, totals)
    out["kitten_x1024"] = dict(_rates(med, [int(x) for x in totals.cpu().numpy()]), us_min=mn, viewport=[w, h])
    d_indexed = depth.cpu().numpy().copy()
    # the same triangles through the cluster path
    meshlets, data, mvert = meshlet_builder.build_meshlets(positions, indices.reshape(-1, 3).astype(np.int64))
    k = len(meshlets)
    per = (k + 63) // 64
    tc = np.zeros(n * per, dtype=L.TASKCMD)
    ids = []
    for d in range(n):
        for c in range(per):
            i = d * per + c
            tc[i]["drawId"], tc[i]["taskOffset"], tc[i]["taskCount"] = d, c * 64, min(64, k - c * 64)
            ids += [i | j << 24 for j in range(int(tc[i]["taskCount"]))]
    cc4_h = np.array([len(ids), 0, 0, 0], np.uint32)
    cib_h = np.concatenate([np.array(ids, np.uint32), np.zeros(512, np.uint32)])
    oracle.clustersubmit(cc4_h, cib_h)
    t = [P.to_device(a, dev) for a in (tc, draws, meshlets, data, mvert, cib_h, cc4_h)]

    def cluster():
        ctx.rasterdepth(g, *t, depth, w, h)

    med, mn = _time(cluster, iters, depth.zero_)
    depth.zero_()
    totals.zero_()
    ctx.rasterdepth(g, *t, depth, w, h, None, totals)
    out["kitten_x1024_cluster_path"] = dict(_rates(med, [int(x) for x in totals.cpu().numpy()]), us_min=mn, meshlets_per_draw=k,
                                            same_depth_bits=bool(depth.cpu().numpy().tobytes() == d_indexed.tobytes()))
    # one 120 k-triangle draw (the balance case)
    xs, ys = np.linspace(-6, 6, 301), np.linspace(-4, 4, 201)
    pos = np.array([(x, y, 0.0) for y in ys for x in xs], np.float32)
    i, j = np.meshgrid(np.arange(300), np.arange(200))
    a = (j * 301 + i).reshape(-1)
    big = np.stack([np.stack([a, a + 1, a + 302], 1), np.stack([a, a + 302, a + 301], 1)], 1).reshape(-1).astype(np.uint32)
    bv = np.zeros(len(pos), dtype=L.VERTEX)
    hp = pos.astype(np.float16)
    bv["vx"], bv["vy"], bv["vz"] = (hp[:, c].view(np.uint16) for c in range(3))
    bd = np.zeros(1, dtype=L.MESHDRAW)
    bd["position"], bd["scale"], bd["orientation"] = (0.3, -0.2, -5.0), 1.0, (0, 0, 0, 1)
    b_dcb, b_db, b_ib, b_vb = P.to_device(RI.commands_for([(0, len(big))]), dev), P.to_device(bd, dev), P.to_device(big, dev), P.to_device(bv, dev)
    b_dccb = P.to_device(np.array([1, 0, 0, 0], np.uint32), dev)

    def one():
        ctx.rasterdepth_indexed(g, b_dcb, b_dccb, b_db, 1, b_ib, len(big), b_vb, len(bv), depth, w, h)

    med, mn = _time(one, iters, depth.zero_)
    depth.zero_()
    totals.zero_()
    ctx.rasterdepth_indexed(g, b_dcb, b_dccb, b_db, 1, b_ib, len(big), b_vb, len(bv), depth, w, h, totals)
    out["one_draw_120k"] = dict(_rates(med, [int(x) for x in totals.cpu().numpy()]), us_min=mn)
    ctx.close()
    # the classic closed loop
    s = synth.occluder_scene_indexed(meshlet_bounds=oracle.meshlet_bounds)
    for task in (False, True):
        pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], task_capacity=4096, cluster_capacity=4096 * 64, fused=True,
                                    meshlet_data=s["data"], vertices=s["vertices"], indices=s["indices"], near_clip=near_clip)
        for _ in range(4):
            pipe.frame(s["cull"], task=task)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            pipe.frame(s["cull"], task=task)
        torch.cuda.synchronize()
        us = (time.perf_counter() - t0) / iters * 1e6
        dvb = pipe.dvb.cpu().numpy()
        out["loop_classic" if not task else "loop_cluster"] = dict(frame_us=us, draws=len(s["draws"]), hidden_boxes_visible=int(dvb[s["hidden"]].sum()),
                                                                   visible_draws=int(dvb.sum()))
        pipe.ctx.close()
    return out


def bench_alpha(iters):
    import raster_alpha_ref as RA
    ctx = P.Context()
    dev = ctx.device
    ctx.set_option(P.NV_OPT_RASTER_VISIBILITY_ID, 1)  # the frame's post phase writes the stable word
    w, h = 1920, 1080
    out = {}

    def case(name, s, list_draws, size, limit):
        t = synth.with_textures(s, size=size, cutout=True)
        draws = t["draws"].copy()
        draws["postPass"][list_draws] = 1
        draws["materialIndex"][list_draws] = 0
        t["draws"] = draws
        commands, cib_h, cc4_h = RA.draw_list(t, list_draws)
        cd = t["cull"].copy()
        cd["postPass"] = 1
        g = synth.make_globals(cd, (w, h))
        descs, texels = ctx.texture_decode(t["textures"])
        dev_args = [P.to_device(a, dev) for a in (commands, draws, t["meshlets"], t["data"], t["vertices"], cib_h, cc4_h)]
        mat, table = P.to_device(t["materials"], dev), P.to_device(descs, dev)
        depth = torch.zeros((h, w), dtype=torch.float32, device=dev)
        vis = torch.zeros((h, w), dtype=torch.int64, device=dev)
        tot, alpha = torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
        tex = dict(materials=mat, material_count=len(t["materials"]), textures=table, texture_count=len(descs), texels=texels, texel_words=texels.numel())
        plain = lambda totals=None: ctx.rasterdepth(g, *dev_args, depth, w, h, vis, totals)
        textured = lambda totals=None, a2=None: ctx.rasterdepth_textured(g, *dev_args, depth, w, h, vis, totals, alpha_totals2=a2, **tex)
        # the same pass over the block-resident form of the set
        bdescs, bbuf = ctx.texture_blocks(t["textures"])
        btex = dict(materials=mat, material_count=len(t["materials"]), textures=P.to_device(bdescs, dev), texture_count=len(bdescs), blocks=bbuf,
                    units16=bbuf.numel() // 16)
        blocks = lambda totals=None, a2=None: ctx.rasterdepth_blocks(g, *dev_args, depth, w, h, vis, totals, alpha_totals2=a2, **btex)

        def reset():  # every launch starts from cleared targets
            depth.zero_()
            vis.zero_()
        ctx.set_option(P.NV_OPT_RASTER_SMALL_LIMIT, limit)
        rounds = [(_time(plain, iters, reset), _time(textured, iters, reset), _time(blocks, iters, reset)) for _ in range(3)]  # alternated
        reset()
        plain(tot)
        p = [int(x) for x in tot.cpu().numpy()]
        tot.zero_()
        reset()
        textured(tot, alpha)
        k, a2 = [int(x) for x in tot.cpu().numpy()], [int(x) for x in alpha.cpu().numpy()]
        want = (depth.cpu().numpy().tobytes(), vis.cpu().numpy().tobytes(), k, a2)
        tot.zero_()
        alpha.zero_()
        reset()
        blocks(tot, alpha)
        same = want == (depth.cpu().numpy().tobytes(), vis.cpu().numpy().tobytes(), [int(x) for x in tot.cpu().numpy()], [int(x) for x in alpha.cpu().numpy()])
        ctx.status()
        ctx.set_option(P.NV_OPT_RASTER_SMALL_LIMIT, 16)
        out[name] = dict(texture_side=size, small_limit=limit, clusters=p[0], triangles=p[1], rasterised=p[2], samples=p[3], kept=k[3], dropped=a2[0],
                         unevaluated=a2[1], plain_us_median=[r[0][0] for r in rounds], textured_us_median=[r[1][0] for r in rounds],
                         blocks_us_median=[r[2][0] for r in rounds], plain_us_min=min(r[0][1] for r in rounds), textured_us_min=min(r[1][1] for r in rounds),
                         blocks_us_min=min(r[2][1] for r in rounds), blocks_equal_textured=same, decoded_bytes=int(texels.numel()) * 4,
                         block_bytes=int(bbuf.numel()))

    wall = synth.occluder_scene(viewport=(w, h), box_scale=3.0, meshlet_bounds=oracle.meshlet_bounds)
    case("wall_1080p_64", wall, wall["wall"], 64, 16)
    case("wall_1080p_1024", wall, wall["wall"], 1024, 16)
    # 512 instances of the wall, far away and small: triangles of a few pixels
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
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--only", choices=("raster", "loop", "indexed", "alpha"), default=None)
    ap.add_argument("--limits", default="0,4,9,16,32,64,%d" % INT_MAX)
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--near-clip", action="store_true", help="NV_OPT_RASTER_NEAR_CLIP 1 on every context")
    a = ap.parse_args()
    res = dict(near_clip=bool(a.near_clip))
    if a.only in (None, "raster"):
        ctx = P.Context()
        ctx.set_option(P.NV_OPT_RASTER_NEAR_CLIP, int(a.near_clip))
        res["raster"] = bench_raster(ctx, a.iters, [int(x) for x in a.limits.split(",")], split=not a.no_split)
        ctx.close()
    if a.only in (None, "loop"):
        res["loop"] = bench_loop(a.iters, a.near_clip)
    if a.only in (None, "indexed"):
        res["indexed"] = bench_indexed(a.iters, a.near_clip)
    if a.only == "alpha":
        res["alpha"] = bench_alpha(a.iters)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
