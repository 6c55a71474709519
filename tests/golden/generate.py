#!/usr/bin/env python3
"""Generates tests/golden/*.npz from the REFERENCE'S OWN shader sources executing on the CPU (oracle/_ref, built by
`make -C oracle ref` from /root/reference/src/shaders/*.glsl).  Run in the build container, where the reference tree is
mounted; the fixtures travel with the repository, the reference does not.

    python tests/golden/generate.py

Each fixture stores the inputs (meshes, meshlets, draws, CullData, depth target, flags) and every buffer the
reference's passes leave behind over two frames of the early -> pyramid -> late protocol (src/niagara.cpp:1765-1788).

Sections of their own, each in a directory of its own: `--shade` (tests/golden/shade: the shading passes) and `--shadow`
(tests/golden/shadow: shadow.comp.glsl against a CPU ray query — masks per quality, the textured mask and the ray log; see
shadow_fixtures).  Without an argument everything is written.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import oracle.ref as R  # noqa: E402
import passes  # noqa: E402
from scenes import make_scene  # noqa: E402

CASES = [
    # name, scene kwargs, flags (cullingEnabled, lodEnabled, occlusionEnabled, clusterOcclusionEnabled, clusterBackfaceEnabled)
    ("all_on", dict(seed=101, n_draws=300, meshlets_lod0=130, zero_radius_fraction=0.02), (1, 1, 1, 1, 1)),
    ("no_cluster_occlusion", dict(seed=102, n_draws=300, meshlets_lod0=100), (1, 1, 1, 0, 1)),
    ("frustum_only", dict(seed=103, n_draws=400, meshlets_lod0=70, lods=1), (1, 0, 0, 0, 0)),
    ("culling_off_backface_off", dict(seed=104, n_draws=120, meshlets_lod0=90, random_camera=False), (0, 1, 1, 1, 0)),
]


def main():
    assert R.available(), "oracle/_ref is not built: run `make -C oracle ref` where /root/reference exists"
    for name, kw, flags in CASES:
        scene = make_scene(**kw)
        frames = passes.run_frames(R, scene, flags, frames=2)
        out = dict(meshes=scene["meshes"], meshlets=scene["meshlets"], draws=scene["draws"], cull=scene["cull"], depth=scene["depth"],
                   flags=np.array(flags, np.int32), slots=np.array([scene["slots"]], np.uint32), viewport=np.array(scene["viewport"], np.uint32))
        for f, rec in enumerate(frames):
            out["f%d_pyramid" % f] = rec["pyramid"]
            for phase in ("early", "late"):
                for key, val in rec[phase].items():
                    out["f%d_%s_%s" % (f, phase, key)] = val
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        vis = int(frames[0]["late"]["cc4"][0])
        print("%-28s %6d bytes, frame-0 late visible clusters: %d" % (name + ".npz", os.path.getsize(path), vis))


def mesh_fixture():
    """tests/golden/mesh/trianglecull.npz: inputs + the reference mesh shader's own triangle-cull decisions (MESH_CULL = 1)"""
    import test_trianglecull as T
    from scenes import make_triangle_scene
    s = make_triangle_scene(seed=77, n_draws=20, commands_per_draw=1, scene_radius=8.0, cam_pos=(1.0, 0.5, -2.0))
    cib, cc4 = T.cluster_list(R, s)
    masks, totals = T.run(R.meshlet_mesh, s, cib, cc4)
    os.makedirs(os.path.join(HERE, "mesh"), exist_ok=True)
    path = os.path.join(HERE, "mesh", "trianglecull.npz")
    np.savez_compressed(path, globals=s["globals"], commands=s["commands"], draws=s["draws"], meshlets=s["meshlets"], data=s["data"],
                        vertices=s["vertices"], cib=cib[:len(masks)], cc4=cc4, masks=masks, totals=totals)
    print("%-28s %6d bytes, clusters %d, triangles %d, kept %d" % ("mesh/trianglecull.npz", os.path.getsize(path), *totals))


def task_fixture():
    """tests/golden/mesh/taskcull.npz: task commands of a frame scene + what the reference TASK shader (meshlet.task.glsl, TASK_CULL = 1)
    emits for them in the early and in the late pass: EmitMeshTasksEXT counts, payload entries, visibility words"""
    scene = make_scene(seed=105, n_draws=900, meshlets_lod0=110, zero_radius_fraction=0.02)
    from oracle import Pyramid
    pyr = Pyramid(*scene["viewport"])
    R.depthreduce(scene["depth"], pyr)
    cd = passes.set_flags(scene["cull"], (1, 1, 1, 1, 1))
    cmds, c4 = passes.run_drawcull(R, scene, cd, 0, 1, np.ones(len(scene["draws"]), np.uint32), pyr)
    R.tasksubmit(c4, cmds)
    rng = np.random.default_rng(9)
    cmds["lateDrawVisibility"][:int(c4[0])] = rng.integers(0, 2, int(c4[0]))
    ncmd = int(c4[1]) * 64
    mvb0 = rng.integers(0, 2 ** 32, (scene["slots"] + 31) // 32 + 2, dtype=np.uint64).astype(np.uint32)
    out = dict(meshlets=scene["meshlets"], draws=scene["draws"], cull=cd, depth=scene["depth"], viewport=np.array(scene["viewport"], np.uint32),
               commands=cmds[:ncmd], count4=c4, mvb0=mvb0)
    for late in (0, 1):
        pay, cnt, mvb = np.zeros((ncmd, 64), np.uint32), np.zeros(ncmd, np.uint32), mvb0.copy()
        R.meshlet_task(cd, late, cmds, c4, scene["draws"], scene["meshlets"], mvb, pyr, pay, cnt)
        pay[np.arange(64)[None, :] >= cnt[:, None]] = 0  # entries past the emitted count are not part of the result
        out["late%d_payloads" % late], out["late%d_counts" % late], out["late%d_mvb" % late] = pay, cnt, mvb
    path = os.path.join(HERE, "mesh", "taskcull.npz")
    np.savez_compressed(path, **out)
    print("%-28s %6d bytes, %d commands, emitted early %d late %d" % ("mesh/taskcull.npz", os.path.getsize(path), ncmd, int(out["late0_counts"].sum()),
                                                                     int(out["late1_counts"].sum())))


def shade_fixtures():
    """tests/golden/shade/<w>x<h>.npz: the inputs of the shading passes at three image sizes (tests/shade_cases.py) and what the REFERENCE'S
    shaders, translated and run on the CPU (oracle/_ref), make of them: the stored words and the values handed to the stores of shadowfill,
    shadowblur, final (without and with a bloom image), the three bloom passes and the bloom loop, and the attachments and discard flags of
    mesh.frag over the records of one scene, factor-only and textured.  Data only.  A directory of its own: tests/test_golden.py reads the
    .npz files directly under tests/golden as cull scenes."""
    import tempfile

    import bloom_ref as BR
    import shade_cases as SC
    import texture_ref as TR
    import visattr_ref as VA
    os.makedirs(SC.GOLDEN, exist_ok=True)
    tmp = tempfile.mkdtemp()
    aref, tref = VA.load(tmp), TR.load(tmp)
    files, descs, texels = SC.frag_textures()
    total = 0
    for group, (w, h) in enumerate(SC.FIXTURE_SIZES):
        i = SC.pass_inputs(w, h)
        d = i["desc"]
        f = dict(depth=i["depth"], shadow=i["shadow"], gbuffer0=i["gbuffer0"], gbuffer1=i["gbuffer1"], znear=np.float32(i["znear"]),
                 sd=np.stack([np.frombuffer(sd.tobytes(), np.uint8) for sd in i["sd"]]), bloom_g0=i["bloom_g0"], levels=BR.pack(i["levels"]),
                 levels2=BR.pack(i["levels2"]), bloom0=SC.bloom_levels(w, h, seed=4)[0])
        for cb in (0, 1):
            words, handed = R.shadow_fill(i["shadow"], i["depth"], cb)
            f["fill%d_words" % cb], f["fill%d_value" % cb] = words, handed[..., 0]
        for direction in (0, 1):
            words, handed = R.shadow_blur(i["shadow"], i["depth"], direction, i["znear"])
            f["blur%d_words" % direction], f["blur%d_value" % direction] = words, handed[..., 0]
        for shadows in (0, 1):
            shadow = i["shadow"] if shadows else None
            words, handed = R.final(i["sd"][shadows], i["gbuffer0"], i["gbuffer1"], i["depth"], shadow)
            f["final%d_words" % shadows], f["final%d_value" % shadows] = words, handed[..., :3]
            words, handed = R.final(i["sd"][shadows], i["gbuffer0"], i["gbuffer1"], i["depth"], shadow, f["bloom0"])
            f["finalbloom%d_words" % shadows], f["finalbloom%d_value" % shadows] = words, handed[..., :3]
        words, handed = R.bloom_pass(0, i["bloom_g0"], d["sizes"][0][::-1])
        f["extract_words"], f["extract_value"] = words, handed[..., :3]
        down = [R.bloom_pass(1, i["levels"][l - 1], i["levels"][l].shape) for l in range(1, d["levels"])]
        f["down_words"] = BR.pack([i["levels"][0]] + [a for a, _ in down])  # (level 0 is not written by pass 1: the given words)
        f["down_value"] = np.concatenate([b[..., :3].reshape(-1, 3) for _, b in down])
        for k, radius in enumerate(SC.RADII):
            up = [R.bloom_pass(2, i["levels2"][l + 1], i["levels2"][l].shape, radius, dst=i["levels2"][l]) for l in range(d["levels"] - 1)]
            f["up%d_words" % k] = BR.pack([a for a, _ in up] + [i["levels2"][-1]])  # (the last level is not written by pass 2)
            f["up%d_value" % k] = np.concatenate([b[..., :3].reshape(-1, 3) for _, b in up])
        f["loop_words"] = R.bloom(i["bloom_g0"], d["width"], d["height"], d["levels"], d["offsets"], d["total"])
        s, rec = SC.frag_scene(w, h, group)
        f["records"], f["materials"], f["material_index"] = rec, s["materials"], s["draws"]["materialIndex"]
        plain = SC.untextured(s["materials"])
        want = aref.attributes(s["g"], rec, w, h, s["draws"], s["meshlets"], s["data"], s["vertices"], plain)
        out = R.mesh_frag(want["attributes"], w, s["draws"], plain, None, 1)
        f["frag_gbuffer0"], f["frag_gbuffer1"], f["frag_discard"] = out["gbuffer0"], out["gbuffer1"], out["discard"]
        want = tref.attributes(s["g"], rec, w, h, s["draws"], s["meshlets"], s["data"], s["vertices"], s["materials"], descs, texels, taps=True)
        out = R.mesh_frag(want["attributes"], w, s["draws"], s["materials"], want["taps"], 1)
        f["fragtex_gbuffer0"], f["fragtex_gbuffer1"], f["fragtex_discard"] = out["gbuffer0"], out["gbuffer1"], out["discard"]
        path = os.path.join(SC.GOLDEN, "%dx%d.npz" % (w, h))
        np.savez_compressed(path, **f)
        total += os.path.getsize(path)
        print("%-28s %6d bytes, %d arrays" % ("shade/%dx%d.npz" % (w, h), os.path.getsize(path), len(f)))
    kitten = os.path.getsize(os.path.join(HERE, "mesh", "kitten.npz"))
    assert total <= kitten, "the shade fixtures (%d bytes) outgrow the largest committed fixture (%d)" % (total, kitten)


def shadow_fixtures():
    """tests/golden/shadow/<w>x<h>.npz and range.npz: the inputs of the shadow pass at three image sizes, and of the four rays that hold tmin
    and tmax from both sides exactly (tests/shadow_cases.py, range_case: one launch, its own one-mesh scene), and what the REFERENCE'S
    shadow.comp.glsl, translated and run on the CPU against the ray query of oracle/glsl_rayquery_shim.h, makes of them.  Data only.
      inputs   sd (one 96-byte NvShadowData record per launch of shadow_cases.FIXTURE_LAUNCHES), depth, meshes, indices, vertices, the draws
               with the opaque scene's postPass (draws_opaque) and with the textured scene's (draws_textured), materials, the decoded set
               (descs, texels) and the DDS file images it was decoded from (dds, dds_sizes)
      outputs  per launch k: mask_q0_k, mask_q1_k (untextured, draws_opaque), mask_tex_k (quality 1 with the alpha test, draws_textured), each
               over a mask prefilled with shadow_cases.PREFILL, and rays_k (origin, direction, tmin, tmax of every storing invocation)"""
    import shadow_cases as SC
    os.makedirs(SC.GOLDEN, exist_ok=True)

    def record(launches, opaque, textured, tset, files):
        depth = launches[0][1]
        assert opaque["meshes"].tobytes() == textured["meshes"].tobytes() and opaque["indices"].tobytes() == textured["indices"].tobytes()
        f = dict(sd=np.stack([np.frombuffer(sd.tobytes(), np.uint8) for sd, _ in launches]), depth=depth, meshes=textured["meshes"], indices=textured["indices"],
                 vertices=textured["vertices"], draws_opaque=opaque["draws"], draws_textured=textured["draws"], materials=textured["materials"],
                 descs=tset["descs"], texels=tset["texels"], dds=np.frombuffer(b"".join(files), np.uint8), dds_sizes=np.array([len(t) for t in files], np.uint32))
        for k, (sd, d) in enumerate(launches):
            assert d.tobytes() == depth.tobytes()
            for q in (0, 1):
                r = R.shadow(sd, d, textured["meshes"], textured["indices"], textured["vertices"], opaque["draws"], None, None, q, SC.PREFILL)
                f["mask_q%d_%d" % (q, k)] = r["mask"]
            f["rays_%d" % k] = r["rays"]
            r = R.shadow(sd, d, textured["meshes"], textured["indices"], textured["vertices"], textured["draws"], textured["materials"], tset, 1, SC.PREFILL)
            f["mask_tex_%d" % k] = r["mask"]
        return f

    opaque, (textured, tset) = SC.opaque_scene(), SC.textured_scene()
    records = [("%dx%d" % (w, h), record([SC.inputs(w, h, jitter, cb) for cb, jitter in SC.FIXTURE_LAUNCHES], opaque, textured, tset, textured["textures"]))
               for w, h in SC.SIZES]
    # the four rays that hold tmin and tmax from both sides (shadow_cases.range_case): one launch
    sd, depth, opaque, textured, tset, files = SC.range_case()
    records.append(("range", record([(sd, depth)], opaque, textured, tset, files)))
    assert (records[-1][1]["mask_q0_0"] == SC.RANGE_MASK).all() and (records[-1][1]["mask_tex_0"] == SC.RANGE_MASK).all()
    total = 0
    for name, f in records:
        path = os.path.join(SC.GOLDEN, name + ".npz")
        np.savez_compressed(path, **f)
        total += os.path.getsize(path)
        print("%-28s %6d bytes, %d arrays" % ("shadow/%s.npz" % name, os.path.getsize(path), len(f)))
    kitten = os.path.getsize(os.path.join(HERE, "mesh", "kitten.npz"))
    print("tests/golden/shadow: %d bytes" % total)
    assert total <= kitten, "the shadow fixtures (%d bytes) outgrow the largest committed fixture (%d)" % (total, kitten)


def kitten_fixture(obj):
    """tests/golden/mesh/kitten.npz: the reference's data/kitten.obj as arrays (the text file is too large to commit): positions and normals as
    float32 exactly as float() + np.float32 parse them, and every face corner as 0-based (position, normal) indices, three corners per triangle

        python tests/golden/generate.py --kitten <reference>/data/kitten.obj"""
    pos, nrm, corners = [], [], []
    for line in open(obj):
        if line.startswith("v "):
            pos.append([float(x) for x in line.split()[1:4]])
        elif line.startswith("vn "):
            nrm.append([float(x) for x in line.split()[1:4]])
        elif line.startswith("f "):
            toks = line.split()[1:]
            assert len(toks) == 3, line
            for tok in toks:
                a, _, n = tok.split("/")
                corners.append((int(a) - 1, int(n) - 1))
    path = os.path.join(HERE, "mesh", "kitten.npz")
    np.savez_compressed(path, positions=np.array(pos, np.float32), normals=np.array(nrm, np.float32), corners=np.array(corners, np.uint16))
    print("%-28s %6d bytes, %d vertices, %d triangles" % ("mesh/kitten.npz", os.path.getsize(path), len(pos), len(corners) // 3))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--kitten":
        kitten_fixture(sys.argv[2])
        raise SystemExit(0)
    if len(sys.argv) == 2 and sys.argv[1] == "--shade":
        shade_fixtures()
        raise SystemExit(0)
    if len(sys.argv) == 2 and sys.argv[1] == "--shadow":
        shadow_fixtures()
        raise SystemExit(0)
    main()
    mesh_fixture()
    task_fixture()
    shade_fixtures()
    shadow_fixtures()
