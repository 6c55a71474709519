"""BASELINE config 1 — kitten.obj, 1024 draws x 1 meshlet, frustum-only cull (plumbing; the CPU half runs without a GPU).

The mesh bounds follow src/scene.cpp:207-220 (mean of the de-quantised fp16 positions of the unique vertices, max
distance).  meshoptimizer's vertex reordering is not vendored, so the unique vertices are taken in first-appearance
order; the float32 mean is order-sensitive only in its last bits.  kitten.obj is too large to commit: its positions,
normals and face corners are stored as tests/golden/mesh/kitten.npz (tests/golden/generate.py --kitten), from which the bounds
are recomputed and compared with the committed tests/golden/kitten_bounds.json.
"""
import json
import os

import numpy as np
import pytest

import oracle
from niagara_amd import host
from niagara_amd import layouts as L

HERE = os.path.dirname(os.path.abspath(__file__))
NPZ = os.path.join(HERE, "golden", "mesh", "kitten.npz")
JSON = os.path.join(HERE, "golden", "kitten_bounds.json")


def load_kitten():
    """kitten.obj as arrays: positions, normals (float32) and the (position, normal) index of every face corner, three per triangle"""
    k = np.load(NPZ)
    return k["positions"], k["normals"], k["corners"].astype(np.int64)


def bounds_from_kitten():
    pos, nrm, c = load_kitten()
    half = pos[c[:, 0]].astype(np.float16)                       # src/scene.cpp:149-151
    q = np.rint(nrm[c[:, 1]] * 511).astype(np.int32) + 511       # src/scene.cpp:153-155
    key = np.concatenate([half.view(np.uint16).astype(np.int64), q.astype(np.int64)], axis=1)
    _, first = np.unique(key, axis=0, return_index=True)
    uniq = half[np.sort(first)].astype(np.float32)               # src/scene.cpp:193-198
    center, radius = host.mesh_bounds(uniq)                      # src/scene.cpp:207-220 through the C ABI (nv_mesh_bounds)
    return dict(vertices=int(len(pos)), triangles=int(len(c) // 3), unique_vertices=int(len(uniq)),
                center=[float(x) for x in center], radius=float(radius))


def kitten_bounds():
    b = bounds_from_kitten()
    ref = json.load(open(JSON))
    assert b["vertices"] == ref["vertices"] == 14472 and b["triangles"] == ref["triangles"] == 28944
    assert np.allclose(b["center"], ref["center"], atol=1e-6) and abs(b["radius"] - ref["radius"]) < 1e-6
    return ref


def test_mesh_bounds_equal_the_reference_statements():
    """nv_mesh_bounds == src/scene.cpp:207-220 compiled verbatim (oracle/_ref), bit for bit: random clouds of every size
    class (the fp32 sum is order- and size-sensitive), values that cancel, and the kitten"""
    import oracle.ref as R
    if not R.available():
        pytest.skip("oracle/_ref not built")
    rng = np.random.default_rng(12)
    clouds = [rng.normal(0, s, (n, 3)).astype(np.float32) + np.float32(o) for n, s, o in
              [(1, 1, 0), (2, 1, 5), (3, 1e-3, 0), (17, 10, -3), (1000, 1, 100), (14856, 0.3, 0), (200000, 50, 1e4), (65536, 1e-6, 1)]]
    clouds.append(np.array([[1e8, -1e8, 1], [-1e8, 1e8, 1], [1, 1, 1]], np.float32))
    clouds.append(rng.normal(0, 1, (5000, 3)).astype(np.float16).astype(np.float32))  # de-quantised halves, like the real input
    clouds.append(load_kitten()[0].astype(np.float16).astype(np.float32))
    for pos in clouds:
        c, r = host.mesh_bounds(pos)
        cr, rr = R.mesh_bounds(pos)
        assert c.tobytes() == cr.tobytes() and np.float32(r).tobytes() == np.float32(rr).tobytes(), len(pos)
    with pytest.raises(RuntimeError, match="NV_EINVAL"):
        host.mesh_bounds(np.zeros((0, 3), np.float32))


def kitten_scene(n_draws=1024):
    b = kitten_bounds()
    meshes = np.zeros(1, dtype=L.MESH)
    meshes["center"] = np.array(b["center"], np.float32)
    meshes["radius"] = np.float32(b["radius"])
    meshes["lodCount"] = 1
    meshes["lods"][0][0]["meshletCount"] = 1
    meshes["lods"][0][0]["indexCount"] = b["triangles"] * 3
    meshlets = np.zeros(64, dtype=L.MESHLET)  # one real meshlet + padding of the pool
    meshlets["center"][0] = np.array(b["center"], np.float32).astype(np.float16).view(np.uint16)
    meshlets["radius"][0] = np.array([b["radius"]], np.float32).astype(np.float16).view(np.uint16)[0]
    meshlets["cone_cutoff"] = 127
    draws = host.synth_draws(n_draws, 1, 300.0)       # src/niagara.cpp:969-998
    slots, _ = host.assign_visibility_offsets(draws, meshes)
    cd = host.build_cull_data(draw_count=n_draws, cullingEnabled=1)   # camera at the origin, 1024x768, fovY 70 deg
    return meshes, meshlets, draws, cd, slots


def run_cpu(impl, meshes, meshlets, draws, cd):
    n = len(draws)
    dc, c4 = np.zeros(n + 1, dtype=L.DRAWCMD), np.zeros(4, np.uint32)
    impl.drawcull(cd, 0, 0, draws, meshes, dc, c4, np.ones(n, np.uint32), None)
    tc, t4 = np.zeros(n + 64, dtype=L.TASKCMD), np.zeros(4, np.uint32)
    impl.drawcull(cd, 0, 1, draws, meshes, tc, t4, np.ones(n, np.uint32), None)
    impl.tasksubmit(t4, tc)
    cib, cc4 = np.zeros(int(t4[1]) * 64 * 64 + 256, np.uint32), np.zeros(4, np.uint32)
    impl.clustercull(cd, 0, tc, t4, draws, meshlets, None, None, cib, cc4)
    return dc, c4, tc, t4, cib, cc4


def test_kitten_cpu_reference_path():
    meshes, meshlets, draws, cd, slots = kitten_scene()
    assert slots == 1024
    dc, c4, tc, t4, cib, cc4 = run_cpu(oracle, meshes, meshlets, draws, cd)
    # frustum volume / cube volume: a few percent of 1024 draws survive, each with one task command of one meshlet
    assert 10 < c4[0] < 120 and t4[0] == c4[0]
    assert (tc["taskCount"][:t4[0]] == 1).all() and (tc["drawId"][:t4[0]] == dc["drawId"][:c4[0]]).all()
    # the meshlet sphere is the fp16-rounded mesh sphere: nearly every visible draw keeps its meshlet
    assert cc4[0] <= t4[0] and cc4[0] >= t4[0] - 4
    import oracle.ref as R
    if R.available():
        for a, b in zip(run_cpu(oracle, meshes, meshlets, draws, cd), run_cpu(R, meshes, meshlets, draws, cd)):
            assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
def test_kitten_gpu_matches_cpu():
    import torch

    from niagara_amd import pipeline as P
    meshes, meshlets, draws, cd, _ = kitten_scene()
    dc, c4, tc, t4, cib, cc4 = run_cpu(oracle, meshes, meshlets, draws, cd)
    ctx = P.Context()
    dev = ctx.device
    db, mb, mlb = P.to_device(draws, dev), P.to_device(meshes, dev), P.to_device(meshlets, dev)
    n = len(draws)
    dvb = torch.ones(n, dtype=torch.int32, device=dev)
    dcb = torch.zeros((n + 64) * 24, dtype=torch.uint8, device=dev)
    dccb = torch.zeros(4, dtype=torch.int32, device=dev)
    ctx.drawcull(cd, 0, 0, db, mb, dcb, dccb, dvb, None)
    assert int(dccb[0].item()) == c4[0] and P.from_device(dcb, L.DRAWCMD)[:c4[0]].tobytes() == dc[:c4[0]].tobytes()
    dccb.zero_()
    ctx.drawcull(cd, 0, 1, db, mb, dcb, dccb, dvb, None)
    ctx.tasksubmit(dccb, dcb)
    assert (dccb.cpu().numpy().view(np.uint32) == t4).all()
    g_cib = torch.zeros(len(cib), dtype=torch.int32, device=dev)
    g_ccb = torch.zeros(4, dtype=torch.int32, device=dev)
    ctx.clustercull(cd, 0, dcb, dccb, db, mlb, None, None, g_cib, g_ccb)
    assert int(g_ccb[0].item()) == cc4[0]
    assert (g_cib.cpu().numpy().view(np.uint32)[:cc4[0]] == cib[:cc4[0]]).all()
    ctx.status()
    ctx.close()
