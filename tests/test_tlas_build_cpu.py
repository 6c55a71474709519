"""The rebuilt TLAS without a GPU: nv_rt_tlas_build_host, the host twin of the device rebuild.  Its invariants, an independent
numpy restatement of the key, the order and the tree (tests/tlas_ref.py), the edge cases, the refusals, and CONSERVATIVENESS — the traversal on
the rebuilt blob against the brute-force restatement tests/shadow_ref.c on the MOVED draws, zero differences allowed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import shadow_ref as SH
import tlas_ref as TR
import niagara_amd as N
from niagara_amd import host
from niagara_amd import layouts as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shref(tmp_path_factory):
    return SH.load(tmp_path_factory.mktemp("shadow_ref_tlas_cpu"))


@pytest.fixture(scope="module")
def base():
    """the fuzz scene with a third mesh that has no triangles, and its static blob"""
    sc = TR.with_empty_mesh(SH.fuzz_scene())
    return sc, host.rt_scene_build(sc["meshes"], sc["indices"], sc["vertices"], sc["draws"])


def _static_boxes(scene, draws):
    """draw id -> (lo, hi): the leaf boxes nv_rt_scene_build gives the same draws (the host instance_box)"""
    h, nodes, inst, _ = TR.sections(host.rt_scene_build(scene["meshes"], scene["indices"], scene["vertices"], draws))
    leaves = np.flatnonzero(nodes["leaf"] != 0)
    first = nodes["leaf"][leaves] & np.uint32((1 << 29) - 1)
    return {int(inst["drawId"][f]): (nodes["lo"][k].tobytes(), nodes["hi"][k].tobytes()) for k, f in zip(leaves, first)}, h


def _check_invariants(scene, blob, draws):
    out = host.rt_tlas_build_host(blob, draws)
    assert out.tobytes() == host.rt_tlas_build_host(blob, draws).tobytes()       # two builds
    assert out.tobytes() == host.rt_tlas_build_host(out, draws).tobytes()        # a rebuild from a rebuilt blob
    assert host.rt_scene_validate(out)
    st = host.rt_scene_stats(out)
    h, nodes, inst, static = TR.sections(out)
    n = st["instances"]
    assert st["tlasNodes"] == (2 * n - 1 if n else 0) and st["tlasLeaves"] == n and st["tlasMaxLeaf"] == (1 if n else 0)
    assert static == TR.sections(blob)[3] and int(h["drawCount"]) == len(draws) and int(h["bytes"]) == out.nbytes
    want, sh = _static_boxes(scene, draws)
    assert sorted(want) == sorted(inst["drawId"].tolist())  # the casting set is nv_rt_scene_build's
    assert h["padOrigin"].tobytes() == sh["padOrigin"].tobytes()
    leaves = np.flatnonzero(nodes["leaf"] != 0)
    for k, i in zip(leaves, inst):
        assert (nodes["lo"][k].tobytes(), nodes["hi"][k].tobytes()) == want[int(i["drawId"])]
        d = draws[int(i["drawId"])]
        assert i["position"].tobytes() == d["position"].tobytes() and i["orientation"].tobytes() == d["orientation"].tobytes()
        assert i["scale"].tobytes() == d["scale"].tobytes() and int(i["postPass"]) == int(d["postPass"]) and int(i["blas"]) == int(d["meshIndex"])
        assert not i["reserved"].any()
    r = TR.check_blob(out)  # the restatement: instance order, every skip and leaf word; inner boxes = min / max of the children's
    return out, r


def test_library_exports_the_entry_points_and_refuses_bad_arguments(base):
    for name in ("nv_rt_tlas_build_host", "nv_rt_scene_reserve_dynamic", "nv_rt_tlas_build", "nv_rt_scene_download"):
        assert name in N.EXPORTS and hasattr(N.lib, name), name
    sc, blob = base
    d = np.ascontiguousarray(sc["draws"])
    n = C.c_uint64(0)
    call = N.lib.nv_rt_tlas_build_host
    assert call(blob.ctypes.data, blob.nbytes, d.ctypes.data, len(d), None, C.byref(n)) == 0 and n.value >= blob.nbytes - 64
    out = host._aligned_bytes(n.value)
    assert call(blob.ctypes.data, blob.nbytes, d.ctypes.data, len(d), None, None) == -1                     # NULL bytes
    assert call(blob.ctypes.data, blob.nbytes, None, len(d), None, C.byref(n)) == -1                         # NULL draws, count != 0
    assert call(blob.ctypes.data, blob.nbytes, d.ctypes.data, 1 << 29, None, C.byref(n)) == -1               # drawCount > RT_LEAF_FIRST
    assert call(blob.ctypes.data, blob.nbytes, d.ctypes.data, len(d), out.ctypes.data + 4, C.byref(n)) == -1  # a misaligned out
    small = C.c_uint64(n.value - 16)
    assert call(blob.ctypes.data, blob.nbytes, d.ctypes.data, len(d), out.ctypes.data, C.byref(small)) == -1  # too little room
    assert call(blob.ctypes.data, blob.nbytes - 16, d.ctypes.data, len(d), None, C.byref(n)) == -1            # a blob the validator refuses
    bad = host._aligned_bytes(blob.nbytes)
    bad[:] = blob
    bad[int(TR.sections(blob)[0]["tlasOff"]) + 12:][:4].view(np.uint32)[0] = 0  # the root's skip = 0: a loop
    assert not host.rt_scene_validate(bad) and call(bad.ctypes.data, bad.nbytes, d.ctypes.data, len(d), None, C.byref(n)) == -1
    assert call(None, 0, None, 0, None, C.byref(n)) == -1
    # the context entry points refuse a NULL context before they touch a device
    assert N.lib.nv_rt_scene_reserve_dynamic(None, None, 4) == -1 and N.lib.nv_rt_tlas_build(None, None, None, 0) == -1
    assert N.lib.nv_rt_scene_download(None, None, None, C.byref(n)) == -1


def test_static_build_is_unchanged_and_shares_the_leaf_boxes(base):
    """a rebuild from the unmoved draws: the static builder's casting set, leaf boxes and padOrigin (the bytes of nv_rt_scene_build's own
    blobs are compared with the parent commit's outside the suite)"""
    sc, blob = base
    _check_invariants(sc, blob, sc["draws"])


@pytest.mark.parametrize("n", [0, 1, 2, 3, 20, 300, 4133])
def test_invariants_and_the_restatement_over_mixed_draws(n, base):
    sc, blob = base
    draws = TR.mixed_draws(n, 100 + n, 2, 40.0, empty_mesh=2)
    out, r = _check_invariants(sc, blob, draws)
    casting = [i for i, d in enumerate(draws) if d["postPass"] <= 1 and d["scale"] > 0 and np.isfinite(d["position"]).all() and d["meshIndex"] < 2]
    assert r["order"].tolist() != sorted(r["order"].tolist()) or n < 20  # the order is the keys', not the draws'
    assert sorted(r["order"].tolist()) == casting
    if n >= 300:
        assert len(casting) < n and len(np.unique(r["keys"])) < len(r["keys"])  # non-casters and duplicate keys took part


def test_edge_counts(base):
    sc, blob = base
    for n in range(4):
        draws = TR.moved(sc["draws"][sc["draws"]["postPass"] <= 1][:n], 5, 30.0)
        out, r = _check_invariants(sc, blob, draws)
        h, nodes, inst, _ = TR.sections(out)
        assert int(h["instances"]) == n and len(nodes) == (0, 1, 3, 5)[n]
        if n == 1:
            assert int(nodes["skip"][0]) == 1 and int(nodes["leaf"][0]) == 1 << 29


def test_identical_transforms_split_on_the_tie_bits(base):
    """all keys equal: the strings differ in k alone, the tree is the balanced tree of the indices and its depth is ceil(log2 n)"""
    sc, blob = base
    for n in (2, 64, 300):
        draws = np.repeat(TR.moved(sc["draws"][:1], 9, 10.0), n)
        draws["postPass"] = 0
        out, r = _check_invariants(sc, blob, draws)
        assert len(np.unique(r["keys"])) == 1 and r["order"].tolist() == list(range(n))
        assert r["depth"] == int(np.ceil(np.log2(n)))


def test_two_far_clusters_and_the_infinite_box(base):
    sc, blob = base
    draws = TR.moved(np.repeat(sc["draws"][:1], 40), 3, 5.0)
    draws["postPass"] = 0
    draws["position"][20:, 0] += np.float32(1.0e6)  # along x, whose cell holds the key's highest bit
    out, r = _check_invariants(sc, blob, draws)
    h, nodes, inst, _ = TR.sections(out)
    left = set(inst["drawId"][:int(nodes["skip"][1]) // 2].tolist())  # the left child's subtree is [1, skip): 2 m - 1 nodes over the first m leaves
    assert left == set(range(20))  # the root separates the clusters
    # The singular map: rotateQuat(., q) is I + 2 (C C + w C), singular iff w = 0 and |xyz|^2 = 1/2 (a ZERO quaternion is the identity map
    # and keeps a finite box; draw 9 has one).  The fp32 nearest to sqrt(1/2) leaves it so ill-conditioned that it gets the "everything" box
    draws["orientation"][7] = (np.sqrt(0.5), 0.0, 0.0, 0.0)
    draws["orientation"][9] = 0.0
    out, r = _check_invariants(sc, blob, draws)
    h, nodes, inst, _ = TR.sections(out)
    k = int(np.flatnonzero(inst["drawId"] == 7)[0])
    leaf = int(np.flatnonzero(nodes["leaf"] == (1 << 29 | k))[0])
    assert np.isneginf(nodes["lo"][leaf]).all() and np.isposinf(nodes["hi"][leaf]).all()
    assert np.isneginf(nodes["lo"][0]).all() and np.isposinf(nodes["hi"][0]).all()  # and so is every box above it


@pytest.mark.parametrize("kind", ["NaN position", "scale 0", "postPass 2", "meshIndex past the meshes", "a mesh without triangles"])
def test_draws_that_do_not_cast(kind, base):
    sc, blob = base
    draws = TR.moved(sc["draws"], 21, 30.0)
    draws["postPass"] = 0
    before = host.rt_scene_stats(host.rt_tlas_build_host(blob, draws))["instances"]
    assert before == len(draws)
    if kind == "NaN position":
        draws["position"][4, 2] = np.nan
    elif kind == "scale 0":
        draws["scale"][4] = 0.0
    elif kind == "postPass 2":
        draws["postPass"][4] = 2
    elif kind == "meshIndex past the meshes":
        draws["meshIndex"][4] = 3
    else:
        draws["meshIndex"][4] = 2
    out, r = _check_invariants(sc, blob, draws)
    assert 4 not in r["order"].tolist() and len(r["order"]) == before - 1
    assert host.rt_scene_stats(host.rt_tlas_build_host(blob, draws[4:5]))["tlasNodes"] == 0  # alone: no caster at all


# ---------------------------------------------------------------------------------------------------------------- conservativeness

def _same(name, scene, blob, shref, o, d):
    hits = []
    for q in (0, 1):
        want = shref.trace(scene, o, d, q)
        got = host.rt_scene_trace_host(blob, o, d, q)
        diff = int((want != got).sum())
        print("%s quality %d: %d rays, %d occluded, %d differences" % (name, q, len(want), int((want == 0).sum()), diff))
        assert diff == 0
        hits.append(int((want == 0).sum()))
    return hits


def test_fuzz_on_the_moved_draws_equals_the_brute_force(base, shref):
    """fuzz_scene with all transforms redrawn: rotated and scaled instances, postPass 0 / 1 / 2, the ray fuzz of test_shadowtrace_cpu.py"""
    sc, blob = base
    movedscene = dict(sc, draws=TR.moved(sc["draws"], 77, 300.0))
    assert sorted(set(movedscene["draws"]["postPass"].tolist())) == [0, 1, 2]
    rebuilt = host.rt_tlas_build_host(blob, movedscene["draws"])
    TR.check_blob(rebuilt)
    o, d = SH.fuzz_rays(movedscene, 201000)
    hits = _same("moved fuzz", movedscene, rebuilt, shref, o, d)
    assert 20000 < hits[0] < hits[1] < 180000
    # the input condition: the move matters — the static blob answers differently for these rays
    stale = host.rt_scene_trace_host(blob, o, d, 1)
    assert int((stale != shref.trace(movedscene, o, d, 1)).sum()) > 10000


def test_degenerate_rays_on_the_rebuilt_aligned_scene_equal_the_brute_force(shref):
    """axis-aligned rays through box planes, edges and vertices, and non-finite rays, on a TLAS rebuilt for aligned_scene moved by exact
    amounts (integer positions, power-of-two scales: the lattice of degenerate_rays stays exact)"""
    sc = SH.aligned_scene()
    blob = host.rt_scene_build(sc["meshes"], sc["indices"], sc["vertices"], sc["draws"])
    draws = sc["draws"].copy()
    draws["position"] = [(2.0, 0.0, -1.0), (-8.0, 4.0, 4.0), (6.0, -2.0, 3.0)]
    draws["scale"] = (2.0, 1.0, 0.5)
    movedscene = dict(sc, draws=draws)
    rebuilt = host.rt_tlas_build_host(blob, draws)
    TR.check_blob(rebuilt)
    o, d = SH.degenerate_rays(movedscene)
    assert ((d == 0).sum(1) == 2).sum() > 5000 and not np.isfinite(o).all() and not np.isfinite(d).all()
    hits = _same("moved degenerate", movedscene, rebuilt, shref, o, d)
    assert hits[0] > 1000 and hits[1] > hits[0]


@pytest.mark.parametrize("which", ["aligned", "extreme"])
def test_degenerate_launches_on_the_rebuilt_scene_equal_the_brute_force(which, shref):
    """every launch of shadow_ref.degenerate_launches around the exactly-moved draws, on the TLAS the host twin rebuilds for them
    (tests/test_shadow_degenerate_gpu.py hands the same launches to the device's rebuild); the input conditions on the restatement alone"""
    sc = SH.aligned_scene() if which == "aligned" else SH.extreme_scene()
    blob = host.rt_scene_build(sc["meshes"], sc["indices"], sc["vertices"], sc["draws"])
    movedscene = dict(sc, draws=SH.moved_exactly(sc))
    rebuilt = host.rt_tlas_build_host(blob, movedscene["draws"])
    assert host.rt_scene_validate(rebuilt)
    TR.check_blob(rebuilt)
    launches = SH.degenerate_launches(movedscene)
    o, d, fam = SH.launch_rays(shref, launches)
    masks = {}
    for q in (0, 1):
        masks[q] = SH.in_chunks(lambda a, b: shref.trace(movedscene, a, b, q), o, d)
        got = host.rt_scene_trace_host(rebuilt, o, d, q)
        diff = int((masks[q] != got).sum())
        print("moved %s quality %d: %d launches, %d rays, %d occluded, %d differences" % (which, q, len(launches), len(o), int((masks[q] == 0).sum()), diff))
        assert diff == 0
    SH.input_conditions("moved " + which, o, d, fam, masks)
    stale = host.rt_scene_trace_host(blob, o, d, 1)
    print("moved %s: the static blob answers %d of these rays differently" % (which, int((stale != masks[1]).sum())))
    assert (stale != masks[1]).sum() >= 50  # the move matters (the bound of tests/test_tlas_build_gpu.py's moved draws)
    if which == "extreme":
        assert len(SH.infinite_leaves(TR.sections(blob)[1])) >= 1 and len(SH.infinite_leaves(TR.sections(rebuilt)[1])) >= 1


def test_mixed_draws_equal_the_brute_force(base, shref):
    """clusters, duplicates, the infinite box and non-casters of every kind under the ray fuzz"""
    sc, blob = base
    draws = TR.mixed_draws(60, 31, 2, 30.0, empty_mesh=2)
    draws["position"][:, 0] = np.where(draws["position"][:, 0] > 1e4, draws["position"][:, 0] - np.float32(5.0e4 - 200.0), draws["position"][:, 0])
    movedscene = dict(sc, draws=draws)
    rebuilt = host.rt_tlas_build_host(blob, draws)
    ok = np.isfinite(draws["position"]).all(1) & (draws["meshIndex"] < 2)
    o, d = SH.fuzz_rays(dict(movedscene, draws=draws[ok]), 30000, seed=4)  # aimed at the draws that have a surface
    hits = _same("mixed", movedscene, rebuilt, shref, o, d)
    assert hits[1] > 1000


def test_the_standalone_program_runs_clean_under_the_host_sanitizers(tmp_path):
    """tools/rt_tlas_check.cpp with rtbuild.cpp, host code only, its own main: AddressSanitizer and UBSan linked statically into the program itself"""
    exe = tmp_path / "rt_tlas_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "rt_tlas_check.cpp"),
                           os.path.join(ROOT, "niagara_amd", "csrc", "rtbuild.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    print(out.stdout.decode())
    assert out.returncode == 0 and b"rt_tlas_check: ok" in out.stdout
