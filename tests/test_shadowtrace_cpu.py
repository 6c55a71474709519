"""The ray-traced shadow pass without a GPU: the ABI, the invariants of the scene blob nv_rt_scene_build writes, the
validator, and CONSERVATIVENESS — nv_rt_scene_trace_host (the kernel's traversal, the same text) against the brute-force restatement
tests/shadow_ref.c on every ray, zero differences allowed: the BVH is an acceleration that must never change a bit."""
import os
import subprocess

import numpy as np
import pytest

import oracle
import shade_ref as SR
import shadow_ref as SH
import visattr_ref as VA
import visbuffer_ref as VB
import niagara_amd as N
from niagara_amd import host, synth
from niagara_amd import layouts as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The sun of the frame tests.  niagara's normalize(1, 1, 1) shadows 84 covered pixels of the occluder scene (only the right-hand boxes' inner
# faces); normalize(2, 0.3, 1) puts the left boxes in the wall's shadow: 246 covered pixels store 0 there and 19621 in the interior scene
# (the restatement's counts, asserted below).
SUN = np.array([2.0, 0.3, 1.0]) / np.linalg.norm([2.0, 0.3, 1.0])


@pytest.fixture(scope="session")
def shref(tmp_path_factory):
    return SH.load(tmp_path_factory.mktemp("shadow_ref_cpu"))


@pytest.fixture(scope="session")
def frames(tmp_path_factory):
    """the two frame scenes with the depth their CPU reference frames leave: name -> scene dict with depth, cull, viewport"""
    vref = VB.load(tmp_path_factory.mktemp("visbuffer_ref_shadow_cpu"))
    aref = VA.load(tmp_path_factory.mktemp("visattr_ref_shadow_cpu"))
    f = SR.reference_frame(vref, aref)
    s = f["scene"]
    indices, meshes = synth.indexed_geometry(s["meshes"], s["meshlets"], s["data"])
    ref = synth.occluder_scene_indexed(meshlet_bounds=oracle.meshlet_bounds)
    # synth.occluder_scene_indexed, with the material indices VA.with_attributes spreads over the draws
    assert indices.tobytes() == ref["indices"].tobytes() and meshes.tobytes() == ref["meshes"].tobytes()
    assert all(s["draws"][k].tobytes() == ref["draws"][k].tobytes() for k in ("position", "scale", "orientation", "meshIndex", "postPass"))
    out = dict(occluder=dict(meshes=meshes, indices=indices, vertices=s["vertices"], draws=s["draws"], depth=f["depth"], cull=s["cull"], viewport=s["viewport"]))
    si = synth.interior_scene_indexed(meshlet_bounds=oracle.meshlet_bounds)
    w, h = si["viewport"]
    rec = VB.oracle_frames(si, 2, True, vref, 1)[-1]
    out["interior"] = dict(meshes=si["meshes"], indices=si["indices"], vertices=si["vertices"], draws=si["draws"], cull=si["cull"], viewport=si["viewport"],
                           depth=np.ascontiguousarray(rec["post"]["depth"], np.float32).reshape(h, w))
    return out


def _build(scene):
    return host.rt_scene_build(scene["meshes"], scene["indices"], scene["vertices"], scene["draws"])


# ---------------------------------------------------------------------------------------------------------------- ABI

def test_shadow_data_layout_matches_the_header(tmp_path):
    fields = [n for n in L.SHADOWDATA.names]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "niagara_vis.h"\nint main(void){printf("%zu", sizeof(NvShadowData));\n' +
                   "".join('printf(" %%zu", offsetof(NvShadowData, %s));\n' % f for f in fields) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == L.SHADOWDATA.itemsize == 96
    assert got[1:] == [L.SHADOWDATA.fields[f][1] for f in fields]
    assert [L.SHADOWDATA.fields[f][1] for f in ("sunDirection", "sunJitter", "inverseViewProjection", "imageSize", "checkerboard")] == [0, 12, 16, 80, 88]


def test_library_exports_the_entry_points_and_refuses_bad_arguments():
    for name in ("nv_rt_scene_build", "nv_rt_scene_validate", "nv_rt_scene_stats", "nv_rt_scene_trace_host", "nv_rt_scene_upload", "nv_shadow_trace",
                 "nv_build_shadow_data"):
        assert name in N.EXPORTS and hasattr(N.lib, name), name
    assert N.lib.nv_shadow_trace(None, None, None, None, None, 4, 4, 0) == -1
    assert N.lib.nv_rt_scene_upload(None, None, None, 0) == -1
    assert N.lib.nv_rt_scene_build(None, 0, None, 0, None, 0, None, 0, None, None) == -1
    assert N.lib.nv_rt_scene_validate(None, 64) == -1
    with pytest.raises(N.NvError):  # a singular product
        host.build_shadow_data(np.zeros(1, L.GLOBALS), width=4, height=4)


def test_shadow_data_shares_the_shade_data_inverse():
    cd = host.build_cull_data(cam_pos=(0.5, 1.0, 2.0), viewport=(67, 37), pyramid=(64, 32))
    g = synth.make_globals(cd, (67, 37))
    sd = host.build_shade_data(g, (0.5, 1.0, 2.0), SUN, 1, 67, 37)
    sh = host.build_shadow_data(g, SUN, 1e-2, 1, 67, 37)
    assert sh["inverseViewProjection"].tobytes() == sd["inverseViewProjection"].tobytes()
    assert sh["sunDirection"].tobytes() == sd["sunDirection"].tobytes() and sh["imageSize"].tolist() == [[67.0, 37.0]]
    assert float(sh["sunJitter"][0]) == np.float32(1e-2) and int(sh["checkerboard"][0]) == 1


# ---------------------------------------------------------------------------------------------------------------- the blob

HEADER = np.dtype([(n, "<u4") for n in ("magic", "version", "bytes", "meshCount", "tlasNodes", "instances", "blasNodes", "triangles", "tableOff", "tlasOff",
                                         "instOff", "blasOff", "triOff")] + [("padOrigin", "<f4"), ("drawCount", "<u4"), ("reserved", "<u4")])
BLAS = np.dtype([("nodeFirst", "<u4"), ("nodeCount", "<u4"), ("triFirst", "<u4"), ("triCount", "<u4"), ("maxAbs", "<f4"), ("maxExtent", "<f4"), ("reserved", "<u4", 2)])
NODE = np.dtype([("lo", "<f4", 3), ("skip", "<u4"), ("hi", "<f4", 3), ("leaf", "<u4")])
INSTANCE = np.dtype([("position", "<f4", 3), ("scale", "<f4"), ("orientation", "<f4", 4), ("drawId", "<u4"), ("postPass", "<u4"), ("blas", "<u4"), ("reserved", "<u4", 5)])


def _sections(blob):
    h = blob[:64].view(HEADER)[0]
    part = lambda off, count, dt: blob[int(off):int(off) + int(count) * dt.itemsize].view(dt)
    return h, part(h["tableOff"], h["meshCount"], BLAS), part(h["tlasOff"], h["tlasNodes"], NODE), part(h["instOff"], h["instances"], INSTANCE), \
        part(h["blasOff"], h["blasNodes"], NODE), blob[int(h["triOff"]):int(h["triOff"]) + int(h["triangles"]) * 48].view(np.float32).reshape(-1, 3, 4)


def _walk(nodes, leaf_max, prim_lo, prim_hi):
    """the invariants of one preorder tree with skip links: returns the primitives in leaf order"""
    n = len(nodes)
    seen = []
    for i in range(n):
        skip, leaf = int(nodes["skip"][i]), int(nodes["leaf"][i])
        assert i < skip <= n
        if leaf:
            count, first = leaf >> 29, leaf & ((1 << 29) - 1)
            assert 1 <= count <= leaf_max and skip == i + 1
            seen += list(range(first, first + count))
            lo, hi = prim_lo[first:first + count].min(0), prim_hi[first:first + count].max(0)
            assert (nodes["lo"][i] <= lo).all() and (nodes["hi"][i] >= hi).all()
        else:
            left, right = i + 1, int(nodes["skip"][i + 1])  # the two children of a binary node
            assert right < skip and int(nodes["skip"][right]) == skip
            for c in (left, right):
                assert (nodes["lo"][c] >= nodes["lo"][i]).all() and (nodes["hi"][c] <= nodes["hi"][i]).all()
    return seen


def _kept_triangles(scene, mi):
    m = scene["meshes"][mi]
    lod = m["lods"][m["lodRT"]]
    idx = scene["indices"][lod["indexOffset"]:lod["indexOffset"] + lod["indexCount"] // 3 * 3].astype(np.int64).reshape(-1, 3) + int(m["vertexOffset"])
    v = scene["vertices"]
    pos = np.stack([v[k].view(np.float16).astype(np.float32) for k in ("vx", "vy", "vz")], 1)
    return pos[idx]


@pytest.mark.parametrize("name", ["fuzz", "occluder", "interior"])
def test_builder_invariants(name, frames):
    scene = SH.fuzz_scene() if name == "fuzz" else frames[name]
    blob = _build(scene)
    again = _build(scene)
    assert blob.tobytes() == again.tobytes()  # deterministic; rt_scene_build asserts that the size query equals the bytes written
    assert host.rt_scene_validate(blob)
    h, table, tlas, inst, blas, tris = _sections(blob)
    st = host.rt_scene_stats(blob)
    assert st["bytes"] == blob.nbytes == int(h["bytes"]) and blob.nbytes % 16 == 0
    casting = [i for i, d in enumerate(scene["draws"]) if d["postPass"] <= 1 and d["scale"] > 0]
    assert st["instances"] == len(casting) == len(inst) and sorted(inst["drawId"].tolist()) == casting
    assert st["tlasMaxLeaf"] == 1 and st["tlasLeaves"] == len(inst) and st["tlasNodes"] == 2 * len(inst) - 1
    assert st["blasMaxLeaf"] <= 4 and st["blasCount"] == len(scene["meshes"])
    # TLAS: every instance in exactly one leaf, children inside parents
    everything_lo, everything_hi = np.full((len(inst), 3), np.inf, np.float32), np.full((len(inst), 3), -np.inf, np.float32)
    assert sorted(_walk(tlas, 1, everything_lo, everything_hi)) == list(range(len(inst)))
    total = 0
    for mi, e in enumerate(table):
        nodes = blas[int(e["nodeFirst"]):int(e["nodeFirst"]) + int(e["nodeCount"])]
        mine = tris[int(e["triFirst"]):int(e["triFirst"]) + int(e["triCount"]), :, :3]
        want = _kept_triangles(scene, mi)
        assert len(mine) == len(want)
        key = lambda t: sorted(map(bytes, t.reshape(len(t), -1)))
        assert key(np.ascontiguousarray(mine)) == key(np.ascontiguousarray(want))  # the kept triangles, each once
        order = _walk(nodes, 4, mine.min(1), mine.max(1))
        assert order == list(range(len(mine)))  # every triangle in exactly one leaf, records in leaf order
        assert float(e["maxAbs"]) == np.abs(mine).max() and float(e["maxExtent"]) == (mine.max(1) - mine.min(1)).max()
        total += len(mine)
    assert total == st["triangles"] == len(tris)
    # a TLAS leaf's box holds the instance's transformed BLAS root box
    for k in range(len(tlas)):
        if tlas["leaf"][k]:
            i = inst[int(tlas["leaf"][k]) & ((1 << 29) - 1)]
            e = table[int(i["blas"])]
            root = blas[int(e["nodeFirst"])]
            corners = np.array([[(root["hi"] if c >> a & 1 else root["lo"])[a] for a in range(3)] for c in range(8)], np.float64)
            world = i["position"].astype(np.float64) + float(i["scale"]) * SH._rotate(corners, i["orientation"].astype(np.float64))
            assert (tlas["lo"][k] < world.min(0)).all() and (tlas["hi"][k] > world.max(0)).all()
            assert ((tlas["hi"][k] - tlas["lo"][k]) < (world.max(0) - world.min(0)) + 0.25).all()  # and is not the infinite box


def test_validator_refuses_corrupt_blobs():
    blob = _build(SH.fuzz_scene())
    h, table, tlas, inst, blas, tris = _sections(blob)
    assert host.rt_scene_validate(blob)

    def patched(byte_offset, value):
        raw = np.zeros(blob.nbytes + 16, np.uint8)
        off = (-raw.ctypes.data) % 16
        b = raw[off:off + blob.nbytes]
        b[:] = blob
        b[byte_offset:byte_offset + 4].view(np.uint32)[0] = value
        return b
    assert host.rt_scene_validate(patched(0, int(h["magic"])))  # the helper itself keeps a good blob good
    assert N.lib.nv_rt_scene_validate(blob.ctypes.data, blob.nbytes - 16) == -1  # truncated
    assert N.lib.nv_rt_scene_validate(blob.ctypes.data, 48) == -1
    assert not host.rt_scene_validate(patched(0, 0x12345678))  # magic
    assert not host.rt_scene_validate(patched(4, 99))          # version
    t, b = int(h["tlasOff"]), int(h["blasOff"])
    inner = int(np.flatnonzero(tlas["leaf"] == 0)[-1])
    assert not host.rt_scene_validate(patched(t + 32 * inner + 12, inner))      # skip <= index (a loop)
    assert not host.rt_scene_validate(patched(t + 32 * inner + 12, len(tlas) + 1))  # skip past the count
    assert not host.rt_scene_validate(patched(b + 32 * 5 + 12, 5))                 # a BLAS node: skip <= index
    leaf = int(np.flatnonzero(tlas["leaf"] != 0)[0])
    assert not host.rt_scene_validate(patched(t + 32 * leaf + 28, 1 << 29 | len(inst)))  # a TLAS leaf past the instances
    e = table[1]
    bleaf = int(e["nodeFirst"]) + int(np.flatnonzero(blas["leaf"][int(e["nodeFirst"]):int(e["nodeFirst"]) + int(e["nodeCount"])] != 0)[0])
    assert not host.rt_scene_validate(patched(b + 32 * bleaf + 28, 4 << 29 | (int(e["triCount"]) - 3)))  # a leaf range past its array
    assert not host.rt_scene_validate(patched(b + 32 * bleaf + 28, 5 << 29 | 0))                         # more than 4 triangles
    assert not host.rt_scene_validate(patched(int(h["instOff"]) + 40, len(table)))                       # an instance's BLAS reference
    assert not host.rt_scene_validate(patched(int(h["tableOff"]) + 4, int(h["blasNodes"]) + 1))           # a BLAS's node range
    assert not host.rt_scene_validate(patched(int(h["tableOff"]) + 12, int(h["triangles"]) + 1))          # a BLAS's triangle range
    assert not host.rt_scene_validate(patched(36, int(h["tlasOff"]) + 8))                                 # a misaligned section
    assert not host.rt_scene_validate(patched(16, int(h["tlasNodes"]) + 100000))                          # a section past the end


# ---------------------------------------------------------------------------------------------------------------- conservativeness

def _same(name, scene, blob, shref, o, d):
    hits, masks = [], []
    for q in (0, 1):
        want = shref.trace(scene, o, d, q)
        got = host.rt_scene_trace_host(blob, o, d, q)
        diff = int((want != got).sum())
        print("%s quality %d: %d rays, %d occluded, %d differences" % (name, q, len(want), int((want == 0).sum()), diff))
        assert diff == 0
        assert set(np.unique(want).tolist()) <= {0, 255}
        hits.append(int((want == 0).sum()))
        masks.append(want)
    return hits, masks


@pytest.mark.parametrize("name", ["occluder", "interior"])
def test_the_trace_passes_rays_equal_the_brute_force(name, frames, shref):
    sc = frames[name]
    w, h = sc["viewport"]
    blob = _build(sc)
    covered = (sc["depth"] > 0).reshape(-1)
    for jitter in (0.0, 1e-2):
        sd = host.build_shadow_data(synth.make_globals(sc["cull"], (w, h)), SUN, jitter, 0, w, h)
        o, d = shref.rays(sd, sc["depth"])
        want = _same("%s jitter %g" % (name, jitter), sc, blob, shref, o, d)[1][1]
        # the input condition, on the restatement alone: equality is not vacuous
        dark, lit = int((want[covered] == 0).sum()), int((want[covered] == 255).sum())
        print("%s jitter %g: %d covered pixels store 0, %d store 255" % (name, jitter, dark, lit))
        assert dark >= 200 and lit >= 200
        assert (want[~covered] == 255).all()  # sky: wposh.w == 0, a non-finite ray
    # the restatement of the pass is the per-ray trace over its rays
    full = shref.shadow_trace(sd, sc, sc["depth"], np.full((h, w), 0x5A, np.uint8), 1)
    assert full.reshape(-1).tobytes() == want.tobytes()


def test_fuzz_equals_the_brute_force(shref):
    scene = SH.fuzz_scene()
    assert sorted(set(scene["draws"]["postPass"].tolist())) == [0, 1, 2]
    o, d = SH.fuzz_rays(scene, 201000)
    hits = _same("fuzz", scene, _build(scene), shref, o, d)[0]
    assert 20000 < hits[0] < hits[1] < 180000  # both outcomes, and the post-pass instances cast only at quality 1


def test_degenerate_rays_equal_the_brute_force(shref):
    scene = SH.aligned_scene()
    o, d = SH.degenerate_rays(scene)
    assert ((d == 0).sum(1) == 2).sum() > 5000 and not np.isfinite(o).all() and not np.isfinite(d).all()
    hits = _same("degenerate", scene, _build(scene), shref, o, d)[0]
    assert hits[0] > 1000 and hits[1] > hits[0]
    # non-finite rays and the zero direction hit nothing
    bad = ~(np.isfinite(o).all(1) & np.isfinite(d).all(1)) | (d == 0).all(1)
    assert bad.sum() == 19 and (shref.trace(scene, o[bad], d[bad], 1) == 255).all()
    # a ray through a shared edge or vertex of the closed box is not lost between its triangles: from outside, every axis-aligned ray whose
    # line meets the closed unit box (instance 0, alone in a scene) is occluded
    alone = dict(scene, draws=scene["draws"][:1])
    g = np.arange(-4, 5) * 0.25
    u, v = np.meshgrid(g, g)
    for k in range(3):
        pts = np.zeros((u.size, 3), np.float32)
        pts[:, (k + 1) % 3], pts[:, (k + 2) % 3], pts[:, k] = u.reshape(-1), v.reshape(-1), -3.0
        dirs = np.broadcast_to(np.eye(3, dtype=np.float32)[k], pts.shape)
        assert (shref.trace(alone, pts, dirs, 0) == 0).all()
        assert (host.rt_scene_trace_host(_build(alone), pts, dirs, 0) == 0).all()


def _variant(**kw):
    """aligned_scene with one rule exercised"""
    s = SH.aligned_scene()
    s = dict(s, meshes=s["meshes"].copy(), draws=s["draws"].copy(), indices=s["indices"].copy())
    for k, f in kw.items():
        f(s)
    return s


def _set(path, value):
    def f(s):
        a, field, i = path
        s[a][field][i] = value
    return f


RULES = {
    "scale 0": dict(a=_set(("draws", "scale", 0), 0.0)),
    "scale negative": dict(a=_set(("draws", "scale", 0), -1.0)),
    "scale NaN": dict(a=_set(("draws", "scale", 1), np.nan)),
    "position inf": dict(a=_set(("draws", "position", 0), (np.inf, 0, 0))),
    "orientation NaN": dict(a=_set(("draws", "orientation", 2), (0, np.nan, 0, 1))),
    "meshIndex past the meshes": dict(a=_set(("draws", "meshIndex", 0), 2)),
    "lodRT past lodCount": dict(a=_set(("meshes", "lodRT", 1), 1)),
    "lodRT past 8": dict(a=_set(("meshes", "lodRT", 1), 8), b=_set(("meshes", "lodCount", 1), 9)),
    "indexCount 0": dict(a=lambda s: s["meshes"]["lods"]["indexCount"].__setitem__((1, 0), 0)),
    "indexCount 2": dict(a=lambda s: s["meshes"]["lods"]["indexCount"].__setitem__((0, 0), 2)),
    "index past the vertices": dict(a=lambda s: s["indices"].__setitem__(slice(40, 60), 1 << 30)),
    "index buffer cut short": dict(a=lambda s: s.__setitem__("indices", s["indices"][:100])),
    "vertex buffer cut short": dict(a=lambda s: s.__setitem__("vertices", s["vertices"][:40])),
    "non-unit quaternion": dict(a=_set(("draws", "orientation", 0), (0.3, -0.2, 0.4, 1.5))),
    "zero draws": dict(a=lambda s: s.__setitem__("draws", s["draws"][:0])),
    "zero meshes": dict(a=lambda s: s.__setitem__("meshes", s["meshes"][:0])),
}


@pytest.mark.parametrize("rule", sorted(RULES))
def test_rule_cases_equal_the_brute_force(rule, shref):
    base = SH.aligned_scene()
    s = _variant(**RULES[rule])
    blob = _build(s)
    assert host.rt_scene_validate(blob)
    o, d = SH.degenerate_rays(base)
    o2, d2 = SH.fuzz_rays(dict(base, draws=base["draws"]), 3000, seed=5)
    o, d = np.concatenate([o[::3], o2]), np.concatenate([d[::3], d2])
    hits = _same(rule, s, blob, shref, o, d)[0]
    base_hits = int((shref.trace(base, o, d, 1) == 0).sum())
    print("%s: %d occluded at quality 1 (the unchanged scene: %d)" % (rule, hits[1], base_hits))
    if rule == "non-unit quaternion":
        assert hits[1] > 0
    elif rule in ("zero draws", "zero meshes"):
        assert hits[1] == 0 and host.rt_scene_stats(blob)["instances"] == 0
    else:
        assert hits[1] < base_hits  # the rule removed casters


# ---------------------------------------------------------------------------------------------------------------- the degenerate rays as launches

def test_the_lattice_construction_is_exact(shref):
    """shadow_ref.lattice_launch's hand-made matrix: the rays of the pass are the intended lattice and +-e_k, component for component.
    tests/test_shadow_degenerate_gpu.py hands the same launches to the device kernels"""
    base = SH.aligned_scene()
    rays = 0
    for scene in (base, dict(base, draws=SH.moved_exactly(base))):
        for dr in scene["draws"]:
            p, s = dr["position"].astype(np.float64), float(dr["scale"])
            for k in range(3):
                for sign in (1.0, -1.0):
                    for start in SH.AXIS_STARTS:
                        third = p[k] + sign * start * s
                        o, d = shref.rays(*SH.lattice_launch(p, s, k, third, np.eye(3)[k] * sign))
                        assert np.array_equal(o.astype(np.float64), SH.lattice_points(p, s, k, third))
                        assert np.array_equal(d, np.broadcast_to((np.eye(3)[k] * sign).astype(np.float32), d.shape))
                        rays += o.size // 3
    print("lattice construction: %d rays, every component equal" % rays)
    assert rays == 2 * 18432
    # the comparison notices one ulp in any of the matrix's five entries
    p, s, k, third = np.zeros(3), 1.0, 0, -3.0
    want = SH.lattice_points(p, s, k, third)
    sd, depth = SH.lattice_launch(p, s, k, third, (1.0, 0.0, 0.0))
    entries = np.flatnonzero(sd["inverseViewProjection"][0])
    assert entries.tolist() == [1, 6, 8, 13, 14, 15]
    for e in entries[:-1]:
        for toward in (np.inf, -np.inf):
            bent = sd.copy()
            bent["inverseViewProjection"][0, e] = np.nextafter(sd["inverseViewProjection"][0, e], np.float32(toward))
            assert not np.array_equal(shref.rays(bent, depth)[0].astype(np.float64), want), (e, toward)


@pytest.mark.parametrize("which", ["aligned", "extreme"])
def test_degenerate_launches_equal_the_brute_force(which, shref):
    """every launch of shadow_ref.degenerate_launches: the host twin of the kernel's traversal against the brute force on the rays of the
    pass, both qualities, zero differences; the input conditions on the restatement alone"""
    scene = SH.aligned_scene() if which == "aligned" else SH.extreme_scene()
    blob = _build(scene)
    assert host.rt_scene_validate(blob)
    launches = SH.degenerate_launches(scene)
    o, d, fam = SH.launch_rays(shref, launches)
    masks = {}
    shref.fp64_rays()
    for q in (0, 1):
        masks[q] = SH.in_chunks(lambda a, b: shref.trace(scene, a, b, q), o, d)
        got = host.rt_scene_trace_host(blob, o, d, q)
        diff = int((masks[q] != got).sum())
        print("%s quality %d: %d launches, %d rays, %d occluded, %d differences" % (which, q, len(launches), len(o), int((masks[q] == 0).sum()), diff))
        assert diff == 0
    branch = shref.fp64_rays()
    print("%s: %d rays took the fp64 branch of T against a casting triangle (both qualities)" % (which, branch))
    assert branch >= 1000
    SH.input_conditions(which, o, d, fam, masks)
    # the graze family: rays for which the branch turns an fp32 zero of U, V or W into a sign, so that its precision decides texels (a
    # device build whose branch ran in fp32 answers some of them differently: EXPERIMENTS.md)
    shref.fp64_decided_rays()
    graze = fam == "graze"
    lit = int((shref.trace(scene, o[graze], d[graze], 1) == 255).sum())
    decided = shref.fp64_decided_rays()
    print("%s: graze family: %d rays, %d lit, the fp64 branch decides a zero in %d of them" % (which, int(graze.sum()), lit, decided))
    assert decided >= 100 and lit >= 100 and graze.sum() - lit >= 100
    # the restatement of the pass is the per-ray trace over its rays
    some = launches[::37]
    for q in (0, 1):
        full = SH.reference_masks(shref, scene, some, q)
        assert full.reshape(-1).tobytes() == np.concatenate([masks[q][256 * i:256 * i + 256] for i in range(0, len(launches), 37)]).tobytes()
    alone, six = SH.closed_box_launches(scene)
    SH.closed_box_property(which, SH.reference_masks(shref, alone, six, 0))
    o6, d6, _ = SH.launch_rays(shref, six)
    assert (host.rt_scene_trace_host(_build(alone), o6, d6, 0).reshape(6, 16, 16) == SH.reference_masks(shref, alone, six, 0)).all()
    if which == "extreme":
        import tlas_ref as TR
        leaves = SH.infinite_leaves(TR.sections(blob)[1])
        print("extreme: %d TLAS leaves with the infinite box" % len(leaves))
        assert len(leaves) >= 1


def test_the_standalone_program_runs_clean_under_the_host_sanitizers(tmp_path):
    """tools/rt_scene_check.cpp with rtbuild.cpp, host code only, its own main: AddressSanitizer and UBSan linked statically into the program itself"""
    exe = tmp_path / "rt_scene_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "rt_scene_check.cpp"),
                           os.path.join(ROOT, "niagara_amd", "csrc", "rtbuild.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    print(out.stdout.decode())
    assert out.returncode == 0 and b"rt_scene_check: ok" in out.stdout
