"""The alpha-tested shadow trace on the CPU: nv_rt_scene_build_textured's blob, the validator's flag check, the host TLAS
rebuild, and nv_rt_scene_trace_host_textured_rays (the text the kernel runs, niagara_amd/csrc/rtalpha.h) against the brute-force restatement
tests/shadow_alpha_ref.c — zero differences on every ray.  The restatement has no BVH and ends no loop early, so it also says per ray how many
accepted candidates the alpha test rejected: the input conditions below are asserted on it alone."""
import os
import subprocess

import numpy as np
import pytest

import oracle
import shadow_alpha_ref as SA
import shadow_ref as SH
import visbuffer_ref as VB
import niagara_amd as N
from niagara_amd import host, synth
from niagara_amd import layouts as L
from niagara_amd._lib import NvError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUN = np.array([2.0, 0.3, 1.0]) / np.linalg.norm([2.0, 0.3, 1.0])  # tests/test_shadowtrace_cpu.py records why
FUZZ_RAYS = 100_000
# the fuzz scene's values are shadow_alpha_ref.FUZZ: 20 instances within +-8 (the rays meet several instances), 60 % of the draws in the post
# pass, six textures whose texels are clear or solid with equal odds.  On the restatement they give 3230 rays whose byte differs from the
# alpha = 1 mask and 39790 occluded rays with a rejected candidate (needed: 1000 and 200).
BOX_SCALE = 3.0  # the cut-out occluder scene: boxes large enough that the wall's shadow on them covers some 1500 texels at 320 x 192

HEADER = np.dtype([(n, "<u4") for n in ("magic", "version", "bytes", "meshCount", "tlasNodes", "instances", "blasNodes", "triangles", "tableOff", "tlasOff",
                                         "instOff", "blasOff", "triOff")] + [("padOrigin", "<f4"), ("drawCount", "<u4"), ("flags", "<u4")])
BLAS = np.dtype([("nodeFirst", "<u4"), ("nodeCount", "<u4"), ("triFirst", "<u4"), ("triCount", "<u4"), ("maxAbs", "<f4"), ("maxExtent", "<f4"), ("reserved", "<u4", 2)])


@pytest.fixture(scope="session")
def aref(tmp_path_factory):
    return SA.load(tmp_path_factory.mktemp("shadow_alpha_ref_cpu"))


@pytest.fixture(scope="session")
def shref(tmp_path_factory):
    return SH.load(tmp_path_factory.mktemp("shadow_ref_alpha_cpu"))


@pytest.fixture(scope="module")
def fuzz():
    s, t = SA.textured_fuzz_scene()
    o, d = SH.fuzz_rays(s, FUZZ_RAYS)
    return s, t, o, d


def _build(scene, texcoords=True):
    return host.rt_scene_build(scene["meshes"], scene["indices"], scene["vertices"], scene["draws"], texcoords=texcoords)


def _host(blob, scene, tset, o, d, quality=1, **kw):
    return host.rt_scene_trace_host_textured(blob, o, d, scene["draws"], scene["materials"], tset["descs"], tset["texels"], quality, **kw)


def _header(blob):
    return blob[:64].view(HEADER)[0]


def _triangles(blob):
    """(n, 3, 4) uint32 view of the triangle section: x, y, z bits and the w word of every corner"""
    h = _header(blob)
    return blob[int(h["triOff"]):int(h["triOff"]) + int(h["triangles"]) * 48].view(np.uint32).reshape(-1, 3, 4)


def _same(name, aref, scene, tset, o, d, blob=None):
    blob = _build(scene) if blob is None else blob
    want, rejected = aref.trace(scene, tset, o, d, 1)
    got = _host(blob, scene, tset, o, d)
    diff = int((want != got).sum())
    print("%s: %d rays, %d occluded, %d with a rejected candidate, %d differences" % (name, len(want), int((want == 0).sum()), int((rejected > 0).sum()), diff))
    assert diff == 0 and set(np.unique(want).tolist()) <= {0, 255}
    return want, rejected


# ---------------------------------------------------------------------------------------------------------------- ABI, blob

def test_library_exports_the_entry_points_and_refuses_bad_arguments(fuzz):
    for f in ("nv_rt_scene_build_textured", "nv_rt_scene_trace_host_textured_rays", "nv_shadow_trace_textured", "nv_rt_alpha_sample_host"):
        assert hasattr(N.lib, f)
    s, t, o, d = fuzz
    plain = _build(s, texcoords=False)
    with pytest.raises(NvError):  # a blob without the texcoord flag
        _host(plain, s, t, o[:4], d[:4])
    with pytest.raises(NvError):
        _host(_build(s), s, t, o[:4], d[:4], quality=2)
    n = np.zeros(1, np.uint64)
    assert N.lib.nv_rt_scene_build_textured(None, 1, None, 0, None, 0, None, 0, None, n.ctypes.data_as(N._lib.C.POINTER(N._lib.C.c_uint64))) != 0


@pytest.mark.parametrize("name", ["fuzz", "occluder"])
def test_the_textured_blob_is_the_plain_blob_plus_texcoords(name, fuzz):
    s = fuzz[0] if name == "fuzz" else synth.with_textures(synth.occluder_scene_indexed(meshlet_bounds=oracle.meshlet_bounds))
    plain, tex = _build(s, texcoords=False), _build(s)
    assert host.rt_scene_validate(plain) and host.rt_scene_validate(tex)
    assert _header(plain)["flags"] == 0 and _header(tex)["flags"] == 1
    assert (_triangles(plain)[:, :, 3] == 0).all()
    zeroed = tex.copy()
    zeroed[60:64] = 0
    _triangles(zeroed)[:, :, 3] = 0
    assert zeroed.tobytes() == plain.tobytes()
    # every triangle's w words are the packed texcoords of a source triangle with those three positions in that corner order
    h = _header(tex)
    table = tex[int(h["tableOff"]):int(h["tableOff"]) + int(h["meshCount"]) * 32].view(BLAS)
    tris = _triangles(tex)
    m, idx, v = s["meshes"], s["indices"].astype(np.int64), s["vertices"]
    pos = np.stack([v[k].view(np.float16).astype(np.float32) for k in ("vx", "vy", "vz")], 1).view(np.uint32)
    tc = v["tu"].astype(np.uint32) | v["tv"].astype(np.uint32) << 16
    checked = 0
    for mi in range(len(m)):
        lod = m["lods"][mi][int(m["lodRT"][mi])]
        corners = idx[int(lod["indexOffset"]):int(lod["indexOffset"]) + int(lod["indexCount"]) // 3 * 3].reshape(-1, 3) + int(m["vertexOffset"][mi])
        source = {}
        for c in corners:
            source.setdefault(pos[c].tobytes(), set()).add(tuple(int(x) for x in tc[c]))
        first, count = int(table["triFirst"][mi]), int(table["triCount"][mi])
        assert count == len(corners)
        for t in tris[first:first + count]:
            assert tuple(int(x) for x in t[:, 3]) in source[np.ascontiguousarray(t[:, :3]).tobytes()]
            checked += 1
    assert checked == len(tris) and (tris[:, :, 3] != 0).any()


def test_the_validator_accepts_flag_bit_0_alone(fuzz):
    s, t, o, d = fuzz
    blob = _build(s)
    for flags, ok in ((0, True), (1, True), (2, False), (3, False), (0x80000000, False), (0x80000001, False), (0x100, False)):
        b = blob.copy()
        b[60:64].view(np.uint32)[0] = flags
        assert host.rt_scene_validate(b) == ok, hex(flags)
    # any bit pattern in a w word is safe: the blob validates and walks
    b = blob.copy()
    w = _triangles(b)
    w[:, :, 3] = np.random.default_rng(3).integers(0, 1 << 32, w[:, :, 3].shape, dtype=np.uint64).astype(np.uint32)
    w[::5, 0, 3], w[1::5, 1, 3], w[2::5, 2, 3] = 0x7c007e00, 0xfc00ffff, 0x7fff7c01  # inf, nan halves
    assert host.rt_scene_validate(b)
    got = _host(b, s, t, o[:5000], d[:5000])
    assert set(np.unique(got).tolist()) <= {0, 255}


def test_the_host_tlas_rebuild_keeps_the_flag_and_the_texcoords(fuzz):
    s = fuzz[0]
    moved = s["draws"].copy()
    moved["position"] += np.random.default_rng(5).uniform(-2, 2, moved["position"].shape).astype(np.float32)
    for texcoords in (True, False):
        blob = _build(s, texcoords=texcoords)
        out = host.rt_tlas_build_host(blob, moved)
        assert host.rt_scene_validate(out)
        assert _header(out)["flags"] == (1 if texcoords else 0)
        assert _triangles(out).tobytes() == _triangles(blob).tobytes()
        again = host.rt_tlas_build_host(out, s["draws"])  # and through a second rebuild
        assert _header(again)["flags"] == _header(blob)["flags"] and _triangles(again).tobytes() == _triangles(blob).tobytes()


# ---------------------------------------------------------------------------------------------------------------- the four-tap alpha

def test_the_four_tap_alpha_is_the_samplers_w_bit_for_bit():
    """rtalpha.h's rt_alpha_lod0 against tx_sample_lod0(...).w of texmath.h over random textures (one-level chains, non-square and one-texel
    sizes among them) and uv: finite of every magnitude, exact texel edges and their neighbours, and non-finite.  Every number is compared by
    its bits.  Where the sampler gives a NaN (a non-finite uv) the four-tap form must give a NaN too; the sign and payload of a NaN are not
    compared: IEEE 754 leaves open which operand's NaN an operation hands on, the host compiler is free in the operand order of a commutative
    instruction, and the alpha test asks nothing of a NaN but that it is not >= 0.5"""
    rng = np.random.default_rng(9)
    shapes = [(8, 8, 1), (5, 3, 2), (1, 1, 1), (16, 4, 3), (7, 1, 1), (2, 9, 2), (64, 32, 7), (3, 3, 1), (1, 6, 3)]
    total = nans = 0
    for w, h, levels in shapes:
        chain = [rng.integers(0, 256, (max(1, h >> l), max(1, w >> l), 4)).astype(np.uint8) for l in range(levels)]
        tset = SA.texture_set([chain])
        uv = rng.normal(size=(4000, 2)) * np.exp(rng.uniform(np.log(1e-3), np.log(1e6), (4000, 1)))
        k = rng.integers(-3 * w, 3 * w, (600, 2)).astype(np.float64) / (w, h)
        edges = np.concatenate([k, np.nextafter(k.astype(np.float32), np.float32(np.inf)), np.nextafter(k.astype(np.float32), np.float32(-np.inf)),
                                k + 0.5 / np.array([w, h])])
        special = np.array([0.0, -0.0, 1.0, -1.0, 1e-45, -1e-45, -1e-8, 1e30, -1e30, 3.4e38, np.inf, -np.inf, np.nan], np.float32)
        grid = np.stack(np.meshgrid(special, special), -1).reshape(-1, 2)
        uv = np.concatenate([uv, edges, grid]).astype(np.float32)
        four, full = host.rt_alpha_sample_host(tset["descs"][1], tset["texels"], uv)
        nan = np.isnan(full)
        assert (np.isnan(four) == nan).all() and four[~nan].view(np.uint32).tobytes() == full[~nan].view(np.uint32).tobytes(), (w, h, levels)
        finite = np.isfinite(uv).all(axis=1)
        assert np.isnan(four[~finite]).all() and ((four[finite] >= 0) & (four[finite] <= 1)).all()
        for i in range(0, len(uv), 97):  # and the public sampler entry point says the same
            ref = host.texture_sample_host(tset["descs"], tset["texels"], 1, uv[i])[3]
            assert np.float32(ref).view(np.uint32) == four[i].view(np.uint32) or (np.isnan(ref) and np.isnan(four[i]))
        total += len(uv)
        nans += int((~finite).sum())
    print("four-tap alpha: %d samples over %d textures, %d of them at non-finite uv, 0 differences" % (total, len(shapes), nans))


# ---------------------------------------------------------------------------------------------------------------- against the restatement

def test_fuzz_equals_the_restatement_and_exercises_the_loop(fuzz, aref, shref):
    s, t, o, d = fuzz
    assert len(o) >= 100_000
    want, rejected = _same("fuzz", aref, s, t, o, d)
    opaque = shref.trace(s, o, d, 1)
    differs = int((want != opaque).sum())
    past = int(((want == 0) & (rejected > 0)).sum())
    print("fuzz input conditions: %d rays differ from the alpha = 1 mask, %d are occluded although a candidate was rejected" % (differs, past))
    assert (want[want != opaque] == 255).all()  # the alpha test only ever lights a ray
    assert differs >= 1000 and past >= 200
    # quality 0 is nv_rt_scene_trace_host_rays
    blob = _build(s)
    q0 = _host(blob, s, t, o, d, quality=0)
    assert q0.tobytes() == host.rt_scene_trace_host(blob, o, d, 0).tobytes() == shref.trace(s, o, d, 0).tobytes()
    assert aref.trace(s, t, o[:20000], d[:20000], 0)[0].tobytes() == q0[:20000].tobytes()
    # a set whose every alpha is 255 gives the untextured quality-1 mask; so does a draw array the instances' ids lie past
    solid = dict(descs=t["descs"], texels=t["texels"] | np.uint32(0xff000000))
    assert _host(blob, s, solid, o, d).tobytes() == opaque.tobytes() == host.rt_scene_trace_host(blob, o, d, 1).tobytes()
    none = host.rt_scene_trace_host_textured(blob, o, d, s["draws"][:0], s["materials"], t["descs"], t["texels"])
    assert none.tobytes() == opaque.tobytes()


def test_degenerate_rays_equal_the_restatement(aref):
    """the aligned scene's rays on edges and vertices: U, V or W is 0, T takes its fp64 branch and the barycentrics come from its values"""
    s, t = SA.textured_aligned_scene()
    o, d = SH.degenerate_rays(s)
    want, rejected = _same("degenerate", aref, s, t, o, d)
    assert int((rejected > 0).sum()) >= 200 and int((want == 0).sum()) >= 200


def test_degenerate_launches_equal_the_restatement(aref, shref):
    """every launch of shadow_ref.degenerate_launches around the textured aligned scene (tests/test_shadow_degenerate_gpu.py hands the same
    launches to the device kernels): the host twin against the restatement on the rays of the pass, zero differences"""
    s, t = SA.textured_aligned_scene()
    blob = _build(s)
    assert host.rt_scene_validate(blob)
    launches = SH.degenerate_launches(s)
    o, d, fam = SH.launch_rays(shref, launches)
    want, rejected = aref.trace(s, t, o, d, 1)
    got = _host(blob, s, t, o, d)
    diff = int((want != got).sum())
    print("degenerate launches: %d launches, %d rays, %d occluded, %d with a rejected candidate, %d differences" % (len(launches), len(want), int((want == 0).sum()),
                                                                                                            int((rejected > 0).sum()), diff))
    assert diff == 0 and set(np.unique(want).tolist()) == {0, 255}
    assert int((rejected > 0).sum()) >= 200 and int((want == 0).sum()) >= 200
    finite = np.isfinite(o).all(1) & np.isfinite(d).all(1)
    assert (~finite).sum() >= 100 and (want[~finite] == 255).all() and (want[fam == "suns"] == 255).all()
    # the restatement of the pass is the per-ray trace over its rays; quality 0 is the opaque trace
    some = launches[::37]
    full, _ = SA.reference_masks(aref, s, t, some, 1)
    assert full.reshape(-1).tobytes() == np.concatenate([want[256 * i:256 * i + 256] for i in range(0, len(launches), 37)]).tobytes()
    q0 = _host(blob, s, t, o, d, quality=0)
    assert q0.tobytes() == shref.trace(s, o, d, 0).tobytes() == aref.trace(s, t, o, d, 0)[0].tobytes()


def cutout_occluder():
    """the occluder scene with its wall in the post pass and with_textures' cut-out albedo (the wall's texcoords span one period of the 8 x 8
    checker), boxes of scale BOX_SCALE, the index buffer of the classic path, and the set decoded on the CPU"""
    s = synth.with_textures(synth.occluder_scene_indexed(meshlet_bounds=oracle.meshlet_bounds, box_scale=BOX_SCALE), cutout=True)
    s["draws"] = s["draws"].copy()
    s["draws"]["postPass"][s["wall"]] = 1
    descs, texels = host.texture_decode_host(s["textures"])
    return s, dict(descs=descs, texels=texels)


def test_the_passes_rays_over_the_cutout_occluder_equal_the_restatement(aref, shref, tmp_path_factory):
    s, t = cutout_occluder()
    w, h = s["viewport"]
    vref = VB.load(tmp_path_factory.mktemp("visbuffer_ref_alpha_cpu"))
    depth = np.ascontiguousarray(VB.oracle_frames(s, 2, True, vref, 0)[-1]["post"]["depth"], np.float32).reshape(h, w)
    covered = (depth > 0).reshape(-1)
    blob = _build(s)
    for jitter in (0.0, 1e-2):
        sd = host.build_shadow_data(synth.make_globals(s["cull"], (w, h)), SUN, jitter, 0, w, h)
        o, d = shref.rays(sd, depth)
        want, rejected = _same("cut-out occluder jitter %g" % jitter, aref, s, t, o, d, blob)
        opaque = shref.trace(s, o, d, 1)
        print("cut-out occluder: %d covered texels, %d in shadow, %d with the opaque wall, %d differ" % (int(covered.sum()), int((want[covered] == 0).sum()),
                                                                                                    int((opaque[covered] == 0).sum()), int((want != opaque)[covered].sum())))
        assert (want != opaque)[covered].sum() >= 200 and (want[covered] == 0).sum() >= 200
        assert (want[~covered] == 255).all()
    full, _ = aref.shadow_trace(sd, s, t, depth, np.full((h, w), 0x5A, np.uint8), 1)
    assert full.reshape(-1).tobytes() == want.tobytes()  # the restatement of the pass is the per-ray trace over its rays


# ---------------------------------------------------------------------------------------------------------------- rule cases

def _wall(post_pass=(1,), z=(6.0,), alpha=(0,), uv_scale=1.0, uv_shift=0.0, tu=None):
    """walls (mesh 0 at scale 4, facing +z) at heights z with materials 0, 1, .. naming textures 1, 2, ..: flat 1 x 1 textures of the given
    alpha codes (or full chains); texcoords (x, y) * 0.5 + 0.5, scaled and shifted"""
    s, _ = SA.layered_scene()
    v = s["vertices"].copy()
    uv = np.stack([v["tu"], v["tv"]], -1).view(np.float16).astype(np.float32) * uv_scale + uv_shift
    uv = uv.astype(np.float16)
    v["tu"], v["tv"] = uv[:, 0].view(np.uint16), uv[:, 1].view(np.uint16)
    if tu is not None:
        v["tu"] = tu
    n = len(z)
    draws = np.zeros(n, L.MESHDRAW)
    draws["orientation"], draws["scale"], draws["meshIndex"] = (0.0, 0.0, 0.0, 1.0), 4.0, 0
    draws["position"] = [(0.0, 0.0, zz) for zz in z]
    draws["postPass"], draws["materialIndex"] = post_pass, np.arange(n)
    m = np.zeros(n, L.MATERIAL)
    m["albedoTexture"] = np.arange(n) + 1
    t = SA.texture_set([a if isinstance(a, list) else SA.flat_texture(a) for a in alpha])
    return dict(s, vertices=v, draws=draws, materials=m), t


def _up_rays():
    """a handful of rays from z = 0 straight up through the walls, off the mesh's edges and on them"""
    g = np.array([-3.3, -1.7, -0.4, 0.0, 0.9, 2.0, 3.1])
    x, y = np.meshgrid(g, g)
    o = np.stack([x.reshape(-1), y.reshape(-1), np.zeros(x.size)], 1).astype(np.float32)
    return o, np.broadcast_to(np.array([0, 0, 1], np.float32), o.shape).copy()


def _inverted_chain(rng):
    """16 x 4 with three levels: level 0 random clear / solid texels, levels 1 and 2 solid where... everything level 0 is not: all 255 where a
    mip of level 0 would be clear and the reverse, so a sampler that touched them would change the mask"""
    l0 = np.full((4, 16, 4), 99, np.uint8)
    l0[..., 3] = np.where(rng.random((4, 16)) < 0.5, 0, 255)
    l1, l2 = np.full((2, 8, 4), 99, np.uint8), np.full((1, 4, 4), 99, np.uint8)
    l1[..., 3] = 255 - l0[::2, ::2, 3]
    l2[..., 3] = 255 - l0[::4, ::4, 3]
    return [l0, l1, l2]


def _case(name):
    rng = np.random.default_rng(77)
    if name == "alpha 127 is lit":
        return _wall(alpha=(127,)), "lit"
    if name == "alpha 128 is shadow":
        return _wall(alpha=(128,)), "shadow"
    if name == "albedoTexture 0":
        (s, t) = _wall(alpha=(0,))
        s["materials"]["albedoTexture"] = 0
        return (s, t), "shadow"
    if name == "material index out of range":
        (s, t) = _wall(alpha=(0,))
        s["draws"]["materialIndex"] = 1
        return (s, t), "shadow"
    if name == "texture id out of range":
        (s, t) = _wall(alpha=(0,))
        s["materials"]["albedoTexture"] = 2
        return (s, t), "shadow"
    if name == "descriptor past the texels":
        (s, t) = _wall(alpha=(0,))
        t["descs"]["offset"][1] = 1
        return (s, t), "shadow"
    if name == "descriptor with no levels":
        (s, t) = _wall(alpha=(0,))
        t["descs"]["levels"][1] = 0
        return (s, t), "shadow"
    if name == "descriptor with 16 levels":
        (s, t) = _wall(alpha=(0,))
        t["descs"]["levels"][1] = 16
        return (s, t), "shadow"
    if name == "postPass 0 ignores its transparent texture":
        return _wall(post_pass=(0,), alpha=(0,)), "shadow"
    if name == "postPass 2 never casts":
        return _wall(post_pass=(2,), alpha=(255,)), "lit"
    if name == "only level 0 counts":
        return _wall(alpha=(_inverted_chain(rng),), uv_scale=1.0), "mixed"
    if name == "uv scaled by 3 and shifted by -2":
        return _wall(alpha=(_inverted_chain(rng)[:1],), uv_scale=3.0, uv_shift=-2.0), "mixed"
    if name == "a transparent texel in front of an opaque caster":
        return _wall(post_pass=(1, 0), z=(3.0, 6.0), alpha=(0, 0)), "shadow past a rejection"
    if name == "two transparent layers":
        return _wall(post_pass=(1, 1), z=(3.0, 6.0), alpha=(0, 100)), "lit past two rejections"
    if name == "inf texcoords":
        return _wall(alpha=(255,), tu=0x7c00), "lit"
    if name == "nan texcoords":
        return _wall(alpha=(255,), tu=0x7e00), "lit"
    raise KeyError(name)


RULES = ["alpha 127 is lit", "alpha 128 is shadow", "albedoTexture 0", "material index out of range", "texture id out of range", "descriptor past the texels",
         "descriptor with no levels", "descriptor with 16 levels", "postPass 0 ignores its transparent texture", "postPass 2 never casts", "only level 0 counts",
         "uv scaled by 3 and shifted by -2", "a transparent texel in front of an opaque caster", "two transparent layers", "inf texcoords", "nan texcoords"]


@pytest.mark.parametrize("rule", RULES)
def test_rule_cases(rule, aref):
    (s, t), expect = _case(rule)
    o, d = _up_rays()
    want, rejected = _same(rule, aref, s, t, o, d)
    if expect == "lit":
        assert (want == 255).all()
    elif expect == "shadow":
        assert (want == 0).all() and (rejected == 0).all()
    elif expect == "mixed":
        assert set(np.unique(want).tolist()) == {0, 255}
    elif expect == "shadow past a rejection":
        assert (want == 0).all() and (rejected >= 1).all()
    elif expect == "lit past two rejections":
        assert (want == 255).all() and (rejected >= 2).all()
    if rule == "only level 0 counts":  # the same level 0 alone gives the same mask
        one = SA.texture_set([[t["texels"][:64].view(np.uint8).reshape(4, 16, 4)]])
        assert aref.trace(s, one, o, d, 1)[0].tobytes() == want.tobytes()


def test_the_standalone_program_runs_clean_under_the_host_sanitizers(tmp_path):
    """tools/rt_alpha_check.cpp with rtbuild.cpp, host code only, its own main: AddressSanitizer and UBSan linked statically into the program itself"""
    exe = tmp_path / "rt_alpha_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "rt_alpha_check.cpp"),
                           os.path.join(ROOT, "niagara_amd", "csrc", "rtbuild.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    print(out.stdout.decode())
    assert out.returncode == 0 and b"rt_alpha_check: ok" in out.stdout
