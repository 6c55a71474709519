"""The shadow fixtures without the reference tree and without a GPU: tests/golden/shadow/*.npz hold what the
reference's own shadow.comp.glsl, run on the CPU against the ray query of oracle/glsl_rayquery_shim.h, makes of fixed inputs
(tests/golden/generate.py, section `shadow`; tests/test_shadow_vs_ref.py is the live form of the same pin).  The restatements
tests/shadow_ref.c and tests/shadow_alpha_ref.c replay every fixture byte for byte, prefill bytes included, and the ray of every storing
invocation bit for bit; so do the host twins of the kernels (nv_rt_scene_trace_host_rays, nv_rt_scene_trace_host_textured_rays: the text the
kernels run) over the fixture's rays, on a blob from nv_rt_scene_build / nv_rt_scene_build_textured and on one whose TLAS
nv_rt_tlas_build_host rebuilt.  No tolerance: nothing here holds pow or exp2.  tests/test_shadow_fixtures_gpu.py is the device's replay."""
import os

import numpy as np
import pytest

import shadow_alpha_ref as SA
import shadow_cases as SC
import shadow_ref as SH
from niagara_amd import host

FILES = SC.FIXTURES


def _launches(f):
    return range(len(f["sd"]))


@pytest.fixture(scope="module")
def shref(tmp_path_factory):
    return SH.load(tmp_path_factory.mktemp("shadow_ref_fixtures"))


@pytest.fixture(scope="module")
def aref(tmp_path_factory):
    return SA.load(tmp_path_factory.mktemp("shadow_alpha_ref_fixtures"))


def _zero(name, ok):
    ok = np.asarray(ok)
    print("%s: %d elements, %d differ" % (name, ok.size, int((~ok).sum())))
    assert ok.all(), "%s: %d of %d differ, first at %s" % (name, int((~ok).sum()), ok.size, np.argwhere(~ok)[:4].tolist())


def _poison(f):
    return np.full(f["depth"].shape, SC.PREFILL, np.uint8)


def test_the_fixtures_are_the_three_sizes_and_stay_small():
    """(and the range case's file; nothing else lies in the directory)"""
    total = sum(os.path.getsize(p) for p in FILES)  # (a missing file fails here)
    assert sorted(os.listdir(SC.GOLDEN)) == sorted(os.path.basename(p) for p in FILES)
    print("tests/golden/shadow: %d bytes" % total)
    assert total <= os.path.getsize(os.path.join(SC.HERE, "golden", "mesh", "kitten.npz"))  # the cap tests/test_shade_fixtures_cpu.py applies


@pytest.mark.parametrize("path", SC.SIZE_FIXTURES, ids=SC.FIXTURE_IDS[:len(SC.SIZE_FIXTURES)])
def test_the_fixtures_hold_both_outcomes_and_the_scenes_the_live_pin_uses(path):
    """what the replays below rest on, from the fixture alone: the launches are the (checkerboard, sunJitter) pairs named in shadow_cases; every
    owned texel is 0 or 255 and everything else the prefill byte; the larger images hold lit and shadowed texels in every mask; the scene has
    the properties the live pin's scenes were given (a mesh that traces LOD 1, postPass {0, 2} among the opaque draws and 1 among the
    textured ones, a material without a texture and one past the table); the decoded set is the decode of the stored files"""
    f = np.load(path)
    h, w = f["depth"].shape
    assert "%dx%d.npz" % (w, h) == os.path.basename(path) and len(f["sd"]) == len(SC.FIXTURE_LAUNCHES)
    for k, (cb, jitter) in enumerate(SC.FIXTURE_LAUNCHES):
        sd, depth = SC.fixture_launch(f, k)
        assert int(sd["checkerboard"][0]) == cb and float(sd["sunJitter"][0]) == np.float32(jitter) and sd["imageSize"][0].tolist() == [w, h]
        own = SC.owned(w, h, cb)
        logged = f["rays_%d" % k][..., 6] != 0  # tmin of a storing invocation
        assert (logged == own).all() and (depth == 0).any()
        for name in ("mask_q0_%d", "mask_q1_%d", "mask_tex_%d"):
            m = f[name % k]
            assert (m[~own] == SC.PREFILL).all() and np.isin(m[own], (0, 255)).all()
            print("%s %s: %d lit, %d shadowed, %d kept" % (os.path.basename(path), name % k, int((m == 255).sum()), int((m == 0).sum()), int((m == SC.PREFILL).sum())))
            assert w * h < 1000 or ((m == 255).sum() >= 100 and (m == 0).sum() >= 100)
        assert (f["mask_q0_%d" % k] == f["mask_q1_%d" % k]).all()  # no post-pass caster among draws_opaque
    s, t = SC.fixture_scene(f, True)
    assert s["meshes"]["lodRT"].tolist() == [1, 0] and (s["meshes"]["lods"]["indexOffset"][:, 1] != s["meshes"]["lods"]["indexOffset"][:, 0]).all()
    assert set(SC.fixture_scene(f, False)[0]["draws"]["postPass"].tolist()) == {0, 2} and set(s["draws"]["postPass"].tolist()) == {0, 1, 2}
    assert (s["materials"]["albedoTexture"] == 0).sum() == 1 and (s["materials"]["albedoTexture"] >= len(t["descs"])).sum() == 1
    descs, texels = host.texture_decode_host(SC.fixture_files(f))
    assert descs.tobytes() == t["descs"].tobytes() and texels.tobytes() == t["texels"].tobytes()


def test_the_range_fixture_holds_tmin_and_tmax_from_both_sides():
    """shadow_cases.range_case as the reference's shader answered it: triangles at t = 2^-7, 2^-6, 512, 1024 in front of rays along +z from z =
    0, and the masks lit, shadowed, shadowed, lit — from the stored arrays alone"""
    f = np.load(SC.RANGE_FIXTURE)
    s, t = SC.fixture_scene(f, True)
    z = s["vertices"]["vz"].view(np.float16).astype(np.float64).reshape(4, 3)
    assert (z == np.array(SC.RANGE_T)[:, None]).all() and len(f["sd"]) == 1
    rays = f["rays_0"][0]
    assert (rays[:, 2] == 0).all() and (rays[:, 3:6] == [0, 0, 1]).all() and (rays[:, 6] == SC.TMIN).all() and (rays[:, 7] == SC.TMAX).all()
    for name in ("mask_q0_0", "mask_q1_0", "mask_tex_0"):
        assert (f[name] == SC.RANGE_MASK).all(), name
    assert SC.fixture_scene(f, False)[0]["draws"]["postPass"].tolist() == [0] and s["draws"]["postPass"].tolist() == [1]
    descs, texels = host.texture_decode_host(SC.fixture_files(f))
    assert descs.tobytes() == t["descs"].tobytes() and texels.tobytes() == t["texels"].tobytes() and (texels >> 24 == 255).all()


@pytest.mark.parametrize("path", FILES, ids=SC.FIXTURE_IDS)
def test_the_restatements_replay_the_fixture(path, shref, aref):
    f = np.load(path)
    opaque, _ = SC.fixture_scene(f, False)
    textured, tset = SC.fixture_scene(f, True)
    for k in _launches(f):
        sd, depth = SC.fixture_launch(f, k)
        rays = f["rays_%d" % k]
        stored = rays[..., 6] != 0
        o, d = shref.rays(sd, depth)
        _zero("launch %d, origins" % k, SC.same_bits(o, rays[..., :3])[stored])
        _zero("launch %d, directions" % k, SC.same_bits(d, rays[..., 3:6])[stored])
        assert (rays[..., 6][stored] == SC.TMIN).all() and (rays[..., 7][stored] == SC.TMAX).all()
        for q in (0, 1):
            _zero("launch %d, quality %d" % (k, q), shref.shadow_trace(sd, opaque, depth, _poison(f), q) == f["mask_q%d_%d" % (q, k)])
        got, _ = aref.shadow_trace(sd, textured, tset, depth, _poison(f), 1)
        _zero("launch %d, textured" % k, got == f["mask_tex_%d" % k])
        plain = shref.shadow_trace(sd, textured, depth, _poison(f), 1)
        print("launch %d: the alpha test changes %d texels" % (k, int((plain != f["mask_tex_%d" % k]).sum())))
        assert depth.size < 1000 or (plain != f["mask_tex_%d" % k]).sum() >= 20


@pytest.mark.parametrize("rebuilt", [False, True], ids=["built", "rebuilt TLAS"])
@pytest.mark.parametrize("path", FILES, ids=SC.FIXTURE_IDS)
def test_the_host_twins_replay_the_fixture(path, rebuilt):
    """the fixture's rays through the kernels' own traversal on the CPU.  rebuilt: the blob is built over the draws at other positions
    (shadow_cases.moved) and its TLAS is then rebuilt by nv_rt_tlas_build_host from the fixture's draws"""
    f = np.load(path)
    opaque, _ = SC.fixture_scene(f, False)
    textured, tset = SC.fixture_scene(f, True)

    def blob(s, texcoords):
        if not rebuilt:
            return host.rt_scene_build(s["meshes"], s["indices"], s["vertices"], s["draws"], texcoords=texcoords)
        first = host.rt_scene_build(s["meshes"], s["indices"], s["vertices"], SC.moved(s["draws"]), texcoords=texcoords)
        out = host.rt_tlas_build_host(first, s["draws"])
        assert host.rt_scene_validate(out) and out.tobytes() != first.tobytes()
        return out
    plain, tex = blob(opaque, False), blob(textured, True)
    for k in _launches(f):
        rays = f["rays_%d" % k]
        stored = rays[..., 6] != 0
        o, d = rays[..., :3][stored], rays[..., 3:6][stored]
        for q in (0, 1):
            _zero("launch %d, nv_rt_scene_trace_host_rays quality %d" % (k, q), host.rt_scene_trace_host(plain, o, d, q) == f["mask_q%d_%d" % (q, k)][stored])
        got = host.rt_scene_trace_host_textured(tex, o, d, textured["draws"], textured["materials"], tset["descs"], tset["texels"], 1)
        _zero("launch %d, nv_rt_scene_trace_host_textured_rays" % k, got == f["mask_tex_%d" % k][stored])
