"""The keyframe animation without a GPU: the layouts and the exported symbols, nv_animate_draws_host (the kernel's text,
niagara_amd/csrc/animmath.h) against the independent restatement tests/animate_ref.c — bit for bit except in slerp's trigonometric branch, which
is held to the counted bound of its fp64 build —, the rule cases, the validator's refusals, the scene-cache reader of the three animation
sections, and tools/animate_check.cpp under the host sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import animate_ref as AR
import niagara_amd as N
import oracle.ref as R
import scenecache_writer as SW
from niagara_amd import host, synth
from niagara_amd import layouts as L
from niagara_amd._lib import NvError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANIMATIONS, DRAWS, LIGHTS = 20000, 30000, 100


@pytest.fixture(scope="module")
def aref(tmp_path_factory):
    return AR.load(tmp_path_factory.mktemp("animate_ref_cpu"))


@pytest.fixture(scope="module")
def fuzz(aref):
    a, k = AR.fuzz_table(ANIMATIONS, DRAWS, seed=21, light_count=LIGHTS)
    which, times = AR.fuzz_times(a)  # 16 times each
    return dict(a=a, k=k, which=which, times=times, r32=aref.eval(a, k, which, times, "f32"), r64=aref.eval(a, k, which, times, "f64"))


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def test_layouts_and_exports():
    assert (L.ANIMATION.itemsize, L.KEYFRAME.itemsize, L.LIGHT.itemsize) == (24, 32, 32)
    assert [L.ANIMATION.fields[n][1] for n in L.ANIMATION.names] == [0, 4, 8, 12, 16, 20]
    assert (L.KEYFRAME.fields["scale"][1], L.KEYFRAME.fields["rotation"][1]) == (12, 16)
    assert (L.LIGHT.fields["range"][1], L.LIGHT.fields["color"][1], L.LIGHT.fields["intensity"][1]) == (12, 16, 28)
    for name in ("nv_scenecache_animations", "nv_animation_validate_host", "nv_animation_phase_host", "nv_animate_draws_host", "nv_upload_animations",
                 "nv_animate_draws"):
        assert name in N.EXPORTS and hasattr(N.lib, name), name


@pytest.mark.skipif(not R.available(), reason="oracle/_ref not built (no reference tree and no prebuilt .so)")
def test_layouts_match_the_reference_structs():
    assert (R.scene_sizeof(19), R.scene_sizeof(20), R.scene_sizeof(18)) == (L.ANIMATION.itemsize, L.KEYFRAME.itemsize, L.LIGHT.itemsize)


def test_the_fuzz_takes_every_path(fuzz):
    """the input condition, on the restatement alone"""
    r = fuzz["r32"]
    live = ~r["skipped"]
    trig = live & ((r["flags"] & AR.TRIG) != 0)
    counts = dict(mix=int((live & ~trig).sum()), trig=int(trig.sum()), negated=int((live & ((r["flags"] & AR.NEGATED) != 0)).sum()),
                  skipped=int(r["skipped"].sum()), wrap=int((live & (r["index1"] == 0) & (r["index0"] > 0)).sum()), instants=int((live & (r["t"] == 0)).sum()))
    print(counts)
    assert min(counts.values()) >= 1000
    assert np.abs(fuzz["k"]["rotation"]).max() <= 1.0  # the bound's input condition
    assert (fuzz["r32"]["flags"] == fuzz["r64"]["flags"]).all() and (fuzz["r32"]["skipped"] == fuzz["r64"]["skipped"]).all()


def test_time_statements_equal_the_restatement_bit_for_bit(fuzz):
    skipped, i0, i1, t = host.animation_phase(fuzz["a"], fuzz["which"], fuzz["times"])
    r = fuzz["r32"]
    assert (skipped == r["skipped"]).all()
    live = ~skipped
    assert (i0[live] == r["index0"][live]).all() and (i1[live] == r["index1"][live]).all()
    assert (_bits(t[live]) == _bits(r["t"][live])).all()
    kc = fuzz["a"]["keyframeCount"][fuzz["which"]]
    assert (i0[live] < kc[live]).all() and (i1[live] == (i0[live] + 1) % kc[live]).all()


def test_host_twin_equals_the_restatement(fuzz):
    """position, scale and the linear branch's orientation bit for bit; the trigonometric branch within AR.TRIG_BOUND of the fp64 build; lights;
    untargeted and skipped draws and words 8-11 of every draw byte for byte"""
    a, k, r32, r64 = fuzz["a"], fuzz["k"], fuzz["r32"], fuzz["r64"]
    rng = np.random.default_rng(5)
    draws0 = rng.integers(0, 256, DRAWS * L.MESHDRAW.itemsize, dtype=np.uint8).view(L.MESHDRAW)
    lights0 = rng.integers(0, 256, LIGHTS * L.LIGHT.itemsize, dtype=np.uint8).view(L.LIGHT)
    targeted = np.zeros(DRAWS, bool)
    targeted[a["drawIndex"]] = True
    n = len(a)
    got = np.zeros((len(fuzz["which"]), 8), np.float32)
    light_got = np.zeros((len(fuzz["which"]), 3), np.float32)
    for j, time in enumerate(AR.TIMES):  # the whole table per time, each from the untouched buffers
        draws, lights = draws0.copy(), lights0.copy()
        host.animate_draws_host(time, a, k, draws, lights)
        rows = slice(j * n, (j + 1) * n)
        d = draws[a["drawIndex"]]
        got[rows, :3], got[rows, 3], got[rows, 4:] = d["position"], d["scale"], d["orientation"]
        light_got[rows][:LIGHTS] = lights[a["lightIndex"][:LIGHTS]]["position"]
        skipped = r32["skipped"][rows]
        assert d[skipped].tobytes() == draws0[a["drawIndex"]][skipped].tobytes()  # a skipped animation leaves its draw alone
        # what no animation names is untouched, words 8-11 of every draw, and a light's range / colour / intensity
        assert draws[~targeted].tobytes() == draws0[~targeted].tobytes()
        w, w0 = draws.view(np.uint32).reshape(DRAWS, 12), draws0.view(np.uint32).reshape(DRAWS, 12)
        assert (w[:, 8:] == w0[:, 8:]).all()
        lw, lw0 = lights.view(np.uint32).reshape(LIGHTS, 8), lights0.view(np.uint32).reshape(LIGHTS, 8)
        assert (lw[:, 3:] == lw0[:, 3:]).all()
    which = fuzz["which"]
    live = ~r32["skipped"]
    trig = live & ((r32["flags"] & AR.TRIG) != 0)
    lin = live & ~trig
    want32 = r32["out"].astype(np.float32)
    assert (_bits(got[live, :4]) == _bits(want32[live, :4])).all()
    assert (_bits(got[lin, 4:]) == _bits(want32[lin, 4:])).all()
    err = np.abs(got[trig, 4:].astype(np.float64) - r64["out"][trig, 4:])
    print("trigonometric branch: %d samples, largest |host twin - fp64| = %.3g (%.2f x 2^-23), bound %.3g; %d of %d components equal the fp32 restatement's bits"
          % (int(trig.sum()), err.max(), err.max() * 2 ** 23, AR.TRIG_BOUND, int((_bits(got[trig, 4:]) == _bits(want32[trig, 4:])).sum()), err.size))
    assert err.max() <= AR.TRIG_BOUND
    lit = live & (a["lightIndex"][which] >= 0)
    assert lit.sum() >= 1000 and (_bits(light_got[lit]) == _bits(want32[lit, :3])).all()


def test_whole_table_at_one_time_equals_the_reference_loop(aref):
    """the table in one call (what the kernel runs) against the restatement's loop in array order, linear-branch keyframes: byte for byte"""
    draws = host.synth_draws(500, 4, 40.0)
    a, k = synth.orbit_animations(draws, np.arange(0, 500, 3), 2, seed=4)
    k["rotation"][1::2] = k["rotation"][0::2]  # both keyframes of a pair share the rotation: slerp's linear branch
    for time in (-1.0, 0.0, 0.3, 1.7, 1e9):
        want, _ = aref.apply(time, a, k, draws)
        got = draws.copy()
        host.animate_draws_host(time, a, k, got)
        assert got.tobytes() == want.tobytes()
        if time > 1.0:
            assert got.tobytes() != draws.tobytes()


def test_rule_cases(aref):
    draws = host.synth_draws(4, 2, 10.0)
    lights = np.zeros(2, L.LIGHT)
    lights["range"], lights["intensity"], lights["color"] = 7.0, 3.0, (0.25, 0.5, 1.0)
    k = np.zeros(3, L.KEYFRAME)
    k["translation"] = [[1, 2, 3], [4, 5, 6], [-7, 8, -9]]
    k["scale"] = [0.5, 2.0, 3.0]
    k["rotation"] = [0.0, 0.0, 0.0, 1.0]
    a = np.zeros(3, L.ANIMATION)
    a["period"] = 1.0
    a["drawIndex"], a["lightIndex"], a["keyframeOffset"], a["keyframeCount"] = [1, 3, -1], [-1, 0, -1], [2, 0, 0], [1, 3, 2]
    assert host.animation_validate(a, 3, 4, 2) == ("ok", 0)
    for time in (0.0, 0.25, 1.5, 2.75, 17.125):
        got_d, got_l = draws.copy(), lights.copy()
        host.animate_draws_host(time, a, k, got_d, got_l)
        want_d, want_l = aref.apply(time, a, k, draws, lights)
        assert got_d.tobytes() == want_d.tobytes() and got_l.tobytes() == want_l.tobytes()
        # keyframeCount == 1: both indices 0, the draw sits on its only keyframe (mix(x, x, t) is x up to its roundings)
        assert np.allclose(got_d["position"][1], k["translation"][2], rtol=1e-6) and np.isclose(got_d["scale"][1], 3.0, rtol=1e-6)
        # a draw and a light: the light's position is the draw's, its other fields stay
        assert got_l["position"][0].tobytes() == got_d["position"][3].tobytes()
        assert all(got_l[f].tobytes() == lights[f].tobytes() for f in ("range", "color", "intensity"))
        # neither target, and the draws nobody names
        assert got_d[[0, 2]].tobytes() == draws[[0, 2]].tobytes() and got_l[1].tobytes() == lights[1].tobytes()
    # NULL arrays skip their targets; the indices are still validated
    only_l = lights.copy()
    host.animate_draws_host(0.25, a, k, None, only_l, draw_count=4)
    assert only_l.tobytes() == aref.apply(0.25, a, k, None, lights)[1].tobytes()
    with pytest.raises(NvError):
        host.animate_draws_host(0.25, a, k, None, only_l, draw_count=3)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(NvError):
            host.animate_draws_host(bad, a, k, draws.copy(), lights.copy())


def _table():
    a = np.zeros(4, L.ANIMATION)
    a["drawIndex"], a["lightIndex"], a["period"], a["keyframeOffset"], a["keyframeCount"] = [0, 1, 2, -1], [-1, 0, -1, 1], 1.0, [0, 2, 4, 6], 2
    return a


@pytest.mark.parametrize("reason,index,edit", [
    ("no_keyframes", 2, lambda a: a["keyframeCount"].__setitem__(2, 0)),
    ("keyframe_range", 3, lambda a: a["keyframeCount"].__setitem__(3, 3)),
    ("keyframe_range", 1, lambda a: a["keyframeOffset"].__setitem__(1, 0xFFFFFFFF)),
    ("period", 0, lambda a: a["period"].__setitem__(0, 0.0)),
    ("period", 1, lambda a: a["period"].__setitem__(1, -2.0)),
    ("period", 2, lambda a: a["period"].__setitem__(2, np.inf)),
    ("period", 3, lambda a: a["period"].__setitem__(3, np.nan)),
    ("period", 1, lambda a: a["startTime"].__setitem__(1, np.nan)),
    ("draw_index", 2, lambda a: a["drawIndex"].__setitem__(2, 3)),
    ("light_index", 3, lambda a: a["lightIndex"].__setitem__(3, 2)),
    ("duplicate_draw", 2, lambda a: a["drawIndex"].__setitem__(2, 0)),
    ("duplicate_light", 3, lambda a: a["lightIndex"].__setitem__(3, 0)),
])
def test_the_validator_names_each_refusal(reason, index, edit):
    a = _table()
    assert host.animation_validate(a, 8, 3, 2) == ("ok", 0)
    edit(a)
    assert host.animation_validate(a, 8, 3, 2) == (reason, index)
    draws, lights = host.synth_draws(3, 1, 5.0), np.zeros(2, L.LIGHT)
    before = draws.tobytes()
    with pytest.raises(NvError):
        host.animate_draws_host(0.5, a, np.zeros(8, L.KEYFRAME), draws, lights)
    assert draws.tobytes() == before  # a refused table rewrites nothing


def _records(seed, lights, animations, keyframes):
    rng = np.random.default_rng(seed)
    return tuple(rng.integers(0, 256, n * dt.itemsize, dtype=np.uint8).view(dt) for n, dt in ((lights, L.LIGHT), (animations, L.ANIMATION), (keyframes, L.KEYFRAME)))


@pytest.mark.parametrize("compressed", [False, True])
def test_reader_returns_the_three_sections(compressed, tmp_path):
    meshes, total = synth.make_meshes(3, 2, 10)
    meshlets, draws = synth.make_meshlets(total), host.synth_draws(7, 3, 10.0)
    path = str(tmp_path / "scene.cache")
    counts = dict(vertex_count=100, index_count=300, meshletdata_count=500, meshletvtx0_count=64, material_count=3)
    sizes = SW.write_scene_cache(path, meshes, meshlets, draws, compressed=compressed, light_count=5, animation_count=9, keyframe_count=31, **counts)
    lights, anims, keys = _records(8, 5, 9, 31)
    # the offset, computed here from the section sizes (src/scenecache.cpp:163-186)
    at = 160 + sizes["v"] + sizes["i"] + meshlets.nbytes + sizes["md"] + sizes["v0"] + meshes.nbytes + 3 * 64 + draws.nbytes
    with open(path, "r+b") as f:
        f.seek(at)
        f.write(lights.tobytes() + anims.tobytes() + keys.tobytes())
    gl, ga, gk = host.scenecache_animations(path)
    assert gl.tobytes() == lights.tobytes() and ga.tobytes() == anims.tobytes() and gk.tobytes() == keys.tobytes()
    assert host.scenecache_read(path)[3].tobytes() == draws.tobytes()  # the neighbours are where they were
    # truncated inside the keyframes, inside the lights, and right behind the draws
    data = open(path, "rb").read()
    for cut in (at + lights.nbytes + anims.nbytes + keys.nbytes - 1, at + 10, at):
        short = str(tmp_path / ("short%d.cache" % cut))
        open(short, "wb").write(data[:cut])
        with pytest.raises(NvError, match="NV_EFORMAT"):
            host.scenecache_animations(short)
    whole = str(tmp_path / "whole.cache")  # nothing behind the keyframes: still readable
    open(whole, "wb").write(data[:at + lights.nbytes + anims.nbytes + keys.nbytes])
    assert host.scenecache_animations(whole)[2].tobytes() == keys.tobytes()


@pytest.mark.skipif(not R.available(), reason="oracle/_ref not built (no reference tree and no prebuilt .so)")
def test_reader_on_a_file_the_reference_saved(tmp_path):
    meshes, total = synth.make_meshes(3, 2, 10)
    meshlets, draws = synth.make_meshlets(total), host.synth_draws(7, 3, 10.0)
    path = str(tmp_path / "ref.cache")
    R.save_scene_cache(path, meshes, meshlets, draws, light_count=4, animation_count=6, keyframe_count=20, texture_paths=2)
    info = host.scenecache_info(path)
    assert (info.lightCount, info.animationCount, info.keyframeCount) == (4, 6, 20)
    lights, anims, keys = host.scenecache_animations(path)
    assert (len(lights), len(anims), len(keys)) == (4, 6, 20)
    assert not lights.view(np.uint8).any() and not anims.view(np.uint8).any() and not keys.view(np.uint8).any()  # value-initialised vectors
    end = info.drawOffset + info.drawCount * 48 + 4 * 32 + 6 * 24 + 20 * 32
    assert end + info.texturePathCount * 256 == info.fileSize


def test_the_standalone_program_runs_clean_under_the_host_sanitizers(tmp_path):
    """tools/animate_check.cpp with host.cpp, host code only, its own main: AddressSanitizer and UBSan linked statically into the program itself"""
    exe = tmp_path / "animate_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "animate_check.cpp"),
                           os.path.join(ROOT, "niagara_amd", "csrc", "host.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe), str(tmp_path / "animate_check.cache")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    print(out.stdout.decode())
    assert out.returncode == 0 and b"animate_check: ok" in out.stdout
