"""The attribute pass of the visibility buffer on the MI355X: nv_visibility_attributes after frame(visibility=) and
resolve() against tests/visattr_ref.c — the attribute records and the gbuffer1 words bit for bit, the gbuffer0 words within one code per
channel (pow and log2 are correctly rounded on neither side) — the per-run and the per-pixel form, optional outputs, NV_EINVAL, hand-made
invalid records, a captured graph, and the sharded frame."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import raster_ref as RR
import shade_cases as SC
import visattr_ref as VA
import visbuffer_ref as VB
from niagara_amd import layouts as L
from niagara_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 2
POISON = 0x5A


@pytest.fixture(scope="session")
def vref(tmp_path_factory):
    return VB.load(tmp_path_factory.mktemp("visbuffer_ref_attr_gpu"))


@pytest.fixture(scope="session")
def aref(tmp_path_factory):
    return VA.load(tmp_path_factory.mktemp("visattr_ref_gpu"))


def _scene(name):
    if name == "occluder":
        return VA.with_attributes(synth.occluder_scene(meshlet_bounds=oracle.meshlet_bounds)), 0
    if name == "interior":
        return VA.with_attributes(synth.interior_scene(meshlet_bounds=oracle.meshlet_bounds)), 1
    return VA.with_attributes(VA.kitten_scene(meshlet_bounds=oracle.meshlet_bounds)), 0


def _kw(s, near_clip):
    return dict(task_capacity=4096, cluster_capacity=4096 * 64, fused=True, vertices=s["vertices"], meshlet_data=s["data"], near_clip=bool(near_clip),
                stable_ids=True)


_REFS = {}


def _reference(name, vref, aref):
    if name not in _REFS:
        s, near_clip = _scene(name)
        rec, want = VA.reference_frame(s, near_clip, vref, aref, frames=FRAMES)
        _REFS[name] = (s, near_clip, rec, want)
    return _REFS[name]


def _channels(words, bits):
    out, at = [], 0
    for b in bits:
        out.append((words >> np.uint32(at)) & np.uint32((1 << b) - 1))
        at += b
    return np.stack(out, -1).astype(np.int64)


def _host(out):
    from niagara_amd import pipeline as P
    g = lambda t: None if t is None else t.cpu().numpy().view(np.uint32).reshape(-1).copy()
    return dict(attributes=None if out["attributes"] is None else P.from_device(out["attributes"], L.PIXELATTR).copy(), gbuffer0=g(out["gbuffer0"]),
                gbuffer1=g(out["gbuffer1"]), totals=out["totals"].cpu().numpy().view(np.uint64).copy())


def _same_attributes(got, want, gbuffers=True):
    """the issue's comparison: records and gbuffer1 bit for bit, gbuffer0 within one code per channel and >= 90 % of the channels equal, totals"""
    if got["attributes"].tobytes() != want["attributes"].tobytes():  # say where before failing
        a, b = got["attributes"].view(np.uint32).reshape(-1, 16), want["attributes"].view(np.uint32).reshape(-1, 16)
        bad = np.nonzero((a != b).any(axis=1))[0]
        print("attribute records differ at %d pixels; first:" % len(bad), [(int(i), np.nonzero(a[i] != b[i])[0].tolist()) for i in bad[:12]])
    assert got["totals"].tolist() == want["totals"].tolist()
    assert got["attributes"].tobytes() == want["attributes"].tobytes()
    if gbuffers:
        assert got["gbuffer1"].tobytes() == want["gbuffer1"].tobytes()
        shaded = (want["flags"] & VA.SHADED) != 0
        assert (got["gbuffer0"][~shaded] == 0).all()
        c, r = _channels(got["gbuffer0"][shaded], (8, 8, 8, 8)), _channels(want["gbuffer0"][shaded], (8, 8, 8, 8))
        print("gbuffer0: %d channels, %d differ, largest difference %d" % (c.size, int((c != r).sum()), int(np.abs(c - r).max()) if c.size else 0))
        assert np.abs(c - r).max() <= 1
        assert (c == r).mean() >= 0.9


def _poisoned(pipe, materials=True):
    """the outputs of VisibilityPipeline.attributes as poisoned tensors (the kernel writes every pixel of every output it is given)"""
    import torch
    dev = pipe.ctx.device
    n = pipe.depth_w * pipe.depth_h
    return dict(attributes=torch.full((n * 64,), POISON, dtype=torch.uint8, device=dev),
                gbuffer0=torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=dev) if materials else None,
                gbuffer1=torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=dev) if materials else None,
                totals=torch.zeros(4, dtype=torch.int64, device=dev))


def _run(pipe, s, records, out, materials=True, mat=None):
    """one launch of the entry point into `out`; mat: the material table already on the device (a captured step uploads nothing)"""
    from niagara_amd import pipeline as P
    w, h = s["viewport"]
    if materials and mat is None:
        mat = P.to_device(s["materials"], pipe.ctx.device)
    g = synth.make_globals(s["cull"], (w, h))
    pipe.ctx.visibility_attributes(g, records, w, h, getattr(pipe, "db_all", pipe.db), getattr(pipe, "total_draws", pipe.draw_count), pipe.mlb,
                                   pipe.meshlet_count, pipe.mdb, pipe.mdb.numel() // 4, pipe.vb, pipe.vertex_count, mat,
                                   len(s["materials"]) if materials else 0, out["attributes"], out["gbuffer0"], out["gbuffer1"], out["totals"])
    return mat


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["occluder", "interior", "kitten"])
def test_attributes_after_frame_and_resolve_equal_the_restatement(name, vref, aref):
    from niagara_amd import pipeline as P
    s, near_clip, rec, want = _reference(name, vref, aref)
    pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], **_kw(s, near_clip))
    try:
        vis = pipe.new_visibility()
        for _ in range(FRAMES):
            pipe.frame(s["cull"], post_pass=True, visibility=vis)
        res = pipe.resolve(s["cull"], vis)
        assert P.from_device(res["records"], L.VISRECORD).tobytes() == rec["resolve"]["records"].tobytes()
        out = _poisoned(pipe)
        keep = _run(pipe, s, res["records"], out)
        pipe.ctx.status()
        _same_attributes(_host(out), want)
        # the pipeline's own entry (fresh outputs) gives the same bytes
        again = _host(pipe.attributes(s["cull"], res["records"], s["materials"]))
        pipe.ctx.status()
        got = _host(out)
        assert all(again[k].tobytes() == got[k].tobytes() for k in got)
        del keep
    finally:
        pipe.ctx.close()
    assert want["totals"][0] > 0 and want["totals"][1] == 0 and want["totals"][2] == 0 and want["totals"][3] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("path", SC.FIXTURES, ids=SC.FIXTURE_IDS)
def test_fixture_of_the_reference_fragment_shader_replays(path, aref):
    """tests/golden/shade: records of one scene and the attachments the reference's own mesh.frag.glsl, run on the CPU, writes for them with
    factor-only materials (tests/test_shade_fixtures_cpu.py holds the restatement to them bit for bit).  This file's rule,
    unchanged: records and gbuffer1 bit for bit, gbuffer0 within one code and 90 % of the channels equal."""
    import torch
    from niagara_amd import pipeline as P
    f = np.load(path)
    w, h = SC.fixture_size(f)
    s, rec = SC.fixture_frag_scene(path, f)
    s["materials"] = SC.untextured(s["materials"])
    want = aref.attributes(s["g"], rec, w, h, s["draws"], s["meshlets"], s["data"], s["vertices"], s["materials"])
    want["gbuffer0"], want["gbuffer1"] = f["frag_gbuffer0"], f["frag_gbuffer1"]  # the expectation is the reference's
    ctx = P.Context()
    try:
        dev, n = ctx.device, w * h
        t = [P.to_device(s[k], dev) for k in ("draws", "meshlets", "data", "vertices", "materials")] + [P.to_device(rec, dev)]
        out = dict(attributes=torch.full((n * 64 + 64,), POISON, dtype=torch.uint8, device=dev), gbuffer0=torch.full((n + 16,), 0x5A5A5A5A, dtype=torch.int32, device=dev),
                   gbuffer1=torch.full((n + 16,), 0x5A5A5A5A, dtype=torch.int32, device=dev), totals=torch.zeros(4, dtype=torch.int64, device=dev))
        ctx.visibility_attributes(s["g"], t[5], w, h, t[0], len(s["draws"]), t[1], len(s["meshlets"]), t[2], len(s["data"]), t[3], len(s["vertices"]), t[4],
                                  len(s["materials"]), out["attributes"], out["gbuffer0"], out["gbuffer1"], out["totals"])
        ctx.status()
        assert (out["attributes"][n * 64:].cpu().numpy() == POISON).all() and (out["gbuffer0"][n:].cpu().numpy() == 0x5A5A5A5A).all()
        assert (out["gbuffer1"][n:].cpu().numpy() == 0x5A5A5A5A).all(), "words behind the images were written"
        got = _host(dict(attributes=out["attributes"][:n * 64], gbuffer0=out["gbuffer0"][:n], gbuffer1=out["gbuffer1"][:n], totals=out["totals"]))
        _same_attributes(got, want)
    finally:
        ctx.close()


def _frame_records(pipe, s):
    vis = pipe.new_visibility()
    for _ in range(FRAMES):
        pipe.frame(s["cull"], post_pass=True, visibility=vis)
    return pipe.resolve(s["cull"], vis)["records"]


@pytest.mark.gpu
def test_each_output_is_optional_and_arguments_are_checked(vref, aref):
    import torch
    from niagara_amd import pipeline as P
    from niagara_amd._lib import NvError
    s, near_clip, rec, want = _reference("occluder", vref, aref)
    _, bare = VA.reference_frame(s, near_clip, vref, aref, frames=FRAMES, materials=False)
    pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], **_kw(s, near_clip))
    try:
        records = _frame_records(pipe, s)
        full = _poisoned(pipe)
        mat = _run(pipe, s, records, full)
        pipe.ctx.status()
        full = _host(full)
        for leave in ("attributes", "gbuffer0", "gbuffer1", "totals"):
            out = _poisoned(pipe)
            out[leave] = None
            _run(pipe, s, records, out)
            pipe.ctx.status()
            for k in ("attributes", "gbuffer0", "gbuffer1", "totals"):
                if k != leave:
                    t = out[k].cpu().numpy().reshape(-1)
                    assert t.view(np.uint8).tobytes() == full[k].view(np.uint8).tobytes(), (leave, k)
        # without a material table: the same attribute records, totals word 3 stays 0
        out = _poisoned(pipe, materials=False)
        _run(pipe, s, records, out, materials=False)
        pipe.ctx.status()
        got = _host(out)
        assert got["attributes"].tobytes() == bare["attributes"].tobytes() == want["attributes"].tobytes()
        assert got["totals"].tolist() == bare["totals"].tolist() and got["totals"][3] == 0
        # NV_EINVAL
        c, (w, h) = pipe.ctx, s["viewport"]
        g = synth.make_globals(s["cull"], (w, h))
        n_data = pipe.mdb.numel() // 4
        args = lambda **kw: {**dict(globals_=g, records=records, width=w, height=h, db=pipe.db, draw_count=pipe.draw_count, mlb=pipe.mlb,
                                    meshlet_count=pipe.meshlet_count, meshlet_data=pipe.mdb, data_words=n_data, vertices=pipe.vb,
                                    vertex_count=pipe.vertex_count, materials=mat, material_count=len(s["materials"])), **kw}
        gb = torch.zeros(w * h, dtype=torch.int32, device=c.device)
        attr = torch.zeros(w * h * 64 + 16, dtype=torch.uint8, device=c.device)
        for bad in (dict(records=None), dict(width=0), dict(height=16385), dict(width=w + 1), dict(db=None), dict(mlb=None), dict(meshlet_data=None),
                    dict(vertices=None), dict(materials=None), dict(materials=None, material_count=0, gbuffer0=gb),
                    dict(materials=None, material_count=0, gbuffer1=gb), dict(attributes=attr[4:]), dict(records=records[8:]),
                    dict(globals_=synth.make_globals(s["cull"], (w, h + 1)))):
            with pytest.raises(NvError):
                c.visibility_attributes(**args(**bad))
        c.visibility_attributes(**args())  # no output at all: allowed, writes nothing
        c.status()
        with pytest.raises(NvError):  # the pipeline's entry needs stable ids
            kw = _kw(s, near_clip)
            kw["stable_ids"] = False
            p2 = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], **kw)
            try:
                p2.attributes(s["cull"], records)
            finally:
                p2.ctx.close()
    finally:
        pipe.ctx.close()


def _invalid_records(s, rec):
    """the frame's records with hand-made ones of every invalid class among them, and the capacities that make them invalid"""
    import test_visattr_cpu as TC
    return TC.invalid_cases(s, rec["resolve"]["records"])


@pytest.mark.gpu
def test_hand_made_invalid_records_are_counted_and_written_like_no_sample(vref, aref):
    import torch
    from niagara_amd import pipeline as P
    s, near_clip, rec, _ = _reference("occluder", vref, aref)
    w, h = s["viewport"]
    g = RR.globals_for(s["cull"], (w, h))
    ctx = P.Context()
    try:
        dev = ctx.device
        for records, meshlets, data, counts, expect_invalid in _invalid_records(s, rec):
            want = aref.attributes(g, records, w, h, rec["draws"], meshlets, data, s["vertices"], s["materials"], counts=counts)
            assert want["totals"][1] >= expect_invalid > 0
            cnt = dict(draws=len(rec["draws"]), meshlets=len(meshlets), data=len(data), vertices=len(s["vertices"]), materials=len(s["materials"]))
            cnt.update(counts)
            # exactly-sized device buffers: a load past a capacity would leave the allocation
            t = dict(db=P.to_device(rec["draws"][:max(1, cnt["draws"])], dev), mlb=P.to_device(meshlets[:max(1, cnt["meshlets"])], dev),
                     data=P.to_device(data[:max(1, cnt["data"])], dev), vb=P.to_device(s["vertices"][:max(1, cnt["vertices"])], dev),
                     mat=P.to_device(s["materials"][:max(1, cnt["materials"])], dev))
            out = dict(attributes=torch.full((w * h * 64,), POISON, dtype=torch.uint8, device=dev),
                       gbuffer0=torch.full((w * h,), 0x5A5A5A5A, dtype=torch.int32, device=dev),
                       gbuffer1=torch.full((w * h,), 0x5A5A5A5A, dtype=torch.int32, device=dev), totals=torch.zeros(4, dtype=torch.int64, device=dev))
            ctx.visibility_attributes(g, P.to_device(records, dev), w, h, t["db"], cnt["draws"], t["mlb"], cnt["meshlets"], t["data"], cnt["data"], t["vb"],
                                      cnt["vertices"], t["mat"], cnt["materials"], out["attributes"], out["gbuffer0"], out["gbuffer1"], out["totals"])
            ctx.status()
            _same_attributes(_host(out), want)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_attributes_replay_from_a_captured_graph(vref, aref):
    import torch
    from niagara_amd import pipeline as P
    s, near_clip, rec, want = _reference("occluder", vref, aref)
    pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], **_kw(s, near_clip))
    try:
        dev = pipe.ctx.device
        records = P.to_device(rec["resolve"]["records"], dev)
        out = _poisoned(pipe)
        mat = P.to_device(s["materials"], dev)

        def step():
            out["totals"].zero_()
            _run(pipe, s, records, out, mat=mat)
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            step()
            torch.cuda.synchronize()
            _same_attributes(_host(out), want)
            graph = torch.cuda.CUDAGraph()
            for t in (out["attributes"], out["gbuffer0"], out["gbuffer1"]):
                t.fill_(POISON)
            with torch.cuda.graph(graph, stream=st):
                step()
            torch.cuda.synchronize()
            assert (out["attributes"] == POISON).all()  # nothing ran during capture
            for _ in range(2):
                for t in (out["attributes"], out["gbuffer0"], out["gbuffer1"]):
                    t.fill_(POISON)
                graph.replay()
                torch.cuda.synchronize()
                _same_attributes(_host(out), want)
        pipe.ctx.status()
    finally:
        pipe.ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_local_shards_give_the_unsharded_attributes(world, vref, aref):
    from niagara_amd import pipeline as P
    for name in ("occluder", "interior"):
        s, near_clip, rec, want = _reference(name, vref, aref)
        shards = P.ShardedVisibilityPipeline.local_shards(s["meshes"], s["meshlets"], s["draws"], s["viewport"], world, **_kw(s, near_clip))
        try:
            vis = shards.new_visibility()
            for _ in range(FRAMES):
                shards.frame(s["cull"], post_pass=True, visibility=vis)
            for k, p in enumerate(shards.pipes):
                res = p.resolve(s["cull"], vis[k])
                got = _host(p.attributes(s["cull"], res["records"], s["materials"]))
                shards.status()
                _same_attributes(got, want)
        finally:
            shards.close()


_FORMS = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import oracle, visattr_ref as VA, visbuffer_ref as VB, test_visattr_gpu as T
from niagara_amd import pipeline as P
vref, aref = VB.load(sys.argv[2]), VA.load(sys.argv[2])
for name in ("occluder", "interior"):
    s, near_clip, rec, want = T._reference(name, vref, aref)
    pipe = P.VisibilityPipeline(s["meshes"], s["meshlets"], s["draws"], s["viewport"], **T._kw(s, near_clip))
    out = T._poisoned(pipe)
    keep = T._run(pipe, s, P.to_device(rec["resolve"]["records"], pipe.ctx.device), out)
    pipe.ctx.status()
    got = T._host(out)
    T._same_attributes(got, want)
    np.savez(sys.argv[3] + "_" + name, **got)
    pipe.ctx.close()
print("forms ok")
"""


@pytest.mark.gpu
def test_per_run_and_per_pixel_forms_write_identical_bytes(tmp_path):
    """the experiments build with and without NV_ATTRIBUTES_PER_PIXEL=1, each in a process of its own (the library reads the switch when a
    context is created): both equal the restatement, and each other byte for byte"""
    exp = os.path.join(ROOT, "niagara_amd", "libniagara_vis_exp.so")
    assert os.path.exists(exp)
    script = tmp_path / "forms.py"
    script.write_text(_FORMS)
    for form, value in (("runs", "0"), ("pixel", "1")):
        env = dict(os.environ, NV_LIBRARY_PATH=exp, NV_ATTRIBUTES_PER_PIXEL=value)
        r = subprocess.run([sys.executable, str(script), ROOT, str(tmp_path), str(tmp_path / form)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "forms ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    for name in ("occluder", "interior"):
        a, b = np.load(str(tmp_path / "runs") + "_" + name + ".npz"), np.load(str(tmp_path / "pixel") + "_" + name + ".npz")
        for k in ("attributes", "gbuffer0", "gbuffer1", "totals"):
            assert a[k].tobytes() == b[k].tobytes(), (name, k)
