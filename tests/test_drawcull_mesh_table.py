"""drawcull over Mesh-table sizes and registration states.

The decide launch is draw_decide_kernel<LATE, TASK, MESH_LDS, SOA, VISFIRST, RECORDS>.  The rest of the suite moves MESH_LDS (the Mesh table
staged in LDS: registered by nv_upload_meshes, at most DC_MESH_LDS = 64 meshes) and SOA (the draw mirror of nv_upload_draws) only together and
with at most 8 meshes.  Here every combination of the two is launched, with tables of 1, 63, 64 (the exact fit of the staging loops), 65 and
200 meshes whose last entries are looked up as often as their first, and the host-side rules that choose the form (context.hip, nv_drawcull)
are pinned one by one.

The reference is always the CPU oracle, fed with exactly the table and the draws the pass is given.  Compared bytewise: the count word, the
first `count` commands, every drawVisibility word.  No tolerances.
"""
import functools

import numpy as np
import pytest
import torch

import oracle
from niagara_amd import host
from niagara_amd import layouts as L
from niagara_amd import pipeline as P

import gpu_passes as G
import passes
from scenes import mesh_table_scene, task_capacity

MESH_COUNTS = (1, 63, 64, 65, 200)
# what is registered, in which order                                            -> the form a pass takes
STATES = ("none",         # nothing                                                gather + records in place
          "meshes",       # the Mesh table; the draws not                          LDS for N <= 64 + records in place
          "draws",        # the draws, against a table that is not registered      gather + mirror
          "both",         # meshes, then draws (the order of INTEGRATION.md)       LDS or gather by N, + mirror
          "draws_first")  # draws, then meshes                                     as `both`; draw_split_kernel ran with meshCount = 0
FLAG_SETS = ((0, 1, 0, 0, 1), (1, 1, 1, 1, 1))
FRACTIONS = (1.0, 0.03)  # of the draws visible last frame
# (late, task, NV_OPT_DRAW_RECORDS, NV_OPT_TASK_EMIT): those of test_gpu_parity.py test_drawcull_ring_and_queue_shapes
FORMS = ((0, 0, 1, 0), (0, 1, 2, 1), (0, 1, 1, 2), (0, 0, 2, 0), (1, 1, 0, 2), (1, 1, 0, 1), (1, 0, 0, 0))
ALL_ON = (1, 1, 1, 1, 1)


@pytest.fixture(scope="module")
def ctx():
    c = P.Context()
    yield c
    c.close()


def oracle_pass(meshes, draws, cd, late, task, dvb0, pyr, post=0):
    """(count, the first `count` commands, drawVisibility after the pass) of the oracle over exactly this table and these draws"""
    cd = cd.copy()
    cd["drawCount"] = len(draws)
    dvb = dvb0.copy()
    cmds, c4 = passes.run_drawcull(oracle, dict(meshes=meshes, draws=draws), cd, late, task, dvb, pyr, post)
    n = int(c4[0])
    out = (n, cmds[:n].copy(), dvb)
    for a in out[1:]:
        a.flags.writeable = False
    return out


def varied_table(meshes):
    """The same table with a radius and LOD errors that differ from mesh to mesh.  The synthetic meshes share both, so a decision taken from
    another mesh's entry chooses the same LOD and shows only where the entry's meshlet range is copied (the RECORDS form); with this table it
    shows in the visibility words and the LOD of every form."""
    m = meshes.copy()
    i = np.arange(len(m))
    m["radius"] *= (0.5 + (i * 7 % 13) / 8.0).astype(np.float32)                  # x 0.5 .. 2.0, neighbours far apart
    m["lods"]["error"] *= (0.4 + (i * 5 % 11) / 4.0).astype(np.float32)[:, None]  # x 0.4 .. 2.9
    return m


TABLES = ("uniform", "varied")  # scenes.mesh_table_scene as it is; with varied_table()


class Case:
    """one scene per mesh count and table with its pyramid and the oracle's result of every pass of the matrix, computed once for all
    registration states"""

    def __init__(self, n_meshes, table="uniform"):
        self.scene = mesh_table_scene(n_meshes)
        if table == "varied":
            self.scene = dict(self.scene, meshes=varied_table(self.scene["meshes"]))
        self.n = len(self.scene["draws"])
        self.pyr = oracle.Pyramid(*self.scene["viewport"])
        oracle.depthreduce(self.scene["depth"], self.pyr)
        self.cap = task_capacity(self.scene)
        rng = np.random.default_rng(1000 + n_meshes)
        self.dvb0 = {f: (rng.random(self.n) < f).astype(np.uint32) for f in FRACTIONS}
        self._ref = {}

    def ref(self, flags, fraction, late, task, post):
        key = (flags, fraction, late, task, post)
        if key not in self._ref:
            cd = passes.set_flags(self.scene["cull"], flags)
            self._ref[key] = oracle_pass(self.scene["meshes"], self.scene["draws"], cd, late, task, self.dvb0[fraction], self.pyr, post)
        return self._ref[key]


@functools.lru_cache(maxsize=None)
def case(n_meshes, table="uniform"):
    return Case(n_meshes, table)


@functools.lru_cache(maxsize=None)
def oracle_frames(n_meshes, table):
    return passes.run_frames(oracle, case(n_meshes, table).scene, ALL_ON, frames=2)


class Device:
    """device copies of a table and of draws, registered piece by piece (gpu_passes.GpuScene ties the registrations together)"""

    def __init__(self, ctx, scene):
        self.ctx = ctx
        dev = ctx.device
        self.mb = P.to_device(scene["meshes"], dev)
        self.db = P.to_device(scene["draws"], dev)
        self.n_meshes, self.n_draws = len(scene["meshes"]), len(scene["draws"])
        vw, vh = scene["viewport"]
        self.pyramid = P.DepthPyramid(dev, vw, vh)
        depth = torch.from_numpy(np.ascontiguousarray(scene["depth"])).to(dev)
        ctx.depthreduce(depth, vw, vh, self.pyramid.desc)

    def register(self, state):
        c = self.ctx
        drop(c)
        if state in ("meshes", "both"):
            c.upload_meshes(self.mb, self.n_meshes)
        if state in ("draws", "both", "draws_first"):
            c.upload_draws(self.db, self.n_draws, self.mb)
        if state == "draws_first":
            c.upload_meshes(self.mb, self.n_meshes)

    def run(self, cd, late, task, dvb0, cap, post=0, db=None, mb=None, ctx=None):
        """one pass over len(dvb0) draws starting at `db`: (count, the commands up to the buffer's capacity, drawVisibility)"""
        ctx = ctx or self.ctx
        dev = ctx.device
        dt = L.TASKCMD if task else L.DRAWCMD
        dcb = torch.zeros(cap * dt.itemsize, dtype=torch.uint8, device=dev)
        dccb = torch.zeros(4, dtype=torch.int32, device=dev)
        dvb = torch.from_numpy(dvb0.view(np.int32).copy()).to(dev)
        pd = cd.copy()
        pd["drawCount"] = len(dvb0)
        pd["clusterBackfaceEnabled"] = 1 if post == 0 else 0
        pd["postPass"] = post
        ctx.drawcull(pd, late, task, self.db if db is None else db, self.mb if mb is None else mb, dcb, dccb, dvb, self.pyramid.desc)
        return int(G.host_u32(dccb)[0]), P.from_device(dcb, dt), G.host_u32(dvb)


def drop(ctx):
    ctx.upload_meshes(None, 0)
    ctx.upload_draws(None, 0)
    ctx.upload_meshlets(None, 0)


def difference(got, want, draws):
    """None if the pass equals the oracle's; otherwise a message naming the first draws that differ and their meshIndex"""
    (n_g, cmds_g, dvb_g), (n_o, cmds_o, dvb_o) = got, want
    k = min(n_g, n_o, len(cmds_g))
    bad_cmd = np.nonzero(cmds_g[:k] != cmds_o[:k])[0]
    bad_vis = np.nonzero(dvb_g != dvb_o)[0]
    if n_g == n_o and not len(bad_cmd) and not len(bad_vis):
        return None
    ids = [int(d) for d in cmds_o["drawId"][bad_cmd[:6]]]
    msg = "count %d, oracle %d; %d commands differ, the first at %s: draws %s (meshIndex %s), got %s; %d visibility words differ: draws %s (meshIndex %s)" % (
        n_g, n_o, len(bad_cmd), bad_cmd[:6].tolist(), ids, draws["meshIndex"][ids].tolist(), cmds_g[bad_cmd[:3]].tolist(),
        len(bad_vis), bad_vis[:6].tolist(), draws["meshIndex"][bad_vis[:6]].tolist())
    return msg


def lod_of(meshes, draws, cmds):
    """LOD index implied by each task command's taskOffset: the LOD ranges of a mesh lie back to back in ascending order"""
    offs = meshes["lods"]["meshletOffset"][draws["meshIndex"][cmds["drawId"]]].astype(np.int64)
    return (cmds["taskOffset"].astype(np.int64)[:, None] >= offs).sum(axis=1) - 1


# ---------------------------------------------------------------- coverage conditions (CPU: the oracle alone)

@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("n_meshes", MESH_COUNTS)
def test_scene_reaches_the_whole_table_and_every_branch(n_meshes, table):
    """Conditions, not measurements, so that a green GPU run is not vacuous (scenes.MESH_TABLE_SEED = 418): the passes of the matrix below
    look up the first and the last entry of the table and those on both sides of DC_MESH_LDS, nearly every mesh emits, several LODs are
    chosen, and the late pass both emits and rejects by occlusion."""
    c = case(n_meshes, table)
    meshes, draws = c.scene["meshes"], c.scene["draws"]
    n, cmds, _ = c.ref(FLAG_SETS[0], 1.0, 0, 1, 0)
    emitting = set(draws["meshIndex"][cmds["drawId"]].tolist())
    assert 0 in emitting and n_meshes - 1 in emitting
    assert n_meshes < 64 or 63 in emitting
    assert n_meshes < 65 or 64 in emitting
    assert len(emitting) >= 0.9 * n_meshes
    assert int(meshes["lodCount"].min()) == 8  # all 28 words of a mesh's decision record are in use
    assert cmds["taskCount"].max() == 64 and len(cmds) > len(np.unique(cmds["drawId"]))  # draws of several task groups
    n, cmds, _ = c.ref(ALL_ON, 1.0, 0, 1, 0)
    assert len(np.unique(lod_of(meshes, draws, cmds))) >= 3
    for fraction in FRACTIONS:
        n, cmds, dvb = c.ref(ALL_ON, fraction, 1, 1, 0)
        assert n > 0 and len(np.unique(cmds["drawId"])) >= 1
        assert len(np.unique(lod_of(meshes, draws, cmds))) >= 3
        # inside the frustum (visible with occlusion off) and rejected by the pyramid
        cd = passes.set_flags(c.scene["cull"], (1, 1, 0, 1, 1))
        _, _, in_frustum = oracle_pass(meshes, draws, cd, 1, 1, c.dvb0[fraction], c.pyr)
        part = draws["postPass"] == 0
        assert int(((in_frustum == 1) & (dvb == 0) & part).sum()) >= 1
    # the early pass with few draws visible last frame still emits, and the post pass has draws of its own
    assert c.ref(ALL_ON, 0.03, 0, 1, 0)[0] > 0 and c.ref(ALL_ON, 1.0, 1, 1, 1)[0] > 0


# ---------------------------------------------------------------- 1. the matrix

@pytest.mark.gpu
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("n_meshes", MESH_COUNTS)
def test_mesh_counts_by_registration_states(ctx, n_meshes, state):
    """Every (MESH_LDS, SOA) form of the decide launch and every MESH_LDS form of the scatter launch: flags, last-frame visibility and
    (late, task, records, emit) as in test_drawcull_ring_and_queue_shapes, main and post pass; the scene's table and the varied one."""
    try:
        for table in TABLES:
            c = case(n_meshes, table)
            draws = c.scene["draws"]
            d = Device(ctx, c.scene)
            assert d.pyramid.data.cpu().numpy().tobytes() == c.pyr.data.tobytes()
            d.register(state)
            for flags in FLAG_SETS:
                cd = passes.set_flags(c.scene["cull"], flags)
                for fraction in FRACTIONS:
                    for late, task, records, emit in FORMS:
                        ctx.set_option(P.NV_OPT_DRAW_RECORDS, records)
                        ctx.set_option(P.NV_OPT_TASK_EMIT, emit)
                        for post in (0, 1):
                            got = d.run(cd, late, task, c.dvb0[fraction], c.cap if task else c.n + 1, post)
                            diff = difference(got, c.ref(flags, fraction, late, task, post), draws)
                            assert diff is None, ((n_meshes, table, state, flags, fraction, late, task, records, emit, post), diff)
            ctx.status()
    finally:
        ctx.set_option(P.NV_OPT_DRAW_RECORDS, 0)
        ctx.set_option(P.NV_OPT_TASK_EMIT, 0)
        drop(ctx)


# ---------------------------------------------------------------- 3. the rules that choose the form

def early_and_late(c):
    """(late, last-frame visibility) of the two passes the rule tests run, task form, all flags on"""
    return ((0, c.dvb0[1.0]), (1, c.dvb0[0.03]))


@pytest.mark.gpu
@pytest.mark.parametrize("n_meshes", [65, 8])
def test_the_mirror_serves_only_the_table_it_was_built_from(ctx, n_meshes):
    """A pass over table B while table A and a mirror built from A are registered reads B and the records in place; over A again, the
    mirror.  B = A with every radius and LOD error scaled by 1.7: commands from the wrong bounds would be plausible, and the oracle's
    on A."""
    c = case(n_meshes)
    scene, draws = c.scene, c.scene["draws"]
    a = scene["meshes"]
    b = a.copy()
    b["radius"] *= np.float32(1.7)
    b["lods"]["error"] *= np.float32(1.7)
    cd = passes.set_flags(scene["cull"], ALL_ON)
    try:
        d = Device(ctx, scene)
        mb_b = P.to_device(b, ctx.device)
        for registered_table in ("A", "B"):
            # "A": table and mirror of A.  "B": the mirror of A beside a registered table B, so that the pass over B stages B in LDS
            # (8 meshes) and the pass over A gathers A beside its mirror.
            drop(ctx)
            ctx.upload_meshes(d.mb if registered_table == "A" else mb_b, n_meshes)
            ctx.upload_draws(d.db, c.n, d.mb)
            for late, dvb0 in early_and_late(c):
                want_a = oracle_pass(a, draws, cd, late, 1, dvb0, c.pyr)
                want_b = oracle_pass(b, draws, cd, late, 1, dvb0, c.pyr)
                assert difference(want_b, want_a, draws) is not None  # the two tables are told apart by this pass
                for table, mb, want, other in (("B", mb_b, want_b, want_a), ("A", d.mb, want_a, want_b)):
                    got = d.run(cd, late, 1, dvb0, c.cap, mb=mb)
                    diff = difference(got, want, draws)
                    assert diff is None, ((n_meshes, registered_table, late, table), diff)
                    assert difference(got, other, draws) is not None, (n_meshes, registered_table, late, table)
        ctx.status()
    finally:
        drop(ctx)


@pytest.mark.gpu
def test_table_grows_past_the_lds_limit_and_shrinks_again(ctx):
    """64, 65, 64 meshes registered on one context (prefixes of one allocation): the form changes on the live context, the 64-mesh
    table fills the LDS staging loops exactly, and nv_profile_variants counts the task form of every pass."""
    c = case(65)
    scene, meshes = c.scene, c.scene["meshes"]
    draws65 = scene["draws"]
    draws64 = draws65.copy()
    draws64["meshIndex"][draws64["meshIndex"] == 64] = 63
    assert (draws65["meshIndex"] == 64).any() and (draws64["meshIndex"] == 63).sum() > (draws65["meshIndex"] == 63).sum()
    cd = passes.set_flags(scene["cull"], ALL_ON)
    try:
        d = Device(ctx, scene)
        ctx.profile_variants()
        for count, draws in ((64, draws64), (65, draws65), (64, draws64)):
            d.db.copy_(P.to_device(draws, ctx.device))
            ctx.upload_meshes(d.mb, count)
            ctx.upload_draws(d.db, c.n, d.mb)
            cap = task_capacity(dict(meshes=meshes, draws=draws))
            for (late, dvb0), emit in zip(early_and_late(c), (1, 2)):
                ctx.set_option(P.NV_OPT_TASK_EMIT, emit)
                got = d.run(cd, late, 1, dvb0, cap)
                diff = difference(got, oracle_pass(meshes[:count], draws, cd, late, 1, dvb0, c.pyr), draws)
                assert diff is None, ((count, late, emit), diff)
            got = d.run(cd, 1, 0, c.dvb0[0.03], c.n + 1)  # (no task form: not counted)
            diff = difference(got, oracle_pass(meshes[:count], draws, cd, 1, 0, c.dvb0[0.03], c.pyr), draws)
            assert diff is None, ((count, "draw commands"), diff)
            assert ctx.profile_variants() == {"task_per_draw": 1, "task_list": 1}, count
        ctx.status()
    finally:
        ctx.set_option(P.NV_OPT_TASK_EMIT, 0)
        drop(ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("table", TABLES)
def test_sub_range_of_the_mirror_with_a_gathered_table(ctx, table):
    """d_draws at record 1000 of the registered buffer, 2049 draws, 65 meshes: the mirror's streams are offset, the table is not"""
    c = case(65, table)
    scene = c.scene
    first, count = 1000, 2049
    sub = scene["draws"][first:first + count]
    cd = passes.set_flags(scene["cull"], ALL_ON)
    cap = task_capacity(dict(meshes=scene["meshes"], draws=sub))
    try:
        d = Device(ctx, scene)
        d.register("both")
        for late, dvb0 in early_and_late(c):
            for task in (1, 0):
                dv = dvb0[first:first + count]
                want = oracle_pass(scene["meshes"], sub, cd, late, task, dv, c.pyr)
                assert want[0] > 0
                got = d.run(cd, late, task, dv, cap if task else count + 1, db=d.db[first * L.MESHDRAW.itemsize:])
                diff = difference(got, want, sub)
                assert diff is None, ((late, task), diff)
        ctx.status()
    finally:
        drop(ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("table", TABLES)
def test_update_draws_moves_draws_across_the_lds_limit(ctx, table):
    """the animation case of test_draw_mirror_update_and_sub_ranges with 65 meshes: 200 records rewritten, meshIndex included — some
    move to mesh 64, some from it — and re-transposed by nv_update_draws"""
    c = case(65, table)
    scene, meshes = c.scene, c.scene["meshes"]
    draws = scene["draws"].copy()
    rng = np.random.default_rng(65)
    at64 = np.nonzero(draws["meshIndex"] == 64)[0]
    ranges = ((17, 1), (int(at64[len(at64) // 2]), 150), (c.n - 49, 49))
    assert sum(k for _, k in ranges) == 200
    old = draws["meshIndex"].copy()
    for first, k in ranges:
        draws["position"][first:first + k] = rng.uniform(-5, 5, (k, 3)).astype(np.float32)
        draws["scale"][first:first + k] = rng.uniform(0.5, 3, k).astype(np.float32)
        q = rng.normal(size=(k, 4)).astype(np.float32)
        draws["orientation"][first:first + k] = q / np.linalg.norm(q, axis=1, keepdims=True)
        draws["meshIndex"][first:first + k] = rng.integers(0, 64, k)
    draws["meshIndex"][17] = 64
    draws["meshIndex"][ranges[1][0] + 1:ranges[1][0] + 150:7] = 64
    assert ((old != 64) & (draws["meshIndex"] == 64)).sum() > 1 and ((old == 64) & (draws["meshIndex"] != 64)).sum() >= 1
    cd = passes.set_flags(scene["cull"], ALL_ON)
    cap = task_capacity(dict(meshes=meshes, draws=draws))
    try:
        d = Device(ctx, scene)
        d.register("both")
        for first, k in ranges:
            s = L.MESHDRAW.itemsize
            d.db[first * s:(first + k) * s].copy_(P.to_device(draws[first:first + k], ctx.device))
            ctx.update_draws(d.db, first, k)
        moved = np.nonzero(old != draws["meshIndex"])[0]
        for late, dvb0 in early_and_late(c):
            for task in (1, 0):
                want = oracle_pass(meshes, draws, cd, late, task, dvb0, c.pyr)
                stale = oracle_pass(meshes, scene["draws"], cd, late, task, dvb0, c.pyr)
                assert difference(stale, want, draws) is not None  # the rewritten records change this pass
                got = d.run(cd, late, task, dvb0, cap if task else c.n + 1)
                diff = difference(got, want, draws)
                assert diff is None, ((late, task), diff)
                if task and not late:
                    assert np.isin(moved, want[1]["drawId"]).any()  # a draw whose mesh changed emits
        ctx.status()
    finally:
        drop(ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("table", TABLES)
def test_second_context_culls_a_shared_65_mesh_scene(ctx, table):
    """nv_share_scene: the table and the mirror registered through one context serve another context's pass over its own view"""
    c = case(65, table)
    scene, draws = c.scene, c.scene["draws"]
    pw, ph = host.previous_pow2(scene["viewport"][0]), host.previous_pow2(scene["viewport"][1])
    view = host.build_cull_data((2.0, -1.0, 1.5), (0.5, -0.5, 0.5, 0.5), draw_distance=60.0, viewport=scene["viewport"], pyramid=(pw, ph),
                                draw_count=c.n, cullingEnabled=1, lodEnabled=1)
    view = passes.set_flags(view, ALL_ON)
    own = passes.set_flags(scene["cull"], ALL_ON)
    other = P.Context()
    try:
        d = Device(ctx, scene)
        other.share_scene(ctx)
        d.register("both")  # registered through `ctx` after the scenes were joined
        for late, dvb0 in early_and_late(c):
            want = oracle_pass(scene["meshes"], draws, view, late, 1, dvb0, c.pyr)
            assert want[0] > 0 and difference(want, oracle_pass(scene["meshes"], draws, own, late, 1, dvb0, c.pyr), draws) is not None
            got = d.run(view, late, 1, dvb0, c.cap, ctx=other)
            diff = difference(got, want, draws)
            assert diff is None, (late, diff)
        other.status()
    finally:
        other.close()
        drop(ctx)


# ---------------------------------------------------------------- 4. whole frames

@pytest.mark.gpu
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("n_meshes", [65, 200])
def test_two_frames_with_a_gathered_table(ctx, n_meshes, fused, table):
    """early -> pyramid -> late (-> post) over two frames with a table too large for LDS and the mirror: the late pass's drawVisibility
    carried from frame to frame through the forms no other test launches"""
    scene = case(n_meshes, table).scene
    want = oracle_frames(n_meshes, table)
    try:
        got = G.run_frames(ctx, scene, ALL_ON, frames=2, use_soa=True, fused=fused)
    finally:
        drop(ctx)
    assert want[1]["early"]["count4"][0] > 0 and want[1]["late"]["count4"][0] > 0 and "post" in want[0]
    for f, (w, g) in enumerate(zip(want, got)):
        assert w["pyramid"].tobytes() == g["pyramid"].tobytes()
        for phase in ("early", "late", "post"):
            for key in ("count4", "cc4", "cib", "dvb", "mvb", "commands"):
                assert w[phase][key].tobytes() == g[phase][key].tobytes(), (f, phase, key)
