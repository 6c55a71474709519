"""The degenerate rays on the DEVICE kernels of the shadow trace.  rtmath.h and rtalpha.h are compiled
twice, by g++ for the host twins and by hipcc for shadow_trace_kernel<QUERY, ARGS>; the statements most likely to part ways between the two
compilations — the fp64 re-evaluation of U, V, W, the slab test with a zero direction component, fminf / fmaxf dropping a NaN, denormal
intermediates of T, non-finite rays, the infinite TLAS box, margins that overflow — are reached only by rays the generic suites never
make.  shadow_ref.affine_launch's hand-made inverseViewProjection turns a 16 x 16 launch of the real entry points into a chosen lattice of
such rays (tests/test_shadowtrace_cpu.py holds the construction exact), and every mask is compared byte for byte with the brute-force
restatement on the same ShadowData and depth bytes: no tolerance, no launch left out.  EXPERIMENTS.md records which of these tests fail
on a device build that flushes denormals or runs T's fp64 branch in fp32 (the older GPU suites pass on both).

Masks start as 0x5A bytes and each is followed by 64 bytes that must keep that byte.  The depth images and masks of a list of launches are
allocated once (Batch) and the restatement's masks are computed once per (scene, quality) and shared by the tests."""
import time

import numpy as np
import pytest

import shadow_alpha_ref as SA
import shadow_ref as SH
import test_shade_gpu as TS
import test_shadow_alpha_gpu as AG
import test_shadowtrace_gpu as TG
import test_texture_blocks_gpu as TB
import test_tlas_build_gpu as TT
import tlas_ref as TR
from niagara_amd import host

N = SH.LATTICE_N
TEXELS = N * N
STRIDE = TEXELS + TS.TAIL  # a mask and the tail behind it
POISON = TG.POISON
assert POISON == SH.POISON == TS.POISON
TOTALS = dict(launches=0, rays=0, differences=0)
STARTED = time.time()

aref = AG.aref


@pytest.fixture(scope="module")
def shref(tmp_path_factory):
    return SH.load(tmp_path_factory.mktemp("shadow_ref_degenerate_gpu"))


SCENES = dict(aligned=SH.aligned_scene, extreme=SH.extreme_scene)
_CACHE = {}


def _scene(which, moved=False):
    key = ("scene", which, moved)
    if key not in _CACHE:
        s = SCENES[which]()
        _CACHE[key] = dict(s, draws=SH.moved_exactly(s)) if moved else s
    return _CACHE[key]


def _launches(which, moved=False, kind="all"):
    """every launch of degenerate_launches around the scene's instances, or its axis family again with checkerboard = 1"""
    key = ("launches", which, moved, kind)
    if key not in _CACHE:
        _CACHE[key] = SH.degenerate_launches(_scene(which, moved)) if kind == "all" else SH.degenerate_launches(_scene(which, moved), checkerboard=1, families=("axis",))
    return _CACHE[key]


def _want(shref, which, moved, kind, quality):
    """the restatement's masks of _launches(which, moved, kind), computed once and left unchanged"""
    key = ("want", which, moved, kind, quality)
    if key not in _CACHE:
        _CACHE[key] = SH.reference_masks(shref, _scene(which, moved), _launches(which, moved, kind), quality)
        _CACHE[key].setflags(write=False)
    return _CACHE[key]


class Batch:
    """the device depth images and masks of a list of launches, allocated once and reused: launch i reads depth image i and writes mask i,
    which is followed by 64 poisoned bytes of its own"""

    def __init__(self, ctx, launches):
        self.ctx, self.launches = ctx, launches
        self.depth = TS._dev(ctx, np.stack([d for _, _, d in launches]))
        self.masks = TS._out(ctx, len(launches) * STRIDE - TS.TAIL)

    def slices(self, i):
        return self.depth[4 * TEXELS * i:4 * TEXELS * (i + 1)], self.masks[STRIDE * i:STRIDE * i + TEXELS]

    def run(self, launch):
        """launch(sd, depth, mask) for every launch into re-poisoned masks: (launches, N, N) u8 on the host"""
        self.masks.fill_(POISON)
        for i, (_, sd, _) in enumerate(self.launches):
            launch(sd, *self.slices(i))
        self.ctx.status()
        n = len(self.launches)
        flat = TS._host(self.masks, n * STRIDE - TS.TAIL, np.uint8, (-1,))  # the last tail
        rows = np.concatenate([flat, np.full(TS.TAIL, POISON, np.uint8)]).reshape(n, STRIDE)
        assert (rows[:, TEXELS:] == POISON).all(), "bytes behind a mask were written"
        return rows[:, :TEXELS].reshape(n, N, N).copy()


def _compare(name, launches, got, want):
    """byte for byte, every launch; prints the totals and the first launches that differ before it asserts"""
    differ = (got != want).reshape(len(launches), -1).sum(1)
    TOTALS["launches"] += len(launches)
    TOTALS["rays"] += int((want != POISON).sum())
    TOTALS["differences"] += int(differ.sum())
    print("%s: %d launches, %d rays, %d occluded, %d lit, %d kept, %d differing bytes in %d launches" % (
        name, len(launches), int((want != POISON).sum()), int((want == 0).sum()), int((want == 255).sum()), int((want == POISON).sum()), int(differ.sum()),
        int((differ != 0).sum())))
    for i in np.flatnonzero(differ)[:20]:
        print("    %s: %d bytes differ" % (launches[i][0], int(differ[i])))
    print("the file so far: %(launches)d launches, %(rays)d rays, %(differences)d differences" % TOTALS, "in %.1f s" % (time.time() - STARTED))
    assert differ.sum() == 0


def _opaque(ctx, quality):
    return lambda sd, depth, mask: ctx.shadow_trace(sd, depth, mask, N, N, quality)


@pytest.fixture(scope="module", params=["aligned", "extreme"])
def static(request):
    """(name, context with the scene's static blob uploaded, its batches)"""
    from niagara_amd import pipeline as P
    which = request.param
    s = _scene(which)
    c = P.Context()
    blob = c.rt_scene_build(s["meshes"], s["indices"], s["vertices"], s["draws"])
    assert host.rt_scene_validate(blob)
    c.rt_scene_upload(blob)
    yield which, c, {kind: Batch(c, _launches(which, False, kind)) for kind in ("all", "checkerboard")}
    c.close()


# ---------------------------------------------------------------------------------------------------------------- 1. the opaque kernel

@pytest.mark.gpu
@pytest.mark.parametrize("quality", [0, 1])
def test_opaque_kernel_on_the_static_blob(static, quality, shref):
    """OpaqueQuery<0> and OpaqueQuery<1>: every launch of degenerate_launches, and the axis family once more with checkerboard = 1"""
    which, ctx, batches = static
    for kind in ("all", "checkerboard"):
        want = _want(shref, which, False, kind, quality)
        got = batches[kind].run(_opaque(ctx, quality))
        if kind == "checkerboard":
            y, x = np.mgrid[0:N, 0:N]
            other = ((x ^ y ^ 1) & 1) != 0
            assert (want[:, other] == POISON).all() and np.isin(want[:, ~other], (0, 255)).all() and (got[:, other] == POISON).all()
        else:  # equality is not vacuous: both outcomes in the axis family, and the denormal jitter changes results
            names = np.array([SH.family(l[0]) for l in batches[kind].launches])
            a0, a42 = want[names == "axis jitter 0"], want[names == "axis jitter 1e-42"]
            print("%s quality %d: axis jitter 0: %d occluded, %d lit; jitter 1e-42 differs in %d texels" % (which, quality, int((a0 == 0).sum()), int((a0 == 255).sum()),
                                                                                                      int((a0 != a42).sum())))
            assert (a0 == 0).sum() >= 1000 and (a0 == 255).sum() >= 1000 and (a0 != a42).sum() >= 200
            assert (want[names == "suns"] == 255).all()
        _compare("%s quality %d %s" % (which, quality, kind), batches[kind].launches, got, want)


# ---------------------------------------------------------------------------------------------------------------- 2. the closed box

@pytest.mark.gpu
def test_the_closed_box_is_closed_on_the_device(shref):
    """instance 0 alone, the six axis directions from outside: a ray through a shared edge or vertex is not lost between the box's triangles"""
    from niagara_amd import pipeline as P
    alone, six = SH.closed_box_launches(SH.aligned_scene())
    c = P.Context()
    try:
        c.rt_scene_upload(c.rt_scene_build(alone["meshes"], alone["indices"], alone["vertices"], alone["draws"]))
        batch = Batch(c, six)
        for quality in (0, 1):
            want = SH.reference_masks(shref, alone, six, quality)
            SH.closed_box_property("the restatement, quality %d" % quality, want)
            got = batch.run(_opaque(c, quality))
            SH.closed_box_property("the device, quality %d" % quality, got)
            _compare("closed box quality %d" % quality, six, got, want)
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------- 3. the alpha kernel, decoded set

def _alpha_conditions(name, want, rejected):
    print("%s: %d rays with a rejected candidate, %d occluded rays" % (name, int((rejected > 0).sum()), int((want == 0).sum())))
    assert (rejected > 0).sum() >= 200 and (want == 0).sum() >= 200


@pytest.mark.gpu
def test_alpha_kernel_with_the_decoded_set(aref):
    """AlphaQuery through nv_shadow_trace_textured at quality 1 on the textured aligned scene of tests/test_shadow_alpha_cpu.py; quality 0 is
    nv_shadow_trace's bytes"""
    s, t = SA.textured_aligned_scene()
    launches = SH.degenerate_launches(s)
    dev = AG.Device(s, t)
    try:
        batch = Batch(dev.ctx, launches)
        args = dev.args()
        want, rejected = SA.reference_masks(aref, s, t, launches, 1)
        _alpha_conditions("textured aligned scene", want, rejected)
        got = batch.run(lambda sd, depth, mask: dev.ctx.shadow_trace_textured(sd, depth, mask, N, N, 1, **args))
        _compare("alpha kernel, decoded set", launches, got, want)
        q0 = batch.run(lambda sd, depth, mask: dev.ctx.shadow_trace_textured(sd, depth, mask, N, N, 0, **args))
        opaque = batch.run(_opaque(dev.ctx, 0))
        assert q0.tobytes() == opaque.tobytes() and np.isin(q0, (0, 255)).all() and (q0 != got).any()
    finally:
        dev.ctx.close()


# ---------------------------------------------------------------------------------------------------------------- 4. the alpha kernel, block-resident set

def _bc_files(rng):
    """four textures of shadow_alpha_ref.random_textures' first shapes as DDS files of random blocks: BC1, BC3, BC7 (a valid mode each), BC2"""
    files = []
    for (w, h, levels), fmt in zip([(8, 8, 1), (5, 3, 2), (16, 4, 3), (7, 1, 1)], (1, 3, 7, 2)):
        b = rng.integers(0, 256, TB.TR.image_size_bc(w, h, levels, TB.TR.BLOCK_BYTES[fmt])[0], dtype=np.uint8)
        if fmt == 7:
            b[0::16] |= 1 << 6
        files.append(TB.TG._dds(fmt, w, h, levels, b))
    return files


@pytest.mark.gpu
@pytest.mark.parametrize("albedo", [(1, 2, 3), (2, 1, 4)])
def test_alpha_kernel_with_the_block_resident_set(albedo, aref):
    """nv_shadow_trace_blocks on the same scene with its textures as BC1, BC3, BC7 and BC2 files: the mask is the decoded entry point's on the
    same device and the restatement's over the decoded form.  The scene's wall is opaque (postPass 0), so a material table samples two of
    its three textures: (1, 2, 3) samples the BC1 and the BC7 texture, (2, 1, 4) the BC3 and the BC2 one"""
    from niagara_amd import pipeline as P
    s, _ = SA.textured_aligned_scene()
    s["materials"] = s["materials"].copy()
    s["materials"]["albedoTexture"] = albedo
    files = _bc_files(np.random.default_rng(79))
    dev = TB.TraceDevice(s, files)
    try:
        assert [int(d["levelsFormat"]) >> 8 for d in dev.bdescs[1:]] == [1, 3, 7, 2]
        assert P.from_device(dev.materials, s["materials"].dtype)["albedoTexture"].tolist() == list(albedo)
        launches = SH.degenerate_launches(s)
        batch = Batch(dev.ctx, launches)
        want, rejected = SA.reference_masks(aref, s, dev.tset, launches, 1)
        _alpha_conditions("BC set, albedo %s" % (albedo,), want, rejected)
        decoded = batch.run(lambda sd, depth, mask: dev.ctx.shadow_trace_textured(sd, depth, mask, N, N, 1, **dev.args()))
        blocks = batch.run(lambda sd, depth, mask: dev.ctx.shadow_trace_blocks(sd, depth, mask, N, N, 1, **dev.block_args()))
        g = dev.guarded.cpu().numpy()
        assert (g[:TB.GUARD] == TB.CANARY).all() and (g[-TB.GUARD:] == TB.CANARY).all(), "a canary of the block buffer was written"
        assert blocks.tobytes() == decoded.tobytes()
        _compare("alpha kernel, block-resident set, albedo %s" % (albedo,), launches, blocks, want)
    finally:
        dev.ctx.close()


# ---------------------------------------------------------------------------------------------------------------- 5. the device-rebuilt TLAS

@pytest.mark.gpu
@pytest.mark.parametrize("which", ["aligned", "extreme"])
def test_opaque_kernel_on_the_device_rebuilt_tlas(which, shref):
    """static upload -> reserve -> the draws moved by exact amounts -> rt_tlas_build -> the moved scene's launches; then a rebuild from the
    unmoved draws and the static scene's launches again"""
    from niagara_amd import pipeline as P
    s, moved = _scene(which), _scene(which, True)
    blob = host.rt_scene_build(s["meshes"], s["indices"], s["vertices"], s["draws"])
    c = P.Context()
    try:
        c.rt_scene_upload(blob)
        c.rt_scene_reserve_dynamic(len(s["draws"]))
        # before the first rebuild the static TLAS answers the moved scene's launches, and differently: the move matters (the bound is the
        # one tests/test_tlas_build_gpu.py asks of its moved draws)
        batch = Batch(c, _launches(which, True))
        stale = SH.reference_masks(shref, s, batch.launches, 1)
        differ = int((stale != _want(shref, which, True, "all", 1)).sum())
        print("%s: the static scene answers %d texels of the moved scene's launches differently" % (which, differ))
        assert differ >= 50
        _compare("%s reserved, static TLAS, quality 1" % which, batch.launches, batch.run(_opaque(c, 1)), stale)
        for name, scene, is_moved in (("moved", moved, True), ("unmoved", s, False)):
            keep = TT._rebuild(c, scene["draws"])
            got_blob = c.rt_scene_download()
            assert got_blob.tobytes() == host.rt_tlas_build_host(blob, scene["draws"]).tobytes() and host.rt_scene_validate(got_blob)
            if which == "extreme":
                leaves = SH.infinite_leaves(TR.sections(got_blob)[1])
                print("%s %s: %d TLAS leaves with the infinite box" % (which, name, len(leaves)))
                assert len(leaves) >= 1
            batch = batch if is_moved else Batch(c, _launches(which, False))
            for quality in (0, 1):
                want = _want(shref, which, is_moved, "all", quality)
                _compare("%s %s, rebuilt TLAS, quality %d" % (which, name, quality), batch.launches, batch.run(_opaque(c, quality)), want)
            del keep
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------- 6. a captured graph

@pytest.mark.gpu
def test_one_launch_replays_from_a_captured_graph(static, shref):
    """the kernel arguments carry the hand-made matrix by value: one axis launch with jitter 0, captured once and replayed twice"""
    import torch
    which, ctx, batches = static
    launches = batches["all"].launches
    i = [l[0] for l in launches].index("axis jitter 0: instance 0 k 1 sign -1 start -1")
    name, sd, depth_host = launches[i]
    sd = sd.copy()
    want = _want(shref, which, False, "all", 1)[i]
    assert (want == 0).sum() >= 20 and (want == 255).sum() >= 20
    depth, shadow = TS._dev(ctx, depth_host), TS._out(ctx, TEXELS)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            ctx.shadow_trace(sd, depth, shadow, N, N, 1)
        torch.cuda.synchronize()
        assert (shadow == POISON).all()  # nothing ran during capture
        sd["inverseViewProjection"] = 0.0  # the launch holds its own copy
        for _ in range(2):
            shadow.fill_(POISON)
            graph.replay()
            torch.cuda.synchronize()
            TG._report("%s: %s, replayed" % (which, name), TS._host(shadow, TEXELS, np.uint8, (N, N)), want)
    ctx.status()
