"""The shadow fixtures on the MI355X: tests/golden/shadow/*.npz hold the masks the reference's own
shadow.comp.glsl, run on the CPU, makes of fixed inputs.  nv_shadow_trace at quality 0 and 1, nv_shadow_trace_textured and
nv_shadow_trace_blocks equal them byte for byte, prefill bytes included (there is no tolerance: nothing in the pass holds pow or exp2), and the
first two do again after nv_rt_scene_reserve_dynamic + nv_rt_tlas_build over the fixture's draws, on a scene uploaded with its draws
elsewhere.  The range fixture's four rays hold tmin and tmax from both sides.  Only the fixtures are read, never the reference tree.  Outputs are poisoned with the fixtures' prefill byte before every launch and carry a tail that must keep its bytes; the block buffer
sits between canaries."""
import numpy as np
import pytest

import shadow_cases as SC
import test_shade_gpu as TS
import test_texture_blocks_gpu as BG
from niagara_amd import host

FILES = SC.FIXTURES
assert TS.POISON == SC.PREFILL


class Plain:
    """a context with the untextured scene of a fixture uploaded; built_from: the draws the blob is built over (the scene's own by default)"""

    def __init__(self, scene, built_from=None):
        from niagara_amd import pipeline as P
        self.scene = scene
        self.ctx = P.Context()
        self.blob = self.ctx.rt_scene_build(scene["meshes"], scene["indices"], scene["vertices"], scene["draws"] if built_from is None else built_from)
        self.ctx.rt_scene_upload(self.blob)

    def trace(self, sd, depth, quality):
        h, w = depth.shape
        d, out = TS._dev(self.ctx, depth), TS._out(self.ctx, w * h)
        self.ctx.shadow_trace(sd, d, out, w, h, quality)
        self.ctx.status()
        return TS._host(out, w * h, np.uint8, (h, w))


def _devices(f, moved=False):
    """(Plain, test_texture_blocks_gpu.TraceDevice) over a fixture's two scenes.  moved: the blobs are built over shadow_cases.moved(draws); the
    tables of the alpha test hold the fixture's own draws either way"""
    from niagara_amd import pipeline as P
    opaque, (textured, tset) = SC.fixture_scene(f, False)[0], SC.fixture_scene(f, True)
    plain = Plain(opaque, SC.moved(opaque["draws"]) if moved else None)
    tex = BG.TraceDevice(dict(textured, draws=SC.moved(textured["draws"])) if moved else textured, SC.fixture_files(f))
    tex.scene, tex.draws = textured, P.to_device(textured["draws"], tex.ctx.device)
    assert tex.tset["descs"].tobytes() == tset["descs"].tobytes() and tex.tset["texels"].tobytes() == tset["texels"].tobytes()
    return plain, tex


SCENE_KEYS = ("meshes", "indices", "vertices", "draws_opaque", "draws_textured", "materials", "descs", "texels", "dds")


@pytest.fixture(scope="module")
def devices():
    """the devices of a fixture, shared by the fixtures that hold the same scene (the three sizes do)"""
    cache = {}

    def get(f):
        key = b"".join(f[k].tobytes() for k in SCENE_KEYS)
        if key not in cache:
            cache[key] = _devices(f)
        return cache[key]
    yield get
    for plain, tex in cache.values():
        plain.ctx.close()
        tex.ctx.close()


def _equal(name, got, want):
    diff = int((got != want).sum())
    print("%s: %d texels, %d occluded, %d lit, %d kept, %d differences" % (name, want.size, int((want == 0).sum()), int((want == 255).sum()),
                                                                          int((want == SC.PREFILL).sum()), diff))
    assert diff == 0


def _masks(f, plain, textured, blocks):
    """name -> the mask each entry point leaves, for every launch of the fixture"""
    out = {}
    for k in range(len(f["sd"])):
        sd, depth = SC.fixture_launch(f, k)
        for q in (0, 1):
            out["launch %d, nv_shadow_trace quality %d" % (k, q)] = (plain.trace(sd, depth, q), f["mask_q%d_%d" % (q, k)])
        out["launch %d, nv_shadow_trace_textured" % k] = (textured.trace(sd, depth, 1), f["mask_tex_%d" % k])
        if blocks:
            out["launch %d, nv_shadow_trace_blocks" % k] = (textured.trace_blocks(sd, depth, 1), f["mask_tex_%d" % k])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("path", FILES, ids=SC.FIXTURE_IDS)
def test_the_kernels_replay_the_fixture(path, devices):
    f = np.load(path)
    for name, (got, want) in _masks(f, *devices(f), blocks=True).items():
        _equal(name, got, want)
    if path == SC.RANGE_FIXTURE:
        assert (f["mask_q0_0"] == SC.RANGE_MASK).all() and (f["mask_tex_0"] == SC.RANGE_MASK).all()  # tmin and tmax from both sides


def _rebuilt(path):
    """the scene is uploaded with its draws ELSEWHERE (shadow_cases.moved), where the masks are others than the fixture's; then
    nv_rt_scene_reserve_dynamic + nv_rt_tlas_build over the fixture's draws: the rebuilt tree is the one walked, and the masks are the fixture's"""
    from niagara_amd import pipeline as P
    f = np.load(path)
    plain, textured = _devices(f, moved=True)
    try:
        for name, (got, want) in _masks(f, plain, textured, blocks=False).items():
            print("%s before the rebuild: %d of %d texels differ from the fixture" % (name, int((got != want).sum()), want.size))
            assert (got != want).sum() >= (1 if path == SC.RANGE_FIXTURE else 50)
        for dev in (plain, textured):
            draws = dev.scene["draws"]
            dev.ctx.rt_scene_reserve_dynamic(len(draws))
            before = dev.ctx.rt_scene_download()
            dev.rebuilt_from = P.to_device(draws, dev.ctx.device)
            dev.ctx.rt_tlas_build(dev.rebuilt_from, len(draws))
            dev.ctx.status()
            after = dev.ctx.rt_scene_download()
            assert after.tobytes() != before.tobytes() and after.tobytes() == host.rt_tlas_build_host(dev.blob, draws).tobytes()
        for name, (got, want) in _masks(f, plain, textured, blocks=False).items():
            _equal(name + ", rebuilt TLAS", got, want)
    finally:
        plain.ctx.close()
        textured.ctx.close()


@pytest.mark.gpu
def test_the_kernels_replay_the_fixtures_over_a_rebuilt_tlas():
    """the largest image and the range case's four rays"""
    for path in (SC.SIZE_FIXTURES[-1], SC.RANGE_FIXTURE):
        _rebuilt(path)
