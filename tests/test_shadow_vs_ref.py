"""The shadow pass's restatements against shadow.comp.glsl itself executing on the CPU: tests/shadow_ref.c and
tests/shadow_alpha_ref.c equal oracle/_ref's translation of the shader — run against the CPU ray query of oracle/glsl_rayquery_shim.h — in the
ray of every invocation BIT FOR BIT and in the mask BYTE FOR BYTE, prefill bytes included.

The criterion is derived, not measured: both sides are fp32 and built with oracle/Makefile's FPFLAGS (one IEEE operation per source operation,
no contraction); the ray set-up and the triangle test T hold no pow or exp2.  There is no tolerance; a NaN matches a NaN.  T, the object-space
ray and the λ = 0 sampler are NOT what is pinned: the shim takes the first two from the library (niagara_amd/csrc/rtmath.h, rtalpha.h) and T has
tests of its own (tests/test_shadowtrace_cpu.py); the shim's sampler is held against nv_rt_alpha_sample_host on the uv the run produced before
any textured mask is compared.  What IS pinned is every statement around them: the checkerboard column, uv / clip, the unprojection, which of
pos.xy / pos.yx feeds which jitter term, tmin / tmax, the flags, which draws cast and which are forced opaque, objid -> draw -> material ->
lods[lodRT].indexOffset, the order of the uv interpolation, albedoTexture > 0, alpha >= 0.5.

A "case" of the mask tests is one (quality, checkerboard, sunJitter) over the three image sizes together: 21 x 3 alone has 63 rays, fewer than
the 100 lit and 100 shadowed a case must hold.  Every test first asserts, on the reference's output and the inputs alone, that the branches it
is about are taken, and prints the counts.  The whole file skips where oracle/_ref is not built, and fails where it was built before it held the
shadow shader; tests/test_shadow_fixtures_cpu.py replays what it pins from committed fixtures."""
import numpy as np
import pytest

import oracle.ref as R
import shadow_alpha_ref as SA
import shadow_cases as SC
import shadow_ref as SH
from niagara_amd import host

pytestmark = pytest.mark.skipif(not R.available(), reason="oracle/_ref not built (no reference tree and no prebuilt .so)")
same = SC.same_bits
CHECKERBOARDS = (0, 1, 2)
JITTERS = (0.0, 1e-2)
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module", autouse=True)
def _the_built_reference_holds_the_shadow_shader():
    """a libniagara_ref.so from before shadow.comp.glsl was translated is an out-of-date build, not a reason to skip"""
    assert R.has_shadow(), "oracle/_ref/libniagara_ref.so is out of date: it has no ref_shadow.  Run `make -C oracle ref` where the reference tree is"


@pytest.fixture(scope="module")
def shref(tmp_path_factory):
    return SH.load(tmp_path_factory.mktemp("shadow_ref_vs_ref"))


@pytest.fixture(scope="module")
def aref(tmp_path_factory):
    return SA.load(tmp_path_factory.mktemp("shadow_alpha_ref_vs_ref"))


def _zero(name, ok):
    ok = np.asarray(ok)
    print("%s: %d elements, %d differ" % (name, ok.size, int((~ok).sum())))
    assert ok.all(), "%s: %d of %d differ, first at %s" % (name, int((~ok).sum()), ok.size, np.argwhere(~ok)[:4].tolist())


def _run(sd, depth, s, quality, tset=None):
    return R.shadow(sd, depth, s["meshes"], s["indices"], s["vertices"], s["draws"], s.get("materials") if tset is not None else None, tset, quality, SC.PREFILL)


def _stored(r, w, h, checkerboard):
    """the texels the reference stored to; they are the parity the checkerboard owns, everything else keeps the prefill byte"""
    stored = r["queries"] > 0
    assert (r["queries"][stored] == 1).all()
    assert (stored == SC.owned(w, h, checkerboard)).all()
    assert (r["mask"][~stored] == SC.PREFILL).all() and np.isin(r["mask"][stored], (0, 255)).all()
    return stored


def _expected_drops(w, h, checkerboard):
    """(stores outside the image, those at pos.x == width inside the rows), from the dispatch alone: W' x h invocations rounded up to 8 x 8 groups"""
    wi = (w + 1) // 2 if checkerboard > 0 else w
    gx, gy = np.meshgrid(np.arange((wi + 7) // 8 * 8), np.arange((h + 7) // 8 * 8))
    px = gx * 2 + ((gy ^ checkerboard) & 1) if checkerboard > 0 else gx
    out = (px >= w) | (gy >= h)
    return int(out.sum()), int(((px == w) & (gy < h)).sum())


# ---- the ray of an invocation (shadow.comp.glsl:125-151, :81 / :89)

@pytest.mark.parametrize("size", SC.SIZES, ids=lambda s: "%dx%d" % s)
def test_ray_setup(size, shref):
    w, h = size
    s = SC.opaque_scene()
    for checkerboard in CHECKERBOARDS:
        dirs = {}
        for jitter in JITTERS + ("zero sun", "dense matrix"):
            zero_sun, dense = jitter == "zero sun", jitter == "dense matrix"
            sd, depth = SC.inputs(w, h, 0.0 if zero_sun else 1e-2 if dense else jitter, checkerboard, sun=(0.0, 0.0, 0.0) if zero_sun else SC.SUN, odd=True,
                                  dense=dense)
            assert not dense or (sd["inverseViewProjection"] != 0).all()
            for quality in (0, 1):
                r = _run(sd, depth, s, quality)
                stored = _stored(r, w, h, checkerboard)
                name = "%dx%d checkerboard %d jitter %s quality %d" % (w, h, checkerboard, jitter, quality)
                o, d = r["rays"][..., :3], r["rays"][..., 3:6]
                sky = stored & (depth == 0)
                odd = stored & ~np.isfinite(depth)
                drops = (r["dropped"], r["dropped_at_width"])
                print("%s: %d rays, %d sky, %d with a non-finite depth texel, %d with a non-finite origin, %d with a non-finite direction; stores "
                      "dropped %d, at pos.x == width %d" % (name, int(stored.sum()), int(sky.sum()), int(odd.sum()), int((~np.isfinite(o).all(-1) & stored).sum()),
                                                            int((~np.isfinite(d).all(-1) & stored).sum()), *drops))
                assert sky.sum() > 0 and (dense or not np.isfinite(o[sky]).all(-1).any())  # depth == 0: wposh.w == 0 under the camera's matrix
                assert odd.sum() > 0
                assert drops == _expected_drops(w, h, checkerboard)
                assert drops[1] > 0 if checkerboard > 0 else drops[1] == (h if w % 8 else 0)  # every width here is odd: the last column's right neighbour
                if zero_sun:
                    assert not np.isfinite(d[stored]).any()  # 0 / 0
                    assert (r["mask"][stored] == 255).all()
                want_o, want_d = shref.rays(sd, depth)
                _zero(name + ", origins", same(o, want_o)[stored])
                _zero(name + ", directions", same(d, want_d)[stored])
                assert (r["rays"][..., 6][stored] == SC.TMIN).all() and (r["rays"][..., 7][stored] == SC.TMAX).all()
                assert (r["flags"][stored] == SC.FLAGS[quality]).all()
                if jitter in JITTERS:
                    dirs[jitter] = (d, stored)
        (d0, stored), (d1, _) = dirs[0.0], dirs[1e-2]
        moved = (d0[..., 0] != d1[..., 0]) & (d0[..., 2] != d1[..., 2])
        sun = np.asarray(SC.SUN, np.float32)
        print("%dx%d checkerboard %d: the jitter moves x and z of %d of %d directions; without it every direction is one vector: %s" % (
            w, h, checkerboard, int(moved[stored].sum()), int(stored.sum()), np.unique(d0[stored], axis=0).tolist()))
        # 90 %, not all: gradientNoise can return exactly 0.5, for which (n * 2 - 1) * sunJitter is 0 and that component stays where it was; and a
        # component moved by less than half an ulp rounds back.  The share is a condition on the inputs, not a tolerance: every direction is
        # compared bit for bit above
        assert moved[stored].mean() >= 0.9
        assert len(np.unique(d0[stored], axis=0)) == 1 and np.abs(d0[stored][0] - sun).max() < 1e-6
        assert (np.abs(d1[..., 0] - sun[0])[stored] > 0).mean() >= 0.9 and (np.abs(d1[..., 2] - sun[2])[stored] > 0).mean() >= 0.9


# ---- tmin and tmax (:81, :89), from both sides

def test_tmin_and_tmax_exactly(shref, aref):
    """shadow_cases.range_case: four rays whose only triangle lies at t = 2^-7, 2^-6, 512 and 1024 exactly (see there for why nothing rounds).
    The random scenes hold no hit in (1e-2, 2e-2] and none beyond 1e3, so their masks cannot tell a tmin of 2e-2 or a tmax of 1e4 from the
    shader's; these rays can.  The reference alone: lit, shadowed, shadowed, lit, through the opaque commit (postPass 0, quality 0 and 1) and
    through candidate and confirm (postPass 1, textured).  Then the restatements, byte for byte"""
    sd, depth, opaque, textured, tset, _ = SC.range_case()
    for q in (0, 1):
        r = _run(sd, depth, opaque, q)
        print("t = %s, quality %d: mask %s, opaque commits %s" % (list(SC.RANGE_T), q, r["mask"][0].tolist(), r["opaque_commits"][0].tolist()))
        assert (r["rays"][0, :, 6] == SC.TMIN).all() and (r["rays"][0, :, 7] == SC.TMAX).all()
        assert (r["rays"][0, :, :3] == [[2, 1, 0], [18, 1, 0], [34, 1, 0], [50, 1, 0]]).all() and (r["rays"][0, :, 3:6] == [0, 0, 1]).all()
        assert (r["mask"] == SC.RANGE_MASK).all() and (r["opaque_commits"][0] == [0, 1, 1, 0]).all()
        _zero("tmin / tmax, quality %d" % q, shref.shadow_trace(sd, opaque, depth, np.full((1, 4), SC.PREFILL, np.uint8), q) == r["mask"])
    r = _run(sd, depth, textured, 1, tset)
    print("textured: mask %s, candidates %s, confirmed %s" % (r["mask"][0].tolist(), r["candidates"][0].tolist(), r["confirmed"][0].tolist()))
    _sampler_first(r, tset)
    assert (r["mask"] == SC.RANGE_MASK).all() and (r["candidates"][0] == [0, 1, 1, 0]).all() and (r["confirmed"][0] == [0, 1, 1, 0]).all()
    want, rejected = aref.shadow_trace(sd, textured, tset, depth, np.full((1, 4), SC.PREFILL, np.uint8), 1)
    _zero("tmin / tmax, textured", want == r["mask"])
    assert (rejected == 0).all()


# ---- the masks, untextured: which draws cast (fillInstanceRT), quality 0 and 1

@pytest.mark.parametrize("jitter", JITTERS)
@pytest.mark.parametrize("checkerboard", CHECKERBOARDS)
@pytest.mark.parametrize("quality", [0, 1])
def test_untextured_masks(quality, checkerboard, jitter, shref):
    s = SC.opaque_scene()
    post = s["draws"]["postPass"]
    assert set(post.tolist()) == {0, 2}
    lit = dark = 0
    for w, h in SC.SIZES:
        sd, depth = SC.inputs(w, h, jitter, checkerboard)
        r = _run(sd, depth, s, quality)
        stored = _stored(r, w, h, checkerboard)
        hit = r["committed_instance"][stored & (r["mask"] == 0)]
        assert (r["candidates"] == 0).all() and (r["committed_instance"][stored & (r["mask"] == 255)] == NONE).all()
        assert (post[hit] == 0).all()  # draws with postPass == 2 contribute no hit
        lit, dark = lit + int((r["mask"][stored] == 255).sum()), dark + int((r["mask"][stored] == 0).sum())
        handed = r["handed"][stored]
        assert (handed[:, 0] == (r["mask"][stored] == 255)).all() and (handed[:, 1:] == 0).all()  # vec4(shadow, 0, 0, 0)
        want = shref.shadow_trace(sd, s, depth, np.full((h, w), SC.PREFILL, np.uint8), quality)
        _zero("%dx%d quality %d checkerboard %d jitter %g" % (w, h, quality, checkerboard, jitter), r["mask"] == want)
    print("quality %d checkerboard %d jitter %g: %d lit, %d shadowed; %d of %d draws have postPass 2 and hit nothing" % (
        quality, checkerboard, jitter, lit, dark, int((post == 2).sum()), len(post)))
    assert lit >= 100 and dark >= 100 and (post == 2).sum() >= 3


@pytest.mark.parametrize("jitter", JITTERS)
@pytest.mark.parametrize("checkerboard", CHECKERBOARDS)
def test_quality_0_with_post_pass_draws(checkerboard, jitter, shref):
    """shadowTrace (:78-84) calls rayQueryProceedEXT once: where a non-opaque triangle is accepted before an opaque one the outcome depends on the
    walk order, and the library defines post-pass draws as non-casters at quality 0.  The rays for which the shim logged no
    non-opaque candidate are compared; the others are counted"""
    s = SC.mixed_scene()
    assert set(s["draws"]["postPass"].tolist()) == {0, 1, 2}
    rays = left = lit = dark = 0
    for w, h in SC.SIZES:
        sd, depth = SC.inputs(w, h, jitter, checkerboard)
        r = _run(sd, depth, s, 0)
        stored = _stored(r, w, h, checkerboard)
        compared = stored & (r["candidates"] == 0)
        rays, left = rays + int(stored.sum()), left + int((stored & ~compared).sum())
        lit, dark = lit + int((r["mask"][compared] == 255).sum()), dark + int((r["mask"][compared] == 0).sum())
        want = shref.shadow_trace(sd, s, depth, np.full((h, w), SC.PREFILL, np.uint8), 0)
        _zero("%dx%d quality 0 checkerboard %d jitter %g, rays without a non-opaque candidate and prefill bytes" % (w, h, checkerboard, jitter),
              (r["mask"] == want)[compared | ~stored])
    print("quality 0 with post-pass draws, checkerboard %d jitter %g: %d rays, %d left out (a non-opaque candidate), %d compared lit, %d compared shadowed" % (
        checkerboard, jitter, rays, left, lit, dark))
    assert 0 < left <= rays // 2 and lit >= 100 and dark >= 100


# ---- quality 1, textured: shadowTraceTransparent (:86-123)

def _sampler_first(r, tset):
    """the shim's textureLod alone equals nv_rt_alpha_sample_host's four-tap alpha, bit for bit, on the uv set the run produced; a later difference
    of masks is then not the sampler's.  Returns the ids sampled"""
    sm = r["samples"]
    ids = sm[:, 0].astype(np.int64)
    for i in np.unique(ids):
        mine = sm[ids == i]
        if 0 < i < len(tset["descs"]):
            four_tap, full = host.rt_alpha_sample_host(tset["descs"][i], tset["texels"], mine[:, 1:3])
            _zero("the shim's sampler against nv_rt_alpha_sample_host, texture %d (%d samples)" % (i, len(mine)), same(four_tap, mine[:, 3]) & same(full, mine[:, 3]))
        else:
            assert (mine[:, 3] == 1).all()  # a texture past the table is "no texture": alpha 1
    return set(ids.tolist())


def _uv_first(r, s, aref):
    """every textureLod call of the run was made with the texture and the uv the restatement forms for that candidate: objid -> draw -> material
    -> albedoTexture, draw -> mesh -> lods[lodRT].indexOffset -> indices -> vertexOffset -> the corners' texcoords, and :113's interpolation (bit
    for bit, from the barycentrics the shim handed out).  The chain of indices is written out once more here, in numpy"""
    sm = r["samples"]
    if not len(sm):
        return
    inst, prim = sm[:, 4].astype(np.int64), sm[:, 5].astype(np.int64)
    draws, meshes = s["draws"][inst], s["meshes"][s["draws"]["meshIndex"][inst]]
    assert (draws["postPass"] == 1).all()  # only non-opaque instances hand out candidates
    _zero("the texture each sample names", sm[:, 0].astype(np.int64) == s["materials"]["albedoTexture"][draws["materialIndex"]])
    first = meshes["lods"]["indexOffset"][np.arange(len(sm)), meshes["lodRT"]].astype(np.int64)
    corners = s["indices"][first[:, None] + 3 * prim[:, None] + np.arange(3)].astype(np.int64) + meshes["vertexOffset"].astype(np.int64)[:, None]
    tu, tv = (s["vertices"][k][corners].view(np.float16).astype(np.float32) for k in ("tu", "tv"))
    _zero("the uv of every sample against the restatement's interpolation", same(aref.interpolate_uv(sm[:, 6:8], tu, tv), sm[:, 1:3]).all(1))


@pytest.mark.parametrize("jitter", JITTERS)
@pytest.mark.parametrize("checkerboard", CHECKERBOARDS)
def test_quality_1_textured(checkerboard, jitter, aref):
    s, tset = SC.textured_scene()
    m = s["materials"]["albedoTexture"]
    assert (m == 0).sum() == 1 and (m >= len(tset["descs"])).sum() == 1
    confirmed = rejected = opaque = through = 0
    sampled = set()
    for w, h in SC.SIZES:
        sd, depth = SC.inputs(w, h, jitter, checkerboard)
        r = _run(sd, depth, s, 1, tset)
        stored = _stored(r, w, h, checkerboard)
        sampled |= _sampler_first(r, tset)
        _uv_first(r, s, aref)
        rej = r["candidates"].astype(np.int64) - r["confirmed"]
        confirmed, rejected, opaque = confirmed + int(r["confirmed"].sum()), rejected + int(rej.sum()), opaque + int(r["opaque_commits"].sum())
        through += int((stored & (rej > 0) & (r["confirmed"] == 0) & (r["opaque_commits"] == 0) & (r["mask"] == 255)).sum())
        want, want_rejected = aref.shadow_trace(sd, s, tset, depth, np.full((h, w), SC.PREFILL, np.uint8), 1)
        _zero("%dx%d textured checkerboard %d jitter %g" % (w, h, checkerboard, jitter), r["mask"] == want)
        # the restatement ends no loop early: it rejects at least what the walk rejected before it stopped, and exactly that for a lit ray
        assert (want_rejected >= rej).all() and (want_rejected == rej)[stored & (r["mask"] == 255)].all()
    print("textured, checkerboard %d jitter %g: %d confirmed, %d rejected candidates, %d opaque commits, %d rays lit after every accepted triangle was "
          "rejected; textures sampled: %s" % (checkerboard, jitter, confirmed, rejected, opaque, through, sorted(sampled)))
    assert confirmed >= 100 and rejected >= 100 and opaque >= 100 and through >= 1
    assert 1 in sampled and int(m.max()) in sampled and 0 not in sampled  # albedoTexture > 0 (:116)


def test_alpha_of_exactly_one_half_confirms(aref):
    """shadow_cases.half_alpha_case: the hit lands on alpha == 0.5 exactly (the construction is exact in fp32, see there); `>= 0.5` (:119) confirms"""
    sd, depth, s, tset, uv = SC.half_alpha_case()
    r = _run(sd, depth, s, 1, tset)
    sm = r["samples"]
    print("alpha == 0.5: %d samples, uv %s, alpha %s; mask %d" % (len(sm), sm[0, 1:3].tolist(), sm[0, 3], int(r["mask"][0, 0])))
    assert len(sm) >= 1 and (sm[:, 1:3] == uv).all() and (sm[:, 3] == np.float32(0.5)).all()
    _sampler_first(r, tset)
    _uv_first(r, s, aref)
    assert r["candidates"][0, 0] == 1 and r["confirmed"][0, 0] == 1 and r["mask"][0, 0] == 0
    want, rejected = aref.shadow_trace(sd, s, tset, depth, np.full((1, 1), SC.PREFILL, np.uint8), 1)
    assert want[0, 0] == 0 and rejected[0, 0] == 0
