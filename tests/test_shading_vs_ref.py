"""The shading restatements against the reference's own shader text executing on the CPU: tests/shade_ref.c, bloom_ref.c,
visattr_ref.c and texture_ref.c, built as fp32, equal oracle/_ref's translation of shadowfill / shadowblur / final / bloom / mesh.frag and of
the helpers of src/shaders/math.h:51-109 BIT FOR BIT — the value handed to every store and the stored word.

The criterion is derived, not measured: both sides are fp32, both are built with oracle/Makefile's FPFLAGS (one IEEE operation per source
operation, no contraction), both call glibc's powf / exp2f / log2f.  There is no tolerance; a NaN matches a NaN whatever its sign or payload.
Every test first asserts, on the reference's output and the inputs alone, that the branches it is about are taken, and prints the counts.
The whole file skips where oracle/_ref is not built; tests/test_shade_fixtures_cpu.py replays what it pins from committed fixtures."""
import ctypes as C

import numpy as np
import pytest

import bloom_ref as BR
import oracle.ref as R
import pixel_cases as PC
import shade_cases as SC
import shade_ref as SR
import texture_ref as TR
import visattr_ref as VA

pytestmark = pytest.mark.skipif(not R.available(), reason="oracle/_ref not built (no reference tree and no prebuilt .so)")
same = SC.same_bits


@pytest.fixture(scope="module")
def sref(tmp_path_factory):
    return SR.load(tmp_path_factory.mktemp("shade_ref_vs_ref"))


@pytest.fixture(scope="module")
def bref(tmp_path_factory):
    return BR.load(tmp_path_factory.mktemp("bloom_ref_vs_ref"))


@pytest.fixture(scope="module")
def aref(tmp_path_factory):
    return VA.load(tmp_path_factory.mktemp("visattr_ref_vs_ref"))


@pytest.fixture(scope="module")
def tref(tmp_path_factory):
    return TR.load(tmp_path_factory.mktemp("texture_ref_vs_ref"))


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _call(lib, name, src, width_out):
    """one of the restatements' thin array wrappers (fp32 build): src (n, k) f32 -> (n, width_out) f32"""
    src = np.ascontiguousarray(src, np.float32)
    out = np.zeros((len(src), width_out), np.float32)
    getattr(lib, name)(_p(src), C.c_uint32(len(src)), _p(out))
    return out


def _zero(name, ok):
    ok = np.asarray(ok)
    print("%s: %d elements, %d differ" % (name, ok.size, int((~ok).sum())))
    assert ok.all(), "%s: %d of %d differ, first at %s" % (name, int((~ok).sum()), ok.size, np.argwhere(~ok)[:4].tolist())


# ---- the helpers of src/shaders/math.h:51-109

def test_unpack_tbn_over_every_code(aref):
    rng = np.random.default_rng(5)
    tp = np.arange(1 << 16, dtype=np.uint32)
    cases = [(np.full(len(tp), 0x1FF7FDFF, np.uint32), tp)]
    for field in range(3):
        for bit30 in (0, 1):
            code = np.arange(1024, dtype=np.uint32)
            other = rng.integers(0, 1 << 30, 1024).astype(np.uint32) & ~np.uint32(1023 << (10 * field))
            cases.append((other | code << np.uint32(10 * field) | np.uint32(bit30 << 30) | np.uint32(rng.integers(0, 2) << 31), rng.integers(0, 1 << 16, 1024).astype(np.uint32)))
    for k, (npc, tpc) in enumerate(cases):
        n_ref, t_ref = R.unpack_tbn(npc, tpc)
        n_got, t_got = np.zeros_like(n_ref), np.zeros_like(t_ref)
        aref.libs["f32"].va_x_unpack_tbn(_p(npc), _p(tpc), C.c_uint32(len(npc)), _p(n_got), _p(t_got))
        print("unpackTBN case %d: tangent.w -1 at %d of %d, t > 0 in decodeOct at %d" % (k, int((t_ref[:, 3] == -1).sum()), len(npc), int((t_ref[:, 2] < 0).sum())))
        assert k == 0 or {float(v) for v in np.unique(t_ref[:, 3])} == ({-1.0} if k % 2 == 0 else {1.0})
        assert k != 0 or ((t_ref[:, 2] < 0).any() and (t_ref[:, 2] > 0).any())
        _zero("unpackTBN normal, case %d" % k, same(n_got, n_ref))
        _zero("unpackTBN tangent, case %d" % k, same(t_got, t_ref))


def _oct_grid():
    a = np.array([-1.0, -0.75, -0.5, -0.25, -1.0 / 3.0, -0.0, 0.0, 1e-30, 0.125, 0.25, 0.5, 0.7, 0.75, 1.0], np.float32)
    return np.stack(np.meshgrid(a, a), -1).reshape(-1, 2)


def test_decode_oct_on_the_grid(sref, aref):
    e = _oct_grid()
    want = R.decode_oct(e)
    diamond = np.abs(e[:, 0]) + np.abs(e[:, 1])
    print("decodeOct: %d points, e.x == 0 at %d, e.y == 0 at %d, on the diamond %d, outside it (t > 0) %d" %
          (len(e), int((e[:, 0] == 0).sum()), int((e[:, 1] == 0).sum()), int((diamond == 1).sum()), int((diamond > 1).sum())))
    assert (e[:, 0] == 0).any() and (e[:, 1] == 0).any() and (diamond == 1).any() and (diamond > 1).any() and (diamond < 1).any()
    assert (want[:, 2] < 0).any() and (want[:, 2] > 0).any()
    _zero("decodeOct, shade_ref.c", same(_call(sref.libs["f32"], "sr_x_decode_oct", e, 3), want))
    _zero("decodeOct, visattr_ref.c", same(_call(aref.libs["f32"], "va_x_decode_oct", e, 3), want))


def test_encode_oct_on_the_grid(aref):
    e = _oct_grid()
    v = np.concatenate([R.decode_oct(e), np.zeros((1, 3), np.float32), np.array([[0.3, -0.4, 0.0], [-0.0, 0.0, -1.0], [0.0, 0.0, 1.0], [1.0, 0.0, -0.0]], np.float32),
                        np.stack([e[:, 0], e[:, 1], -e[:, 0] * e[:, 1]], -1)])
    want = R.encode_oct(v)
    print("encodeOct: %d vectors, v.z <= 0 at %d, v.z > 0 at %d, the zero vector gives %s" % (len(v), int((v[:, 2] <= 0).sum()), int((v[:, 2] > 0).sum()), want[len(e)]))
    assert (v[:, 2] < 0).any() and (v[:, 2] > 0).any() and (v[:, 2] == 0).any() and not v[len(e)].any()
    _zero("encodeOct, visattr_ref.c", same(_call(aref.libs["f32"], "va_x_encode_oct", v, 2), want))


def test_tonemap_at_its_corners(sref):
    below = np.nextafter(np.float32(0.004), np.float32(0))
    c = np.array([0.0, 0.004, below, 0.003, -1.0, np.nan, np.inf, -np.inf, 1e-3, 0.0041, 0.5, 1.0, 11.2, 1e30], np.float32)
    c = np.concatenate([c, np.random.default_rng(3).uniform(0, 4, 4081).astype(np.float32)])
    want = R.tonemap(c.reshape(-1, 3)).reshape(-1)
    print("tonemap: of 0 = %g, of 0.004 = %g, below it = %g, of NaN = %g, of inf = %g" % (want[0], want[1], want[2], want[5], want[6]))
    assert want[0] == want[1] == want[2] == want[5] == 0 and np.isnan(want[6])  # max(vec3(0), c - 0.004): a NaN becomes 0 (math.h:93)
    _zero("tonemap", same(_call(sref.libs["f32"], "sr_x_tonemap", c.reshape(-1, 1), 1).reshape(-1), want))


def test_gradient_noise_on_the_first_and_last_columns_of_a_1920_wide_image(sref):
    y = np.arange(1080, dtype=np.float32)
    px = np.concatenate([np.stack([np.full(1080, x, np.float32), y], -1) for x in (0.0, 1.0, 1918.0, 1919.0)])
    for name, uv in (("final: vec2(pos)", px), ("mesh.frag: gl_FragCoord.xy", px + np.float32(0.5))):
        want = R.gradient_noise(uv)
        print("gradientNoise, %s: %d pixels, in [%.4f, %.4f]" % (name, len(uv), want.min(), want.max()))
        assert 0 <= want.min() < 0.01 and 0.99 < want.max() < 1
        _zero("gradientNoise, " + name, same(_call(sref.libs["f32"], "sr_x_gradient_noise", uv, 1).reshape(-1), want))
    assert (R.gradient_noise(px) != R.gradient_noise(px + np.float32(0.5))).mean() > 0.99  # the half pixel is visible to the test


def test_srgb_curves_on_every_code(sref, aref):
    c = np.concatenate([np.arange(256, dtype=np.float32) / np.float32(255), np.arange(1024, dtype=np.float32) / np.float32(1023),
                        np.array([0.0, -0.0, -0.25, np.nan, np.inf, 2.5, 1e-40, 0.5], np.float32)])
    c = np.concatenate([c, np.zeros(-len(c) % 3, np.float32)])
    lin, srgb = R.fromsrgb(c.reshape(-1, 3)).reshape(-1), R.tosrgb(c.reshape(-1, 3)).reshape(-1)
    print("fromsrgb / tosrgb: %d values; of a negative %g / %g, of NaN %g / %g, of 0 %g / %g" % (len(c), lin[1282], srgb[1282], lin[1283], srgb[1283], lin[0], srgb[0]))
    assert np.isnan(lin[1282]) and np.isnan(lin[1283]) and lin[0] == 0 and lin[255] == 1
    _zero("fromsrgb", same(_call(sref.libs["f32"], "sr_x_fromsrgb", c.reshape(-1, 1), 1).reshape(-1), lin))
    _zero("tosrgb", same(_call(aref.libs["f32"], "va_x_tosrgb", c.reshape(-1, 1), 1).reshape(-1), srgb))
    c4 = np.concatenate([c, np.zeros(-len(c) % 4, np.float32)]).reshape(-1, 4)
    a, b = R.fromsrgb4(c4), R.tosrgb4(c4)  # the vec4 forms pass .w through (math.h:74-77, :84-87)
    assert same(a[:, 3], c4[:, 3]).all() and same(b[:, 3], c4[:, 3]).all()
    assert same(a[:, :3], R.fromsrgb(c4[:, :3])).all() and same(b[:, :3], R.tosrgb(c4[:, :3])).all()


# ---- shadowfill, shadowblur, final

def test_shadow_fill(sref):
    seen = dict(outside=0, at_width=0, owned=0)
    for w, h in SC.SIZES:
        i = SR.test_inputs(w, h)
        for cb in (0, 1):
            R.stats("shadowfill")
            words, handed = R.shadow_fill(i["shadow"], i["depth"], cb)
            st = R.stats("shadowfill")
            x, y = np.meshgrid(np.arange(w), np.arange(h))
            owned = (~(y ^ cb) & 1) == (x & 1)
            print("fill %dx%d cb %d: %d texels owned, %d fetches outside, %d stores dropped, %d of them at pos.x == width" %
                  (w, h, cb, int(owned.sum()), st["outside"], st["dropped"], st["dropped_at_width"]))
            assert (st["dropped_at_width"] > 0) == (w % 2 == 1 and (h > 1 or cb == 0)), "an odd width makes pos.x == width occur"
            assert st["outside"] > 0 and (words[~owned] == i["shadow"][~owned]).all()
            seen["outside"] += st["outside"]
            seen["at_width"] += st["dropped_at_width"]
            seen["owned"] += int(owned.sum())
            got, value = sref.shadow_fill(i["shadow"], i["depth"], cb, value=True)
            _zero("fill %dx%d cb %d, words" % (w, h, cb), got == words)
            _zero("fill %dx%d cb %d, values" % (w, h, cb), same(value[owned], handed[..., 0][owned]))
            assert not handed[..., 1:].any()
    assert seen["at_width"] > 0 and seen["outside"] > 0 and seen["owned"] > 2000


def test_shadow_blur(sref):
    seen = dict(near=0, far=0, outside=0, sky=0)
    for w, h in SC.SIZES:
        i = SR.test_inputs(w, h)
        with np.errstate(all="ignore"):
            d = np.float32(i["znear"]) / i["depth"]
        for direction in (1, 0):
            R.stats("shadowblur")
            words, handed = R.shadow_blur(i["shadow"], i["depth"], direction, i["znear"])
            st = R.stats("shadowblur")
            with np.errstate(all="ignore"):  # :42 over the neighbours inside the image
                step = np.abs(d[:, 1:] - d[:, :-1]) if direction else np.abs(d[1:] - d[:-1])
            near, far = int((step < np.float32(0.1)).sum()), int((~(step < np.float32(0.1))).sum())
            print("blur %dx%d direction %d: |depth - dnext| < 0.1 at %d neighbour pairs, not at %d; %d fetches outside; %d sky texels" %
                  (w, h, direction, near, far, st["outside"], int((i["depth"] == 0).sum())))
            assert st["outside"] > 0
            seen["near"], seen["far"], seen["outside"], seen["sky"] = seen["near"] + near, seen["far"] + far, seen["outside"] + st["outside"], seen["sky"] + int((i["depth"] == 0).sum())
            got, value = sref.shadow_blur(i["shadow"], i["depth"], direction, i["znear"], value=True)
            _zero("blur %dx%d direction %d, words" % (w, h, direction), got == words)
            _zero("blur %dx%d direction %d, values" % (w, h, direction), same(value, handed[..., 0]))
    assert seen["near"] > 1000 and seen["far"] > 100 and seen["sky"] > 100


def _final_conditions(name, i, words):
    g0, g1 = i["gbuffer0"], i["gbuffer1"]
    e = ((g1[..., None] >> np.array([0, 10], np.uint32)) & 1023).astype(np.float64) / 1023 * 2 - 1
    back = int((np.abs(e).sum(-1) > 1).sum())
    gloss, a = (g1 >> 20) & 1023, g0 >> 24
    sky = i["depth"] == 0
    c = dict(sky=int(sky.sum()), geometry=int((i["depth"] > 0).sum()), back=back, front=int(e[..., 0].size - back), gloss0=int((gloss == 0).sum()),
             gloss1=int((gloss == 1023).sum()), a0=int((a == 0).sum()), a255=int((a == 255).sum()))
    print("%s: %s" % (name, c))
    if sky.any():  # a sky pixel's view is NaN; max(vec3(0), NaN - 0.004) turns it into 0: the pixel is tonemap(0) + deband, at most code 1
        assert (SR.channels(words)[sky][:, :3] <= 1).all()
    return c


def test_final_with_an_all_zero_bloom_image(sref):
    total = {}
    for w, h in SC.SIZES:
        i = SR.test_inputs(w, h)
        for shadows in (0, 1):
            sd = SR.test_shade_data(w, h, shadows)
            words, handed = R.final(sd, i["gbuffer0"], i["gbuffer1"], i["depth"], i["shadow"] if shadows else None)
            for k, v in _final_conditions("final %dx%d shadows %d" % (w, h, shadows), i, words).items():
                total[k] = total.get(k, 0) + v
            got, value = sref.shade_final(sd, i["gbuffer0"], i["gbuffer1"], i["depth"], i["shadow"] if shadows else None, value=True)
            _zero("final %dx%d shadows %d, words" % (w, h, shadows), got == words)
            _zero("final %dx%d shadows %d, values" % (w, h, shadows), same(value[..., :3] + value[..., 3:], handed[..., :3]))
            assert (handed[..., 3] == 1).all()
    assert all(total[k] > 0 for k in total), total


def test_final_with_a_bloom_image(sref, bref):
    total = {}
    for w, h in SC.SIZES:
        i = SR.test_inputs(w, h)
        bloom0 = SC.bloom_levels(w, h, seed=4)[0]
        for shadows in (0, 1):
            sd = SR.test_shade_data(w, h, shadows)
            R.stats("final")
            words, handed = R.final(sd, i["gbuffer0"], i["gbuffer1"], i["depth"], i["shadow"] if shadows else None, bloom0)
            edges = R.stats("final")["edges"]
            for k, v in _final_conditions("final + bloom %dx%d shadows %d (taps clamped l/r/t/b %s)" % (w, h, shadows, edges.tolist()), i, words).items():
                total[k] = total.get(k, 0) + v
            assert w * h == 1 or (edges > 0).all()
            plain, _ = R.final(sd, i["gbuffer0"], i["gbuffer1"], i["depth"], i["shadow"] if shadows else None)
            assert w * h < 16 or (plain != words).any()  # the bloom term is visible
            got, value = bref.shade_final_bloom(sd, i["gbuffer0"], i["gbuffer1"], i["depth"], i["shadow"] if shadows else None, bloom0, value=True)
            _zero("final + bloom %dx%d shadows %d, words" % (w, h, shadows), got == words)
            _zero("final + bloom %dx%d shadows %d, values" % (w, h, shadows), same(value[..., :3] + value[..., 3:], handed[..., :3]))
    assert all(total[k] > 0 for k in total), total


# ---- bloom

def _specials(name, levels):
    c = BR.codes(np.concatenate([l.reshape(-1) for l in levels]))
    e, m = c[:, :2] >> 6, c[:, :2] & 63
    n = dict(inf=int(((e == 31) & (m == 0)).sum()), nan=int(((e == 31) & (m != 0)).sum()), denormal=int(((e == 0) & (m != 0)).sum()),
             largest=int(((e == 30) & (m == 63)).sum()))
    print("%s: R and G codes inf %d, NaN %d, denormal %d, the largest finite %d" % (name, n["inf"], n["nan"], n["denormal"], n["largest"]))
    return n


def test_bloom_passes_alone(bref):
    edges, shapes, spec = np.zeros(4, np.int64), set(), {}
    for w, h in SC.SIZES:
        i = SC.pass_inputs(w, h)
        d = i["desc"]
        shapes |= set(d["sizes"])
        R.stats("bloom")
        words, handed = R.bloom_pass(0, i["bloom_g0"], d["sizes"][0][::-1])
        got, value = bref.extract(i["bloom_g0"], value=True)
        _zero("extract %dx%d, words" % (w, h), got == words)
        _zero("extract %dx%d, values" % (w, h), same(value, handed[..., :3]))
        for k, v in _specials("given levels %dx%d" % (w, h), i["levels"] + i["levels2"]).items():
            spec[k] = spec.get(k, 0) + v
        for level in range(1, d["levels"]):
            words, handed = R.bloom_pass(1, i["levels"][level - 1], i["levels"][level].shape)
            got, value = bref.downsample(i["levels"][level - 1], value=True)
            _zero("downsample %dx%d into level %d, words" % (w, h, level), got == words)
            _zero("downsample %dx%d into level %d, values" % (w, h, level), same(value, handed[..., :3]))
        for radius in SC.RADII:
            for level in range(d["levels"] - 1):
                words, handed = R.bloom_pass(2, i["levels2"][level + 1], i["levels2"][level].shape, radius, dst=i["levels2"][level])
                got, value = bref.upsample(i["levels2"][level + 1], i["levels2"][level], radius, value=True)
                _zero("upsample %dx%d into level %d, radius %g, words" % (w, h, level, radius), got == words)
                _zero("upsample %dx%d into level %d, radius %g, values" % (w, h, level, radius), same(value, handed[..., :3]))
        e = R.stats("bloom")["edges"]
        print("bloom passes %dx%d: levels %s, taps clamped at the left / right / top / bottom edge %s" % (w, h, d["sizes"], e.tolist()))
        edges += e
    assert (edges > 0).all(), "the clamp is hit on all four edges"
    assert any(a % 2 == 1 for a, _ in shapes) and any(b % 2 == 1 for _, b in shapes) and any(a == 1 and b > 1 for a, b in shapes)
    assert all(v > 0 for v in spec.values()), spec
    assert max(SC.RADII) > 4 and 2.0 in SC.RADII


def test_bloom_loop(bref):
    for w, h in SC.SIZES:
        g0, d = BR.test_gbuffer0(w, h), BR.desc(w, h)
        want = R.bloom(g0, d["width"], d["height"], d["levels"], d["offsets"], d["total"])
        print("bloom loop %dx%d: %d levels, %d texels, %d of them non-zero" % (w, h, d["levels"], d["total"], int((want != 0).sum())))
        assert w * h < 16 or (want != 0).mean() > 0.5
        _zero("bloom loop %dx%d" % (w, h), BR.pack(bref.chain(g0)) == want)


# ---- mesh.frag

def _frag_compare(name, ref, want, shaded, alpha):
    """ref: oracle.ref.mesh_frag's dict; want: a restatement's output; alpha: albedo.a per pixel (the factor, times the tap's where sampled)"""
    _zero(name + ", gbuffer0", ref["gbuffer0"] == want["gbuffer0"])
    _zero(name + ", gbuffer1", ref["gbuffer1"] == want["gbuffer1"])
    _zero(name + ", channels before the pack", same(ref["written"][shaded], want["chan"][shaded]))
    a = SR.channels(ref["gbuffer0"])[shaded][:, 3]
    print("%s: %d shaded pixels, gbuffer0.a 0 at %d and 255 at %d, albedo.a < 0.5 at %d" % (name, int(shaded.sum()), int((a == 0).sum()), int((a == 255).sum()), int((alpha[shaded] < 0.5).sum())))
    return int((a == 0).sum()), int((a == 255).sum())


def test_mesh_frag_with_factor_only_materials(aref):
    a0 = a255 = discards = 0
    scenes = [SC.frag_scene(w, h, g)[:2] + ("attr %dx%d" % (w, h),) for g, (w, h) in enumerate([(67, 37), (65, 17), (21, 3)])]
    sp = PC.special_scene()
    scenes.append((sp, sp["records"], "special"))
    for s, rec, name in scenes:
        w, h = s["viewport"]
        import raster_ref as RR
        mats = SC.untextured(s["materials"])
        with np.errstate(all="ignore"):
            want = aref.attributes(RR.globals_for(s["cull"], (w, h)), rec, w, h, s["draws"], s["meshlets"], s["data"], s["vertices"], mats)
        shaded = (want["flags"] & VA.SHADED) != 0
        assert shaded.sum() > 0.5 * w * h and (w * h < 1000 or (~shaded).any())
        alpha = mats["diffuseFactor"][want["attributes"]["materialIndex"], 3]
        for post in (0, 1):
            ref = R.mesh_frag(want["attributes"], w, s["draws"], mats, None, post)
            a, b = _frag_compare("mesh.frag %s POST %d" % (name, post), ref, want, shaded, alpha)
            a0, a255 = a0 + a, a255 + b
            expect = shaded & (post > 0) & (alpha < np.float32(0.5))
            _zero("mesh.frag %s POST %d, discard" % (name, post), ref["discard"] == expect)
            discards += int(expect.sum())
    assert a0 > 0 and a255 > 0, "gbuffer0.a 0 and 255 occur"
    assert discards > 500


def test_mesh_frag_with_textured_materials(tref):
    files, descs, texels = SC.frag_textures()
    used = set()
    for group in range(6):
        s, rec = SC.frag_scene(64, 48, group)
        want = tref.attributes(s["g"], rec, 64, 48, s["draws"], s["meshlets"], s["data"], s["vertices"], s["materials"], descs, texels, taps=True)
        shaded = (want["flags"] & VA.SHADED) != 0
        assert shaded.sum() > 1500 and not (want["flags"] & TR.NOT_SAMPLED).any() and tref.bad_indices() == 0
        mi = want["attributes"]["materialIndex"]
        used |= set(np.unique(mi[shaded]).tolist())
        alpha = s["materials"]["diffuseFactor"][mi, 3] * np.where(s["materials"]["albedoTexture"][mi] > 0, want["taps"][:, 0, 3], np.float32(1))
        for post in (0, 1):
            ref = R.mesh_frag(want["attributes"], 64, s["draws"], s["materials"], want["taps"], post)
            _frag_compare("mesh.frag textured, materials %s, POST %d" % (s["draws"]["materialIndex"].tolist(), post), ref, want, shaded, alpha)
            _zero("discard", ref["discard"] == (shaded & (post > 0) & (alpha < np.float32(0.5))))
        plain = R.mesh_frag(want["attributes"], 64, s["draws"], SC.untextured(s["materials"]), None, 0)
        assert (plain["gbuffer0"] != want["gbuffer0"]).any() and (plain["gbuffer1"] != want["gbuffer1"]).any()  # the taps are visible
    print("textured materials shaded: %s" % sorted(used))
    assert used == set(range(16)), "each of the four slots on and off, in every combination"
