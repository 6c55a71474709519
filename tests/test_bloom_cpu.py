"""Bloom without a GPU: NvBloomDesc's layout and nv_bloom_desc_init, the exported symbols, and the rule set as
tests/bloom_ref.c restates it — the UFLOAT decode and store (also as niagara_amd/csrc/bloommath.h states them, compiled for the host),
constant images through passes 1 and 2, an emission-free G-buffer, the fp32 build against the fp64 build, the footprint bounds of the
tiled kernels, and the condition check of tests/test_bloom_gpu.py: the restatement with every pow / exp2 result moved by 2 ULP stays inside
the GPU tests' conditions on the GPU tests' own inputs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bloom_ref as BR
import niagara_amd as N
import shade_ref as SR
from niagara_amd import _lib, host
from niagara_amd import layouts as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESC_SIZES = [(1, 1), (2, 2), (7, 5), (33, 3), (511, 9), (1920, 1080), (67, 37), (67, 67), (16384, 16384), (3, 16384)]
GPU_SIZES = [(1, 1), (2, 2), (7, 5), (33, 3), (67, 37), (511, 9), (67, 67)]  # tests/test_bloom_gpu.py's


@pytest.fixture(scope="session")
def bref(tmp_path_factory):
    return BR.load(tmp_path_factory.mktemp("bloom_ref_cpu"))


@pytest.fixture(scope="session")
def sref(tmp_path_factory):
    return SR.load(tmp_path_factory.mktemp("shade_ref_bloom_cpu"))


def test_bloom_desc_layout_matches_the_header(tmp_path):
    fields = list(L.BLOOMDESC.names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "niagara_vis.h"\nint main(void){printf("%zu", sizeof(NvBloomDesc));\n' +
                   "".join('printf(" %%zu", offsetof(NvBloomDesc, %s));\n' % f for f in fields) + 'printf(" %d", NV_BLOOM_MAX_LEVELS);return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == L.BLOOMDESC.itemsize == C.sizeof(_lib.BloomDesc) == 48
    assert got[1:-1] == [L.BLOOMDESC.fields[f][1] for f in fields] == [getattr(_lib.BloomDesc, f).offset for f in fields]
    assert got[-1] == L.BLOOM_MAX_LEVELS == BR.MAX_LEVELS == 8


def test_library_exports_the_bloom_entry_points():
    for name in ("nv_bloom_desc_init", "nv_bloom_extract", "nv_bloom_downsample", "nv_bloom_upsample", "nv_bloom", "nv_shade_final_bloom"):
        assert name in N.EXPORTS and hasattr(N.lib, name), name
    d = host.bloom_desc(8, 8)
    assert N.lib.nv_bloom_extract(None, None, None, 8, 8, None, C.byref(d)) == -1
    assert N.lib.nv_bloom_downsample(None, None, None, C.byref(d), 1) == -1
    assert N.lib.nv_bloom_upsample(None, None, None, C.byref(d), 0, 2.0) == -1
    assert N.lib.nv_bloom(None, None, None, 8, 8, None, C.byref(d)) == -1
    assert N.lib.nv_shade_final_bloom(None, None, None, None, None, None, None, None, 8, 8, None, C.byref(d)) == -1
    for w, h in ((0, 4), (4, 0), (16385, 4), (4, 16385)):
        assert N.lib.nv_bloom_desc_init(C.byref(d), w, h) == -1
    assert N.lib.nv_bloom_desc_init(None, 4, 4) == -1
    from niagara_amd import pipeline as P
    header = open(os.path.join(ROOT, "include", "niagara_vis.h")).read()
    assert "#define NV_OPT_BLOOM_FUSED_TAIL 12\n" in header and P.NV_OPT_BLOOM_FUSED_TAIL == 12
    assert N.lib.nv_set_option(None, P.NV_OPT_BLOOM_FUSED_TAIL, 1) == -1


@pytest.mark.parametrize("size", DESC_SIZES)
def test_bloom_desc_init_follows_the_formulas(size):
    w, h = size
    d, want = host.bloom_desc(w, h), BR.desc(w, h)
    assert (d.width, d.height, d.levels, list(d.levelOffset), d.totalTexels) == (want["width"], want["height"], want["levels"], want["offsets"], want["total"])
    assert d.width == (w + 1) // 2 and d.height == (h + 1) // 2 and d.levels == min(8, host.image_mip_levels(d.width, d.height))
    if size == (33, 3):  # one axis reaches 1 before the other
        assert want["sizes"] == [(17, 2), (8, 1), (4, 1), (2, 1), (1, 1)]
    if size == (511, 9):  # the 8-level cap
        assert want["width"] == 256 and want["levels"] == 8 and host.image_mip_levels(256, 5) == 9 and want["sizes"][-1] == (2, 1)
    if size == (1920, 1080):
        assert want["levels"] == 8 and want["sizes"][0] == (960, 540) and want["sizes"][7] == (7, 4)


# ---- the UFLOAT formats

def _value(code, mbits):
    """the value of a code by the format's definition, in Python floats (exact)"""
    e, m = code >> mbits, code & ((1 << mbits) - 1)
    if e == 0:
        return m * 2.0 ** (-14 - mbits)
    if e == 31:
        return np.inf if m == 0 else np.nan
    return (1.0 + m / float(1 << mbits)) * 2.0 ** (e - 15)


@pytest.mark.parametrize("mbits", [6, 5])
def test_decode_is_exact_and_every_code_round_trips(mbits, bref):
    codes = np.arange(1 << (mbits + 5), dtype=np.uint32)
    want = np.array([_value(int(c), mbits) for c in codes])
    for real in ("f32", "f64"):
        got = bref.decode(codes, mbits, real)
        nan = np.isnan(want)
        assert (np.isnan(got) == nan).all() and (got[~nan].astype(np.float64) == want[~nan]).all()
        back = bref.encode(got, mbits, real)
        canon = np.where(nan, 31 << mbits | 1 << (mbits - 1), codes)  # every NaN code stores as the one NaN code
        assert (back == canon).all()
    assert _value((31 << 6) - 1, 6) == 65024.0 and _value((31 << 5) - 1, 5) == 64512.0


@pytest.mark.parametrize("mbits", [6, 5])
def test_store_truncates_clamps_and_drops_the_sign(mbits, bref):
    top, nan_code, inf_code = (31 << mbits) - 1, 31 << mbits | 1 << (mbits - 1), 31 << mbits
    codes = np.arange(top, dtype=np.uint32)  # every finite code but the largest
    lo, hi = bref.decode(codes, mbits, "f64"), bref.decode(codes + 1, mbits, "f64")
    for real, eps in (("f32", np.float32), ("f64", np.float64)):
        below = np.nextafter(hi.astype(eps), eps(0))  # the largest value below the next code: still this code (round toward zero)
        mid = ((lo + hi) / 2).astype(eps)
        for v in (lo.astype(eps), mid, below):
            assert (bref.encode(v, mbits, real) == codes).all()
        biggest = float(_value(top, mbits))
        cases = [(biggest, top), (np.nextafter(eps(biggest), eps(np.inf)), top), (65535.9, top), (65536.0, top), (1e30, top), (np.finfo(eps).max, top),
                 (np.inf, inf_code), (-np.inf, 0), (np.nan, nan_code), (0.0, 0), (-0.0, 0), (-1.0, 0), (-1e-30, 0), (-65536.0, 0),
                 (2.0 ** (-14 - mbits), 1), (np.nextafter(eps(2.0 ** (-14 - mbits)), eps(0)), 0), (1e-30, 0), (np.finfo(eps).tiny, 0),
                 (2.0 ** -14, 1 << mbits), (np.nextafter(eps(2.0 ** -14), eps(0)), (1 << mbits) - 1), (3 * 2.0 ** (-14 - mbits), 3), (3.5 * 2.0 ** (-14 - mbits), 3)]
        got = bref.encode(np.array([c[0] for c in cases], eps), mbits, real)
        assert got.tolist() == [c[1] for c in cases], (real, got.tolist())
        neg_nan = np.array([np.nan], eps)
        neg_nan.view(np.uint32 if eps is np.float32 else np.uint64)[0] |= (1 << 31) if eps is np.float32 else (1 << 63)
        assert bref.encode(neg_nan, mbits, real)[0] == nan_code  # a NaN is a NaN whatever its sign bit (inf * 0 has it set on x86, clear on the device)


HOST_CHECK = r'''
#include <stdio.h>
#include <stdlib.h>
#include "bloommath.h"
using namespace nv;
// argv[1]: floats in, argv[2]: codes out (6-bit then 5-bit per float, then the decode of every code); stdout: the footprint extents
int main(int argc, char** argv)
{
	FILE* in = fopen(argv[1], "rb");
	fseek(in, 0, SEEK_END);
	long n = ftell(in) / 4;
	fseek(in, 0, SEEK_SET);
	float* v = (float*)malloc(n * 4);
	if (fread(v, 4, n, in) != (size_t)n) return 1;
	FILE* out = fopen(argv[2], "wb");
	for (long i = 0; i < n; ++i) { uint32_t c[2] = { bl_encode<6>(v[i]), bl_encode<5>(v[i]) }; fwrite(c, 4, 2, out); }
	for (uint32_t c = 0; c < 2048; ++c) { float f = bl_decode<6>(c); fwrite(&f, 4, 1, out); }
	for (uint32_t c = 0; c < 1024; ++c) { float f = bl_decode<5>(c); fwrite(&f, 4, 1, out); }
	fclose(out);
	// pass 1: every tile of every level width w (source W = 2 w or 2 w + 1, or 1 x 1 -> 1 x 1): last i1 - first i0 + 1
	int down = 0, up = 0;
	for (uint32_t w = 1; w <= 8192; ++w)
		for (uint32_t W = (w == 1 ? 1 : 2 * w); W <= 2 * w + 1 && W <= 16384; ++W)
		{
			const float fw = (float)w, fW = (float)W, tx = 1.0f / fw;
			for (uint32_t t = 0; t < w; t += BL_TILE)
			{
				const uint32_t last = t + BL_TILE - 1 < w - 1 ? t + BL_TILE - 1 : w - 1;
				const int e = bl_axis(bl_coord(last, fw, tx, 1.0f), fW).i1 - bl_axis(bl_coord(t, fw, tx, -1.0f), fW).i0 + 1;
				down = e > down ? e : down;
			}
		}
	// pass 2, staged: every tile of every level width w (source W = max(1, w / 2)) at radii up to BL_UP_STAGED_RADIUS
	const float radii[] = { 0.0f, 0.5f, 1.0f, 2.0f, 3.999f, BL_UP_STAGED_RADIUS };
	for (uint32_t w = 1; w <= 8192; ++w)
		for (float radius : radii)
		{
			const uint32_t W = w / 2 ? w / 2 : 1;
			const float fw = (float)w, fW = (float)W, rx = (1.0f / fw) * radius;
			for (uint32_t t = 0; t < w; t += BL_TILE)
			{
				const uint32_t last = t + BL_TILE - 1 < w - 1 ? t + BL_TILE - 1 : w - 1;
				const int e = bl_axis(bl_coord(last, fw, rx, 1.0f), fW).i1 - bl_axis(bl_coord(t, fw, rx, -1.0f), fW).i0 + 1;
				up = e > up ? e : up;
			}
		}
	printf("%d %d %d %d\n", down, BL_DOWN_SIDE, up, BL_UP_SIDE);
	return 0;
}
'''


def test_the_kernels_header_states_the_same_formats_and_its_tiles_hold_their_footprints(tmp_path, bref):
    """niagara_amd/csrc/bloommath.h compiled for the host: its store (integer arithmetic on the float's bits) against the restatement's
    (frexp and floor on the value) over every code's value, its neighbours, every exponent and random bit patterns; its decode of every
    code; and the widest footprint of any tile of passes 1 and 2 against the staged side"""
    src = tmp_path / "check.cpp"
    src.write_text(HOST_CHECK)
    exe = tmp_path / "check"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "niagara_amd", "csrc"), str(src), "-o", str(exe)])
    rng = np.random.default_rng(15)
    exact = np.concatenate([bref.decode(np.arange(2048, dtype=np.uint32), 6), bref.decode(np.arange(1024, dtype=np.uint32), 5)])
    exact = exact[np.isfinite(exact)]
    bits = np.concatenate([exact.view(np.uint32), exact.view(np.uint32) - 1, exact.view(np.uint32) + 1,
                           (np.arange(256, dtype=np.uint32) << 23), (np.arange(256, dtype=np.uint32) << 23) | 0x7FFFFF, (np.arange(256, dtype=np.uint32) << 23) | 1,
                           rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32),
                           (rng.integers(0x33000000, 0x48000000, 200000, dtype=np.uint64)).astype(np.uint32),  # 2^-25 .. 2^17: the formats' range
                           np.array([0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 1, 0x007FFFFF], np.uint32)])
    values = bits.astype(np.uint32).view(np.float32)
    values.tofile(str(tmp_path / "in.bin"))
    extents = [int(v) for v in subprocess.check_output([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")]).split()]
    raw = np.fromfile(str(tmp_path / "out.bin"), np.uint32)
    enc = raw[:2 * values.size].reshape(-1, 2)
    assert (enc[:, 0] == bref.encode(values, 6)).all() and (enc[:, 1] == bref.encode(values, 5)).all()
    dec = raw[2 * values.size:]
    assert dec.size == 2048 + 1024
    want = np.concatenate([bref.decode(np.arange(2048, dtype=np.uint32), 6), bref.decode(np.arange(1024, dtype=np.uint32), 5)])
    nan = np.isnan(want)
    assert (np.isnan(dec.view(np.float32)) == nan).all() and (dec[~nan] == want.view(np.uint32)[~nan]).all()
    print("widest footprint: pass 1 %d of %d staged, pass 2 %d of %d staged" % tuple(extents))
    assert extents[0] <= extents[1] and extents[2] <= extents[3]


# ---- the passes

def _constant(shape, r, g, b, bref):
    word = int(bref.encode([r], 6)[0]) | int(bref.encode([g], 6)[0]) << 11 | int(bref.encode([b], 5)[0]) << 22
    assert bref.decode([word & 2047], 6)[0] == r and bref.decode([word >> 22], 5)[0] == b
    return np.full(shape, word, np.uint32)


def test_constant_images_pass_through_both_passes(bref):
    """the 13 weights of pass 1 and the 9 of pass 2 each sum to 1 exactly; with power-of-two sizes every coordinate is exact (alpha is 0.5 in
    pass 1, 0.25 / 0.75 in pass 2), so a constant image with few mantissa bits comes back as itself, and pass 2 gives existing + constant"""
    assert 0.125 + 4 * (0.5 / 4) + 4 * (0.125 / 4) + 4 * (0.125 / 2) == 1.0 and 4 / 16 + 4 * (2 / 16) + 4 * (1 / 16) == 1.0
    for real in ("f32", "f64"):
        for shape in ((16, 32), (8, 16), (2, 4), (1, 2), (1, 1)):
            src = _constant(shape, 1.5, 0.375, 20.0, bref)
            down = bref.downsample(src, real)
            assert down.shape == (max(1, shape[0] >> 1), max(1, shape[1] >> 1)) and (down == src.flat[0]).all(), (real, shape)
            dst = _constant((shape[0] * 2, shape[1] * 2), 1.0, 2.0, 4.0, bref)
            up = bref.upsample(src, dst, 2.0, real)
            assert (up == _constant(dst.shape, 2.5, 2.375, 24.0, bref)).all(), (real, shape)
            assert (bref.upsample(src, dst, 0.0, real) == up).all()  # radius 0: nine samples of one point


def test_no_emission_gives_an_all_zero_chain_and_final_without_bloom(bref, sref):
    w, h = 67, 37
    i = SR.test_inputs(w, h)
    g0 = i["gbuffer0"] & np.uint32(0x00FFFFFF)  # gbuffer0.a == 0: exp2(0) - 1 == 0
    for real in ("f32", "f64"):
        chain = bref.chain(g0, real)
        assert len(chain) == BR.desc(w, h)["levels"] and all((l == 0).all() for l in chain)
    for shadows in (0, 1):
        sd = SR.test_shade_data(w, h, shadows)
        shadow = i["shadow"] if shadows else None
        for real in ("f32", "f64"):
            for g in (g0, i["gbuffer0"]):  # a zero bloom image adds + 0 * 0.1, whatever the pixel's own emission
                got = bref.shade_final_bloom(sd, g, i["gbuffer1"], i["depth"], shadow, np.zeros(((h + 1) // 2, (w + 1) // 2), np.uint32), real)
                assert got.tobytes() == sref.shade_final(sd, g, i["gbuffer1"], i["depth"], shadow, real).tobytes()


@pytest.mark.parametrize("size", [(67, 37), (511, 9), (130, 70)])
def test_fp32_build_stays_within_one_code_of_the_fp64_build(size, bref):
    w, h = size
    g0 = BR.test_gbuffer0(w, h)
    a, b = BR.codes(bref.extract(g0, "f32")), BR.codes(bref.extract(g0, "f64"))
    d = np.abs(a - b)
    print("pass 0 %dx%d: %d channels, %.4f %% differ, largest difference %d" % (w, h, d.size, 100.0 * (d != 0).mean(), int(d.max())))
    assert d.max() <= 1
    c32, c64 = bref.chain(g0, "f32"), bref.chain(g0, "f64")
    d = np.concatenate([np.abs(BR.codes(x) - BR.codes(y)).reshape(-1) for x, y in zip(c32, c64)])
    print("chain %dx%d: %d channels, %.4f %% differ, largest difference %d" % (w, h, d.size, 100.0 * (d != 0).mean(), int(d.max())))
    assert d.max() <= 1


def bloom0_input(w, h):
    """level 0 of the bloom target that the final-with-bloom tests give: moderate values (up to 8), zeros, denormals, two inf and two NaN codes"""
    return BR.test_levels(w, h, seed=1, top=17)[0]


bloom0_input.__test__ = False


def test_perturbed_pow_and_exp2_stay_inside_the_gpu_tests_conditions(bref):
    """tests/test_bloom_gpu.py asks pass 0 for the same or the adjacent code with 99 % equal, and final with bloom for one 8-bit code with 90 %
    equal (§4.14's): moving every pow / exp2 result of the restatement by 2 ULP, up, down or mixed, on those tests' own inputs stays inside"""
    try:
        for w, h in GPU_SIZES:
            g0 = BR.test_gbuffer0(w, h)
            i = SR.test_inputs(w, h)
            b0 = bloom0_input(w, h)
            sds = [SR.test_shade_data(w, h, s) for s in (0, 1)]
            run = lambda: (BR.codes(bref.extract(g0)),
                           [SR.channels(bref.shade_final_bloom(sd, i["gbuffer0"], i["gbuffer1"], i["depth"], i["shadow"], b0)) for sd in sds])
            base = run()
            for mode in (1, 2, 3):
                bref.perturb(mode, 2)
                got = run()
                bref.perturb(0)
                d = np.abs(got[0] - base[0])
                assert d.max() <= 1 and (d == 0).mean() >= 0.99, (w, h, mode, float((d == 0).mean()))
                for g, b in zip(got[1], base[1]):
                    d = np.abs(g - b)
                    assert d.max() <= 1 and (d == 0).mean() >= 0.9, (w, h, mode, float((d == 0).mean()))
    finally:
        bref.perturb(0)
