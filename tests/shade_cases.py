"""Case builders shared by tests/test_shading_vs_ref.py, tests/golden/generate.py (section `shade`) and the fixture replays (DESIGN.md §2,
§4.13-§4.15, §4.18): the inputs of the shading passes at one image size, from the existing fixed-seed builders.  No GPU, no test."""
import glob
import os

import numpy as np

import bloom_ref as BR
import pixel_cases as PC
import shade_ref as SR
import visattr_ref as VA
from niagara_amd import host, synth
from niagara_amd import layouts as L

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "shade")
SIZES = [(1, 1), (7, 5), (21, 3), (3, 21), (67, 37), (65, 17)]  # of tests/test_shade_gpu.py's list
FIXTURE_SIZES = [(21, 3), (67, 37), (65, 17)]
RADII = (2.0, 5.5)  # 5.5: above 4, the upsample kernel's unstaged form
# largest finite codes of the 11-bit and the 10-bit float, inf, NaN, the smallest and the largest denormal
SPECIAL_WORDS = np.array([(30 << 6 | 63) | (30 << 6 | 63) << 11 | (30 << 5 | 31) << 22, 31 << 6 | (31 << 6) << 11 | (31 << 5) << 22,
                          (31 << 6 | 32) | 1 << 11 | 1 << 22, 1 | 63 << 11 | 31 << 22, 63 | 1 << 11 | 1 << 22], np.uint32)


def same_bits(a, b):
    """elementwise: the same fp32 bits, a NaN matching a NaN whatever its sign or payload (as tests/test_shadow_alpha_cpu.py compares)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return (na & nb) | (~na & ~nb & (a.view(np.uint32) == b.view(np.uint32)))


def bloom_levels(w, h, seed=0):
    """bloom_ref.test_levels with SPECIAL_WORDS in every level that has room (inf, NaN, denormals, the largest finite code)"""
    levels = BR.test_levels(w, h, seed=seed)
    for l in levels:
        if l.size >= 16:
            l.reshape(-1)[3:3 + len(SPECIAL_WORDS)] = SPECIAL_WORDS
    return levels


def frag_materials():
    """16 materials: every combination of the four texture slots on and off (bit k of the index = slot k names texture k + 1), factors of
    visattr_ref.make_materials"""
    m = VA.make_materials(16)
    m["emissiveFactor"][7] = (30.0, 25.0, 40.0)  # log2(1 + emissivef) / 5 > 1: gbuffer0.a saturates
    for i in range(16):
        m[i]["albedoTexture"], m[i]["normalTexture"] = (1 if i & 1 else 0), (2 if i & 2 else 0)
        m[i]["specularTexture"], m[i]["emissiveTexture"] = (3 if i & 4 else 0), (4 if i & 8 else 0)
    return m


def frag_textures():
    """synth.with_textures' four maps (albedo, normal, specular, emissive = textures 1..4), decoded on the host: (files, descs, texels)"""
    files = [synth.dds_bytes(img) for img in synth.texture_images(64)]
    descs, texels = host.texture_decode_host(files)
    return files, descs, texels


def frag_scene(w, h, group):
    """pixel_cases.attr_scene under a w x h viewport, its three draws on materials 3 group .. 3 group + 2 (mod 16) of frag_materials, and
    pixel_cases.random_records: (scene with "g", records)"""
    import raster_ref as RR
    s = PC.attr_scene((w, h))
    s["materials"] = frag_materials()
    s["draws"] = s["draws"].copy()
    s["draws"]["materialIndex"] = (3 * group + np.arange(3)) % 16
    s["g"] = RR.globals_for(s["cull"], (w, h))
    return s, PC.random_records(s, w * h, 40 + group)


def untextured(materials):
    m = materials.copy()
    for k in ("albedoTexture", "normalTexture", "specularTexture", "emissiveTexture"):
        m[k] = 0
    return m


def pass_inputs(w, h):
    """everything the compute passes of one size read: shade_ref.test_inputs, ShadeData with shadows off and on, gbuffer0 of the bloom tests,
    given bloom levels (two seeds: pass 1 reads the first, pass 2 the second), the bloom descriptor"""
    i = SR.test_inputs(w, h)
    i["sd"] = [SR.test_shade_data(w, h, s) for s in (0, 1)]
    i["bloom_g0"] = BR.test_gbuffer0(w, h)
    i["levels"] = bloom_levels(w, h)
    i["levels2"] = bloom_levels(w, h, seed=2)
    i["desc"] = BR.desc(w, h)
    return i


# ---- the committed fixtures (tests/golden/shade/<w>x<h>.npz, written by tests/golden/generate.py from the reference's shaders)

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "*.npz")))
FIXTURE_IDS = [os.path.basename(p)[:-4] for p in FIXTURES]


def fixture_size(f):
    h, w = f["depth"].shape
    return w, h


def fixture_shade_data(f, shadows):
    return np.frombuffer(f["sd"][shadows].tobytes(), L.SHADEDATA).copy()


def fixture_frag_scene(path, f):
    """the scene the fixture's records belong to (frag_scene of the fixture's size and group), its material table, material indices and
    records taken from the fixture: (scene, records)"""
    w, h = fixture_size(f)
    s, _ = frag_scene(w, h, ["%dx%d.npz" % z for z in FIXTURE_SIZES].index(os.path.basename(path)))
    s["materials"] = np.ascontiguousarray(f["materials"]).astype(L.MATERIAL)
    s["draws"]["materialIndex"] = f["material_index"]
    return s, np.ascontiguousarray(f["records"]).astype(L.VISRECORD)
