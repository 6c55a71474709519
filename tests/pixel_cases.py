"""Case builders of tests/test_pixel_passes_cpu.py and tests/test_pixel_passes_gpu.py: the image sizes at which
the persistent per-pixel kernels take a second trip of their grid-stride loop, hand-made record and word images for the run detection of
nv_visibility_attributes and nv_visibility_resolve, and one scene of degenerate triangles and special values.  No GPU, no test: the CPU
file states over these cases the conditions that keep a green GPU run from being vacuous."""
import numpy as np

import raster_ref as RR
import visattr_ref as VA
import visbuffer_ref as VB
from niagara_amd import layouts as L

# ---- 1. the second trip
#
# The per-pixel kernels launch min(ceil(n / 256), persistent_grid(ctx, 8)) workgroups of 256 threads; persistent_grid is numCUs * 8
# (niagara_amd/csrc/context.hip, persistent_grid; numCUs = hipDeviceProp_t::multiProcessorCount there, what
# torch.cuda.get_device_properties(...).multi_processor_count reads).  One trip of `for (i = first; i < n; i += stride)` covers
# trip_items(numCUs) work items.  context.hip names this file at persistent_grid: the two move together.
THREADS = 256
BLOCKS_PER_CU = 8
NONE = 0xFFFFFFFF


def trip_items(cus):
    return int(cus) * BLOCKS_PER_CU * THREADS


def second_trip_sizes(cus):
    """name -> (width, height, work items of the launch).  2051 = 2048 + 3 columns and cus + 1 rows: 2051 (cus + 1) = trip_items(cus) +
    3 cus + 2051 items, at 256 CUs 44 waves and 3 lanes into the second trip (a multiple of 64 only when cus % 64 == 63)"""
    c1 = int(cus) + 1
    return dict(pixel=(2051, c1, 2051 * c1),                                      # resolve, attributes, final: one item per pixel
                fill=(2051, 2 * c1, 1026 * 2 * c1),                               # one item per pair of columns; the odd width drops stores
                extract=(4102, 2 * c1, 2051 * c1),                                # one item per texel of level 0, 2051 x (cus + 1)
                depth_aligned=(2051, 4 * c1 + 1, 2051 * (4 * c1 + 1) // 4),       # n4 16-byte groups, n % 4 == 3
                vis_aligned=(2051, 2 * c1 + 1, 2051 * (2 * c1 + 1) // 2))         # n2 pairs of words, n odd


def check_second_trip(items, width, height, cus):
    """the non-vacuity condition of every second-trip test; returns the trip size"""
    g = trip_items(cus)
    assert items > g, "no second trip: %d items, one trip covers %d" % (items, g)
    assert (items - g) % 64 != 0, "the second trip ends on a whole wave"
    assert 0 < width <= 16384 and 0 < height <= 16384
    return g


def encode_words(depth_bits, mvi, triangle):
    """visbuffer_ref.encode over arrays"""
    d, m, t = (np.asarray(a).astype(np.uint64) for a in (depth_bits, mvi, triangle))
    return (d << np.uint64(VB.SHIFT)) | (((m << np.uint64(7)) | t) + np.uint64(1))


def lod_scene():
    import test_visbuffer_cpu as TC
    s = TC._lod_scene()
    s["mvb_words"] = TC._mvb_words(s["draws"], s["meshes"])
    return s


def resolve_words(draws, n, seed=9):
    """test_resolve_marks_hand_made_words_unresolved's words for n pixels: runs of 7 equal clusters, some past the scene's slots, triangles up
    to 99 (>= 96: unresolved), 20 % empty, and three words no rasteriser writes"""
    rng = np.random.default_rng(seed)
    slots = int(draws["meshletVisibilityOffset"][-1])
    mvi = rng.integers(0, slots + 40, n)
    mvi = np.repeat(mvi[::7], 7)[:n]
    tri = rng.integers(0, 100, n)
    words = encode_words(rng.integers(0, 0x3F800001, n), mvi, tri)
    words[rng.random(n) < 0.2] = 0
    words[5], words[6], words[7] = 9 << VB.SHIFT, VB.encode(3, VB.MVI_END - 1, 0), VB.encode(0x3F800000, 0, 0)
    return words


# ---- the scene of the attribute cases

def attr_scene(viewport):
    """A grid of 9 x 9 vertices, 128 triangles (raster_ref.mesh_scene cuts it into two meshlets), under three draws of different position,
    orientation, scale and material, attributes from visattr_ref.fill_attributes, visattr_ref.make_materials (entry 2 names textures)"""
    k = np.arange(9)
    x, y = np.meshgrid(k, k)
    x, y = x.reshape(-1) / 8.0 - 0.5, y.reshape(-1) / 8.0 - 0.5
    pos = np.stack([x, y, 0.15 * np.sin(3.0 * x) * np.cos(2.0 * y)], -1)
    tris = []
    for j in range(8):
        for i in range(8):
            a = j * 9 + i
            tris += [(a, a + 1, a + 10), (a, a + 10, a + 9)]
    draws = np.zeros(3, L.MESHDRAW)
    draws["position"] = [(-0.6, 0.2, -4.0), (0.5, -0.3, -5.5), (0.1, 0.4, -7.0)]
    draws["scale"] = (2.0, 3.0, 1.25)
    q = np.array([(0.0, 0.0, 0.0, 1.0), (0.3, -0.2, 0.1, 0.9), (-0.1, 0.6, 0.2, 0.7)])
    draws["orientation"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    draws["materialIndex"] = (3, 0, 2)
    s = RR.mesh_scene(pos, tris, viewport, draws=draws)
    s["vertices"] = VA.fill_attributes(s["vertices"], s["meshlets"], s["data"])
    s["materials"] = VA.make_materials()
    assert len(s["meshlets"]) >= 2 and int(s["meshlets"]["triangleCount"].sum()) == 128
    return s


def _records(keys, rng):
    """VISRECORD records of (n, 3) keys: a random depth word under every named key, no sample = (~0, 0, 0, 0), unresolved = all ones"""
    keys = np.asarray(keys, np.uint32).reshape(-1, 3)
    r = np.zeros(len(keys), L.VISRECORD)
    r["drawId"], r["meshletIndex"], r["triangle"] = keys[:, 0], keys[:, 1], keys[:, 2]
    r["depthBits"] = rng.integers(1, 0x3F800001, len(keys))
    blank = keys[:, 0] == NONE
    r["depthBits"][blank] = np.where(keys[blank, 1] == NONE, NONE, 0)
    return r


NO_SAMPLE, UNRESOLVED = (NONE, 0, 0), (NONE, NONE, NONE)
assert VB.NO_SAMPLE[:3] == NO_SAMPLE and VB.UNRESOLVED[:3] == UNRESOLVED


def all_valid_keys(s):
    return np.array([(d, m, t) for d in range(len(s["draws"])) for m in range(len(s["meshlets"])) for t in range(int(s["meshlets"]["triangleCount"][m]))],
                    np.uint32)


def random_records(s, n, seed):
    """the second-trip records: runs of random length 1 .. 9, each of a random valid key of the scene, about 10 % of them no sample"""
    rng = np.random.default_rng(seed)
    keys = all_valid_keys(s)
    runs = n // 2 + 1  # (mean length 5: enough)
    length = rng.integers(1, 10, runs)
    pick = keys[rng.integers(0, len(keys), runs)]
    pick[rng.random(runs) < 0.1] = NO_SAMPLE
    per_pixel = np.repeat(pick, length, axis=0)[:n]
    assert len(per_pixel) == n
    return _records(per_pixel, rng)


# ---- 2. run edges

BOUNDARIES = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 62, 63)
ROW_EDGES = (16, 32, 48)  # the first lanes of the DPP rows of a wave


def key_set(s):
    """(valid keys, invalid keys): a dozen valid keys with (0, 0, 0) and neighbours one word apart; triangle == triangleCount and
    drawId == drawCount"""
    tc = s["meshlets"]["triangleCount"].astype(int)
    valid = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 5), (2, 0, 5), (1, 1, 5), (1, 0, 6), (2, 1, 5), (1, 0, 31), (2, 1, int(tc[1]) - 1),
             (0, 0, int(tc[0]) - 1)]
    invalid = [(0, 0, int(tc[0])), (len(s["draws"]), 0, 0)]
    assert all(d < len(s["draws"]) and m < len(tc) and t < tc[m] for d, m, t in valid) and len(set(valid)) == len(valid)
    return valid, invalid


# pairs of valid keys that differ in exactly one word: drawId, meshletIndex, triangle
ONE_WORD = (((1, 0, 5), (2, 0, 5)), ((1, 0, 5), (1, 1, 5)), ((1, 0, 5), (1, 0, 6)))
TO_ZERO = ((1, 0, 0), (0, 1, 0), (0, 0, 1))  # one word from (0, 0, 0), each word in turn


def _image(name, keys, width, rng, invalid=False):
    keys = np.asarray(keys, np.uint32).reshape(-1, 3)
    assert len(keys) % width == 0
    return dict(name=name, records=_records(keys, rng), width=width, height=len(keys) // width, invalid=invalid)


def _boundary_rows(a, b):
    return [a if lane < at else b for at in BOUNDARIES for lane in range(64)]


def run_edge_cases(s):
    """group -> list of images (dict: name, records, width, height, invalid: the image holds invalid keys).  Images are 64 wide, a row is a
    wave and the column the lane, but for group "d", one row of 256 + 64 + r pixels."""
    valid, invalid = key_set(s)
    rng = np.random.default_rng(77)
    out = dict(a=[], b=[], c=[], d=[], e=[])
    # a. every lane starts a run
    for cycle in ((valid[4], valid[5]), (valid[0], valid[8], valid[3])):
        out["a"].append(_image("alternating %d" % len(cycle), [cycle[i % len(cycle)] for i in range(64 * 4)], 64, rng))
    # b. consecutive runs one word apart, lengths 1, 2, 3; the sequence is no multiple of 64 long, so its repeats drift across the lanes
    seq = []
    for n in (1, 2, 3):
        for p, q in ONE_WORD:
            seq += [p] * n + [q] * n
        seq += [NO_SAMPLE] * n + [(0, 0, 0)] * n + [NO_SAMPLE] * n
    assert len(seq) % 64 not in (0, 32)
    flat = seq * 21
    flat += [NO_SAMPLE] * (-len(flat) % 64)
    out["b"].append(_image("one word apart", flat, 64, rng))
    # c. a boundary at every listed lane
    pairs = [("valid", valid[8], valid[9])] + [("one word %d" % k, p, q) for k, (p, q) in enumerate(ONE_WORD)]
    pairs += [("to zero", valid[8], (0, 0, 0))] + [("to zero, word %d" % k, p, (0, 0, 0)) for k, p in enumerate(TO_ZERO)]
    pairs += [("no sample to zero", NO_SAMPLE, (0, 0, 0)), ("unresolved to zero", UNRESOLVED, (0, 0, 0))]
    for k, bad in enumerate(invalid):
        pairs += [("invalid %d to valid" % k, bad, valid[4]), ("valid to invalid %d" % k, valid[4], bad), ("invalid %d to zero" % k, bad, (0, 0, 0))]
    for name, a, b in pairs:
        out["c"].append(_image("boundary, " + name, _boundary_rows(a, b), 64, rng, invalid="invalid" in name))
    # d. one run over three waves, a workgroup edge and a ragged last wave; record 320 is the one the lanes past n load
    for r in (1, 63):
        n = 256 + 64 + r
        for name, k320 in (("the run's key", valid[8]), ("another key", valid[9]), ("no sample", NO_SAMPLE)):
            keys = [valid[8]] * n
            keys[320] = k320
            out["d"].append(_image("across waves, %d pixels, %s at 320" % (n, name), keys, n, rng))
    # e. random runs of geometric length (mean 3) over the whole key set
    whole = valid + invalid + [NO_SAMPLE, UNRESOLVED]
    for seed in range(4):
        g = np.random.default_rng(500 + seed)
        n = 67 * 37
        length = g.geometric(1.0 / 3.0, n)
        keys = np.repeat(np.array(whole, np.uint32)[g.integers(0, len(whole), n)], length, axis=0)[:n]
        out["e"].append(_image("random %d" % seed, keys, 67, g, invalid=True))
    return out


def run_starts(image):
    """per pixel of an image: (lane, starts a run, the words in which its key differs from its predecessor's as a bit mask, named, the key).
    A wave is 64 consecutive pixels of the flat image (the kernel's stride is a multiple of 64), so the lane is i % 64"""
    r = image["records"]
    key = np.stack([r["drawId"], r["meshletIndex"], r["triangle"]], -1)
    lane = np.arange(len(r)) % 64
    diff = np.zeros(len(r), np.int64)
    diff[1:] = ((key[1:] != key[:-1]) * np.array([1, 2, 4])).sum(axis=1)
    start = (lane == 0) | (diff != 0)
    return lane, start, diff, key[:, 0] != NONE, key


# ---- the run edges of the resolve

def resolve_edge_words(s):
    """name -> (words, width, height) over test_visbuffer_cpu._lod_scene: (c)'s boundaries with B = mvi 0 after another cluster and after
    an empty word; runs of one mvi whose first pixel has triangle >= 96 and whose other pixels are resolved"""
    draws, meshes = s["draws"], s["meshes"]
    has = meshes["lods"]["meshletCount"][draws["meshIndex"], 0] > 1
    assert has[0] and int(draws["meshletVisibilityOffset"][0]) == 0
    other = int(draws["meshletVisibilityOffset"][np.nonzero(has)[0][7]]) + 1
    rng = np.random.default_rng(78)
    out = {}
    for name, a in (("after another cluster", other), ("after an empty word", None)):
        lanes = np.tile(np.arange(64), len(BOUNDARIES))
        first = lanes < np.repeat(BOUNDARIES, 64)
        n = len(lanes)
        words = encode_words(rng.integers(1, 0x3F800001, n), np.where(first, other, 0), rng.integers(0, 96, n))
        if a is None:
            words[first] = 0
        out["boundary " + name] = (words, 64, len(BOUNDARIES))
    n = 64 * 8
    length = rng.integers(2, 10, n)
    owners = np.nonzero(has)[0]
    mvi_run = draws["meshletVisibilityOffset"][owners[rng.integers(0, len(owners), n)]].astype(np.int64) + rng.integers(0, 2, n)
    mvi = np.repeat(mvi_run, length)[:n]
    head = np.zeros(n, bool)
    head[np.cumsum(length)[np.cumsum(length) < n]] = True
    head[0] = True
    tri = np.where(head, rng.integers(96, 128, n), rng.integers(0, 96, n))
    out["unresolved first lane"] = (encode_words(rng.integers(1, 0x3F800001, n), mvi, tri), 64, 8)
    return out


# ---- 3. degenerate triangles and special values

def _h(x):
    return int(np.array(x, np.float32).astype(np.float16).view(np.uint16))


H_NAN, H_INF, H_NINF, H_DENORMAL, H_NZERO = 0x7E00, 0x7C00, 0xFC00, 0x0001, 0x8000

# the triangles, three mesh-local positions each (draw 0 puts the mesh at z = -5 unrotated and unscaled, the camera looks down -z from the origin)
SPECIAL_TRIANGLES = (
    ("ordinary", [(-0.5, -0.5, 0.0), (0.75, -0.25, 0.25), (0.0, 0.5, -0.25)]),
    ("three equal", [(0.5, 0.25, 0.0)] * 3),
    ("two equal", [(0.5, 0.25, 0.0), (0.5, 0.25, 0.0), (-0.5, 0.0, 0.5)]),
    ("collinear", [(-0.5, -0.5, 0.0), (0.0, 0.0, 0.0), (0.5, 0.5, 0.0)]),
    ("in the camera plane", [(-0.5, -0.5, 0.0), (0.5, 0.0, 5.0), (0.0, 0.5, 0.0)]),
    ("behind the camera", [(-0.5, -0.5, 0.0), (0.5, 0.0, 9.0), (0.0, 0.5, 0.0)]),
    ("largest halves", [(65504.0, -65504.0, 65504.0), (-65504.0, 65504.0, 0.0), (65504.0, 65504.0, -65504.0)]),
    ("nan position", [(np.nan, -0.5, 0.0), (0.5, 0.0, 0.0), (0.0, 0.5, np.nan)]),
    ("inf position", [(-0.5, np.inf, 0.0), (0.5, 0.0, -np.inf), (0.0, 0.5, 0.0)]),
)
SPECIAL_DRAWS = ("ordinary", "scale 0", "scale -1", "zero quaternion", "unnormalised quaternion", "nan position", "scale 1e30", "ordinary, rotated")
ORDINARY_MATERIALS = (0, 1, 6)  # the materials whose factors go through pow and log2 to a code strictly inside the range


def special_scene(viewport=(64, 8)):
    """One meshlet of SPECIAL_TRIANGLES (27 vertices), SPECIAL_DRAWS, seven materials, and a record image that cycles through every (draw,
    triangle) pair.  Vertex attributes by hand: uv halves NaN, +-inf, denormal and -0, normal fields all 0, all 1023 and all 511 (a zero
    normal), tangent bytes (0, 0), (255, 255), (127, 127), the bitangent sign (bit 30 of np) set on some"""
    pos = np.array([p for _, tri in SPECIAL_TRIANGLES for p in tri], np.float32)
    tris = np.arange(len(pos)).reshape(-1, 3)
    draws = np.zeros(len(SPECIAL_DRAWS), L.MESHDRAW)
    draws["position"], draws["scale"], draws["orientation"] = (0.0, 0.0, -5.0), 1.0, (0.0, 0.0, 0.0, 1.0)
    draws["scale"][1], draws["scale"][2], draws["scale"][6] = 0.0, -1.0, 1e30
    draws["orientation"][3] = 0.0
    draws["orientation"][4] = (0.5, 1.0, -2.0, 3.0)
    draws["position"][5] = (np.nan, 0.0, -5.0)
    q = np.array([0.2, -0.4, 0.1, 0.85])
    draws["orientation"][7], draws["scale"][7], draws["position"][7] = (q / np.linalg.norm(q)).astype(np.float32), 1.5, (0.25, -0.1, -6.0)
    draws["materialIndex"] = (0, 2, 3, 4, 5, 1, 1, 6)
    s = RR.mesh_scene(pos, tris, viewport, draws=draws)
    assert len(s["meshlets"]) == 1 and int(s["meshlets"]["triangleCount"][0]) == len(SPECIAL_TRIANGLES)
    with np.errstate(all="ignore"):  # (normals of NaN positions: the fields are replaced below)
        v = VA.fill_attributes(s["vertices"], s["meshlets"], s["data"])  # ordinary attributes first, then the special ones over them
    uv = [H_NAN, H_INF, H_NINF, H_DENORMAL, H_NZERO, _h(0.25), _h(0.75)]
    nps = [0x00000000, 0x3FFFFFFF, 0x7FFFFFFF, 511 | 511 << 10 | 511 << 20, 0x40000000]
    tps = [0x0000, 0xFFFF, 0x7F7F, 0xFF00]
    for i in range(3, len(v)):  # (the ordinary triangle keeps its ordinary attributes)
        v["tu"][i], v["tv"][i] = uv[i % len(uv)], uv[(i // 2 + 3) % len(uv)]
        if i % 2:
            v["np"][i] = nps[(i // 2) % len(nps)]
        if i % 3 != 1:
            v["tp"][i] = tps[(i // 3) % len(tps)]
    s["vertices"] = v
    m = np.zeros(7, L.MATERIAL)
    m["diffuseFactor"][0], m["specularFactor"][0], m["emissiveFactor"][0] = (0.8, 0.3, 0.55, 1.0), (0.5, 0.5, 0.5, 0.37), (0.0, 0.0, 0.0)
    m["diffuseFactor"][1], m["specularFactor"][1], m["emissiveFactor"][1] = (0.12, 0.9, 0.4, 1.0), (0.1, 0.2, 0.3, 0.81), (1.5, 0.7, 0.2)
    m["diffuseFactor"][2], m["specularFactor"][2] = (0.0, -0.5, 2.0, 1.0), (0.0, 0.0, 0.0, -1.0)
    m["diffuseFactor"][3], m["specularFactor"][3] = (np.inf, np.nan, 0.0, 1.0), (0.0, 0.0, 0.0, 2.0)
    # 1 + emissivef == 0: -10 * 0.1f rounds to -1, 9.99 * 0.1f + 1e-3f rounds to 1 (asserted in the CPU file from the restatement's channel)
    m["diffuseFactor"][4], m["specularFactor"][4], m["emissiveFactor"][4] = (0.0, 0.0, 9.99, 1.0), (0.0, 0.0, 0.0, np.nan), (0.0, 0.0, -10.0)
    m["diffuseFactor"][5], m["emissiveFactor"][5] = (0.0, 0.0, 0.0, 1.0), (0.0, 0.0, -1.0)  # 1 + emissivef = -99
    m["diffuseFactor"][6], m["specularFactor"][6], m["emissiveFactor"][6] = (0.33, 0.66, 0.21, 1.0), (0.0, 0.0, 0.0, 0.5), (0.3, 0.1, 0.6)
    m[6]["albedoTexture"], m[6]["normalTexture"], m[6]["emissiveTexture"] = 2, 5, 1
    s["materials"] = m
    w, h = viewport
    pairs = np.array([(d, 0, t) for d in range(len(draws)) for t in range(len(SPECIAL_TRIANGLES))], np.uint32)
    s["records"] = _records(pairs[np.arange(w * h) % len(pairs)], np.random.default_rng(79))
    return s
