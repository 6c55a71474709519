"""What the tests that pin the shadow pass to shadow.comp.glsl share (tests/test_shadow_vs_ref.py, test_shadow_fixtures_cpu.py,
test_shadow_fixtures_gpu.py, tests/golden/generate.py): the image sizes, the inputs of a launch, the three scenes, the two exact
single-triangle cases (alpha == 0.5; tmin and tmax from both sides) and the fixture files.

A "scene" is shadow_ref.py's dict (meshes, indices, vertices, draws), the textured one with "materials" and "textures" (DDS file images) too;
a "set" is shadow_alpha_ref.py's dict (descs, texels)."""
import os

import numpy as np

import shadow_ref as SH
from niagara_amd import host, synth
from niagara_amd import layouts as L

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "shadow")
SIZES = [(21, 3), (65, 17), (67, 37)]  # the shading fixtures' (tests/shade_cases.py): odd widths; 65 wide drops the stores at pos.x == width
PREFILL = 0x5A                         # the byte the masks hold before a pass: neither 0 nor 255
SUN = np.array([2.0, 0.3, 1.0]) / np.linalg.norm([2.0, 0.3, 1.0])
RADIUS = 8.0                           # the instances lie within +-8 of the camera: a good part of the rays meets something
TMIN, TMAX = np.float32(1e-2), np.float32(1e3)
FLAGS = {0: 4 | 1024, 1: 4}            # shadow.comp.glsl:155-156: TerminateOnFirstHit (| ForceOpacityMicromap2State)


def same_bits(a, b):
    """elementwise: the same fp32 bits, a NaN matching a NaN whatever its sign or payload"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return (na & nb) | (~na & ~nb & (a.view(np.uint32) == b.view(np.uint32)))


def inputs(w, h, jitter, checkerboard, sun=SUN, odd=False, seed=0, dense=False):
    """(sd, depth): ShadowData of niagara's default camera at a w x h viewport and a random depth image — view-space distances 1 .. 60 (depth =
    znear / distance), a tenth of the texels exact zeros (sky: wposh.w == 0).  odd: the texels whose index is 0 .. 5 modulo 12 hold
    shadow_ref.ODD_DEPTHS (NaN, +inf, -inf, 3e38, -0.0, 1e-40), as shadow_ref.odd_depth_image lays them out.  dense: every entry of
    inverseViewProjection moved by a random amount, so that none is zero — the default camera's has eight zeros, and the order in which the
    four products of a row are summed shows only where all four are there"""
    rng = np.random.default_rng(100 * w + h + seed)
    cd = host.build_cull_data(viewport=(w, h), pyramid=(host.previous_pow2(w), host.previous_pow2(h)))
    sd = host.build_shadow_data(synth.make_globals(cd, (w, h)), sun, jitter, checkerboard, w, h)
    if dense:
        sd["inverseViewProjection"] = sd["inverseViewProjection"] + np.random.default_rng(77).uniform(0.05, 0.5, 16).astype(np.float32)
    depth = (0.1 / np.exp(rng.uniform(0.0, np.log(60.0), (h, w)))).astype(np.float32)
    depth[rng.random((h, w)) < 0.1] = 0.0
    if odd:
        flat = depth.reshape(-1)
        for j, v in enumerate(SH.ODD_DEPTHS):
            flat[j::12] = v
    return sd, depth


def owned(w, h, checkerboard):
    """the texels a pass stores to: pos.x = 2 x + ((y ^ checkerboard) & 1) (shadow.comp.glsl:129-134)"""
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    return ((x ^ y ^ checkerboard) & 1) == 0 if checkerboard > 0 else np.ones((h, w), bool)


INSTANCES, SEED = 40, 11  # shadow_ref.fuzz_scene's arguments for all three scenes: the same boxes and walls, another postPass


def _scene(post_pass):
    """the instances with `post_pass`, and meshes whose lods[lodRT] is not lods[0]: both meshes get a second LOD, the second half of their
    triangles; the wall traces it (lodRT 1: half a wall), the box keeps lodRT 0"""
    s = SH.fuzz_scene(instances=INSTANCES, seed=SEED, radius=RADIUS)
    m = s["meshes"].copy()
    first, count = m["lods"]["indexOffset"][:, 0].copy(), m["lods"]["indexCount"][:, 0].copy()
    assert (m["lodCount"] == 1).all() and (m["lodRT"] == 0).all() and (count % 6 == 0).all()
    m["lods"]["indexOffset"][:, 1], m["lods"]["indexCount"][:, 1] = first + count // 2, count // 2
    m["lodCount"] = 2
    m["lodRT"] = (1, 0)
    s["meshes"] = m
    s["draws"] = s["draws"].copy()
    s["draws"]["postPass"] = post_pass
    return s


def opaque_scene():
    """postPass drawn from {0, 2}: neither side has a post-pass caster at any quality, and every ray is compared"""
    return _scene(np.where(np.random.default_rng(5).random(INSTANCES) < 0.3, 2, 0))


def mixed_scene():
    """every third draw in the post pass (postPass 1), a few more never casting (2): quality 0's single rayQueryProceedEXT meets non-opaque
    triangles, for some rays before an opaque one in the walk order and for some after"""
    i = np.arange(INSTANCES)
    return _scene(np.where(i % 3 == 1, 1, np.where(i % 7 == 3, 2, 0)))


def textured_scene():
    """(scene, set): synth.with_textures(..., cutout=True) over the instances, six in ten of them post-pass draws (postPass 1) among opaque ones
    and a few that never cast (postPass 2).  Of the five materials one has albedoTexture == 0 and one names a texture past the table"""
    r = np.random.default_rng(SEED + 7).random(INSTANCES)
    s = synth.with_textures(_scene(np.where(r < 0.6, 1, np.where(r < 0.67, 2, 0))), size=32, cutout=True)
    m = s["materials"].copy()
    m["albedoTexture"][3] = 0
    m["albedoTexture"][4] = len(s["textures"]) + 5
    s["materials"] = m
    descs, texels = host.texture_decode_host(s["textures"])
    return s, dict(descs=descs, texels=texels)


def half_alpha_case():
    """(sd, depth, scene, set, uv): ONE ray whose hit lands on alpha == 0.5 exactly.  A single triangle with corners (0, 0, 0), (4, 0, 0), (0, 4,
    0) and texcoords (0, 0), (1, 0), (0, 1) (identity transform, postPass 1) under a 2 x 1 texture of alpha 0 and 255; the ray starts at (2, 1,
    -1) and runs along +z.  With kz = z, Sx = Sy = 0 every product of T is a small integer: U = 4, V = 8, W = 4, det = 16, so the barycentrics are
    0.5 and 0.25 and uv = (0.5, 0.25) exactly.  REPEAT: u = 0.5 x 2 - 0.5 = 0.5 = floor 0 + weight 0.5, so alpha = 0 x 0.5 + 1 x 0.5 = 0.5 in
    fp32 without rounding (255 / 255 = 1).  `>= 0.5` confirms; `> 0.5` would not."""
    meshes = np.zeros(1, L.MESH)
    meshes["vertexCount"], meshes["lodCount"] = 3, 1
    meshes["lods"]["indexCount"][0, 0] = 3
    v = np.zeros(3, L.VERTEX)
    pos = np.array([(0, 0, 0), (4, 0, 0), (0, 4, 0)], np.float16)
    uv = np.array([(0, 0), (1, 0), (0, 1)], np.float16)
    for k, n in enumerate(("vx", "vy", "vz")):
        v[n] = pos[:, k].view(np.uint16)
    v["tu"], v["tv"] = uv[:, 0].view(np.uint16), uv[:, 1].view(np.uint16)
    draws = np.zeros(1, L.MESHDRAW)
    draws["orientation"], draws["scale"], draws["postPass"] = (0.0, 0.0, 0.0, 1.0), 1.0, 1
    m = np.zeros(1, L.MATERIAL)
    m["albedoTexture"] = 1
    img = np.full((1, 2, 4), 200, np.uint8)
    img[0, :, 3] = (0, 255)
    import shadow_alpha_ref as SA
    tset = SA.texture_set([[img]])
    # one invocation: clip = (0, 0, depth, 1) at the 1 x 1 image; the matrix puts it at (2, 1, -1)
    mat = np.zeros((4, 4), np.float32)  # mat[column, row]
    mat[3] = (2.0, 1.0, -1.0, 1.0)
    sd = np.zeros(1, L.SHADOWDATA)
    sd["sunDirection"], sd["inverseViewProjection"], sd["imageSize"] = (0.0, 0.0, 1.0), mat.reshape(-1), (1, 1)
    scene = dict(meshes=meshes, indices=np.arange(3, dtype=np.uint32), vertices=v, draws=draws, materials=m)
    return sd, np.full((1, 1), 0.5, np.float32), scene, tset, np.array([0.5, 0.25], np.float32)


RANGE_T = (2.0 ** -7, 2.0 ** -6, 512.0, 1024.0)  # outside / inside tmin = 1e-2, inside / outside tmax = 1e3
RANGE_MASK = np.array([[255, 0, 0, 255]], np.uint8)


def range_case():
    """(sd, depth, opaque scene, textured scene, set, DDS files): FOUR rays that hold tmin and tmax from both sides, exactly.  A 4 x 1 image;
    pixel k starts at (16 k + 2, 1, 0) and runs along +z (the matrix below: clip.x = k / 2 - 3 / 4, origin.x = 32 clip.x + 26, every value a
    small dyadic number).  One mesh of four triangles, triangle k with the corners (16 k, 0, t), (16 k + 4, 0, t), (16 k, 4, t) at t =
    RANGE_T[k]: ray k can meet triangle k alone.  Identity transform, so kz = z, Sx = Sy = 0, Sz = 1 and, as in half_alpha_case, U = 4, V = 8,
    W = 4, det = 16, T = 16 t: the hit parameter is t itself, with no rounding (powers of two, all fp16 numbers).  2^-7 < 1e-2 < 2^-6 and 512 <
    1e3 < 1024, so the mask is lit, shadowed, shadowed, lit — and a tmin of 2e-2 or 5e-3, or a tmax of 1e4 or 5e2, changes a byte.  The opaque
    scene has the draw at postPass 0; the textured one at postPass 1 under a one-colour albedo texture of alpha 255 (a 4 x 4 BC1 file), so that
    the hit goes through the candidate / confirm path"""
    meshes = np.zeros(1, L.MESH)
    meshes["vertexCount"], meshes["lodCount"] = 12, 1
    meshes["lods"]["indexCount"][0, 0] = 12
    pos = np.array([c for k, t in enumerate(RANGE_T) for c in ((16 * k, 0, t), (16 * k + 4, 0, t), (16 * k, 4, t))], np.float16)
    assert (pos.astype(np.float64)[2::3, 2] == RANGE_T).all()
    v = np.zeros(12, L.VERTEX)
    for k, n in enumerate(("vx", "vy", "vz")):
        v[n] = pos[:, k].view(np.uint16)
    draws = np.zeros(1, L.MESHDRAW)
    draws["orientation"], draws["scale"] = (0.0, 0.0, 0.0, 1.0), 1.0
    post = draws.copy()
    post["postPass"] = 1
    m = np.zeros(1, L.MATERIAL)
    m["albedoTexture"] = 1
    img = np.full((4, 4, 4), 200, np.uint8)
    img[..., 3] = 255
    files = [synth.dds_bytes(img, mips=False)]
    descs, texels = host.texture_decode_host(files)
    assert (texels >> 24 == 255).all()
    mat = np.zeros((4, 4), np.float32)  # mat[column, row]
    mat[0, 0] = 32.0
    mat[3] = (26.0, 1.0, 0.0, 1.0)
    sd = np.zeros(1, L.SHADOWDATA)
    sd["sunDirection"], sd["inverseViewProjection"], sd["imageSize"] = (0.0, 0.0, 1.0), mat.reshape(-1), (4, 1)
    geometry = dict(meshes=meshes, indices=np.arange(12, dtype=np.uint32), vertices=v, materials=m)
    return sd, np.full((1, 4), 0.5, np.float32), dict(geometry, draws=draws), dict(geometry, draws=post), dict(descs=descs, texels=texels), files


# the committed fixtures, by name (a missing file fails where it is loaded): the three image sizes, and range_case's four rays
SIZE_FIXTURES = [os.path.join(GOLDEN, "%dx%d.npz" % s) for s in SIZES]
RANGE_FIXTURE = os.path.join(GOLDEN, "range.npz")
FIXTURES = SIZE_FIXTURES + [RANGE_FIXTURE]
FIXTURE_IDS = [os.path.basename(p)[:-4] for p in FIXTURES]
FIXTURE_LAUNCHES = [(0, 0.0), (1, 1e-2)]  # (checkerboard, sunJitter) of the launches a size fixture holds; the range fixture holds one launch


def fixture_files(f):
    """the DDS file images a fixture's set was decoded from"""
    return [x.tobytes() for x in np.split(f["dds"], np.cumsum(f["dds_sizes"])[:-1])]


def moved(draws):
    """the draws at other positions: each takes its neighbour's, 3 further along every axis (a scene built over them has another TLAS, and
    other masks, than one over `draws`)"""
    out = draws.copy()
    out["position"] = np.roll(out["position"], 1, axis=0) + np.float32(3.0)
    return out


def fixture_scene(f, textured):
    """(scene, set) from a fixture's arrays; the untextured scene is the textured one's geometry with opaque_scene's postPass"""
    s = dict(meshes=np.ascontiguousarray(f["meshes"]).view(L.MESH).reshape(-1), indices=f["indices"], vertices=np.ascontiguousarray(f["vertices"]).view(L.VERTEX).reshape(-1),
             draws=np.ascontiguousarray(f["draws_textured" if textured else "draws_opaque"]).view(L.MESHDRAW).reshape(-1),
             materials=np.ascontiguousarray(f["materials"]).view(L.MATERIAL).reshape(-1))
    t = dict(descs=np.ascontiguousarray(f["descs"]).view(L.TEXTUREDESC).reshape(-1), texels=f["texels"])
    return s, t


def fixture_launch(f, k):
    """(sd, depth) of launch k of a fixture"""
    return np.frombuffer(f["sd"][k].tobytes(), L.SHADOWDATA).copy(), f["depth"]
