"""ctypes loader of tests/shadow_alpha_ref.c, the BRUTE-FORCE CPU restatement of nv_shadow_trace_textured (test infrastructure), and the inputs
the alpha-tested shadow trace tests share: the textured fuzz scene, raw RGBA8 texture sets, the layered cut-out scene.

A "scene" is shadow_ref.py's dict (meshes, indices, vertices, draws) plus "materials" (layouts.MATERIAL).  A "set" is a dict with "descs"
(layouts.TEXTUREDESC, entry 0 reserved) and "texels" (uint32: the caller's decoded RGBA8 buffer, R in the low byte, alpha in the top one)."""
import ctypes as C
import os
import subprocess

import numpy as np

import raster_ref as RR
import shadow_ref as SH
from niagara_amd import layouts as L

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "shadow_alpha_ref.c")
_p = SH._p


def _alpha_args(scene, tset, texel_words=None):
    m = np.ascontiguousarray(scene["materials"], L.MATERIAL)
    d = np.ascontiguousarray(tset["descs"], L.TEXTUREDESC)
    x = np.ascontiguousarray(tset["texels"], np.uint32)
    words = len(x) if texel_words is None else int(texel_words)
    return (m, d, x), (_p(m), C.c_uint32(len(m)), _p(d), C.c_uint32(len(d)), _p(x), C.c_uint64(words))


class ShadowAlphaRef:
    def __init__(self, so):
        self.lib = C.CDLL(so)
        for f in ("sar_trace", "sar_shadow_trace", "sar_interpolate_uv"):
            getattr(self.lib, f).restype = None
        assert self.lib.sar_sizes_ok() == 1

    def trace(self, scene, tset, origins, dirs, quality=1, tmin=SH.TMIN, tmax=SH.TMAX, texel_words=None):
        """(mask, rejected) of (n, 3) rays: mask 0 = occluded, 255 = not; rejected = the accepted candidates the alpha test did not confirm"""
        keep, args = SH._scene_args(scene)
        keep2, alpha = _alpha_args(scene, tset, texel_words)
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        r = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        out, rejected = np.zeros(len(o), np.uint8), np.zeros(len(o), np.uint32)
        self.lib.sar_trace(*args, *alpha, _p(o), _p(r), C.c_uint64(len(o)), C.c_float(tmin), C.c_float(tmax), C.c_int(quality), _p(out), _p(rejected))
        del keep, keep2
        return out, rejected

    def interpolate_uv(self, bary, tu, tv):
        """shadow.comp.glsl:113 for n hits: bary (n, 2), the corners' texcoords tu, tv (n, 3) -> uv (n, 2), all float32"""
        b, u, v = (np.ascontiguousarray(a, np.float32) for a in (bary, tu, tv))
        out = np.zeros((len(b), 2), np.float32)
        self.lib.sar_interpolate_uv(_p(b), _p(u), _p(v), C.c_uint64(len(b)), _p(out))
        return out

    def shadow_trace(self, sd, scene, tset, depth, shadow, quality=1):
        """(mask, rejected): the pass over a copy of `shadow` (h, w) u8 — texels no invocation owns keep their bytes, and a rejected count of 0"""
        h, w = depth.shape
        keep, args = SH._scene_args(scene)
        keep2, alpha = _alpha_args(scene, tset)
        sd = np.ascontiguousarray(sd, L.SHADOWDATA)
        d = np.ascontiguousarray(depth, np.float32)
        s = np.ascontiguousarray(shadow, np.uint8).reshape(h, w).copy()
        rejected = np.zeros((h, w), np.uint32)
        self.lib.sar_shadow_trace(_p(sd), *args, *alpha, _p(d), _p(s), _p(rejected), C.c_uint32(w), C.c_uint32(h), C.c_int(quality))
        del keep, keep2
        return s, rejected


def load(directory):
    so = os.path.join(str(directory), "libshadow_alpha_ref.so")
    if not os.path.exists(so):
        subprocess.check_call(["gcc"] + RR.FLAGS + ["-Wall", "-shared", "-fPIC", "-o", so, SRC, "-lm"])
    return ShadowAlphaRef(so)


def texture_set(images):
    """a set from RGBA8 chains: images = a list of textures, each a list of (h, w, 4) uint8 levels (level 0 first).  Entry 0 is reserved"""
    descs = np.zeros(len(images) + 1, L.TEXTUREDESC)
    words, at = [], 0
    for k, levels in enumerate(images):
        h, w = levels[0].shape[:2]
        descs[k + 1] = (at, w, h, len(levels))
        for lv in levels:
            words.append(np.ascontiguousarray(lv, np.uint8).reshape(-1, 4).view(np.uint32).reshape(-1))
            at += words[-1].size
    return dict(descs=descs, texels=np.concatenate(words) if words else np.zeros(0, np.uint32))


def flat_texture(alpha, w=1, h=1):
    """one level of a single alpha code"""
    img = np.full((h, w, 4), 200, np.uint8)
    img[..., 3] = alpha
    return [img]


def random_textures(rng, count=6):
    """`count` textures of odd, non-square and one-texel sizes with one to three levels; every texel's alpha is 0 or 255 with equal odds, so
    about half of the samples land under 0.5"""
    shapes = [(8, 8, 1), (5, 3, 2), (1, 1, 1), (16, 4, 3), (7, 1, 1), (2, 9, 2), (12, 12, 2), (3, 3, 1)]
    out = []
    for k in range(count):
        w, h, levels = shapes[k % len(shapes)]
        chain = []
        for lv in range(levels):
            img = rng.integers(0, 256, (max(1, h >> lv), max(1, w >> lv), 4)).astype(np.uint8)
            img[..., 3] = np.where(rng.random(img.shape[:2]) < 0.5, 0, 255)
            chain.append(img)
        out.append(chain)
    return out


def with_texcoords(scene, rng, span=2.0):
    """a copy of the scene whose vertices carry random fp16 texcoords in [-span, span] (REPEAT takes them anywhere)"""
    s = dict(scene)
    v = scene["vertices"].copy()
    uv = rng.uniform(-span, span, (len(v), 2)).astype(np.float16)
    v["tu"], v["tv"] = uv[:, 0].view(np.uint16), uv[:, 1].view(np.uint16)
    s["vertices"] = v
    return s


# the textured fuzz scene: the values the CPU test tuned until the restatement met the issue's input conditions (tests/test_shadow_alpha_cpu.py)
FUZZ = dict(instances=20, seed=11, radius=8.0, post_share=0.6, textures=6)


def textured_fuzz_scene(instances=FUZZ["instances"], seed=FUZZ["seed"], radius=FUZZ["radius"], post_share=FUZZ["post_share"], textures=FUZZ["textures"]):
    """(scene, set): shadow_ref.fuzz_scene with texcoords, `post_share` of the draws in the post pass (one in 25 postPass 2: never
    casting), a material per texture plus one without a texture, one with a texture id out of range, and a draw whose material index is out
    of range"""
    rng = np.random.default_rng(seed + 1000)
    s = with_texcoords(SH.fuzz_scene(instances=instances, seed=seed, radius=radius), rng)
    tset = texture_set(random_textures(rng, textures))
    m = np.zeros(textures + 2, L.MATERIAL)
    m["albedoTexture"] = list(range(1, textures + 1)) + [0, textures + 7]
    m["diffuseFactor"] = (1, 1, 1, 1)
    d = s["draws"].copy()
    r = rng.random(instances)
    d["postPass"] = np.where(r < post_share, 1, np.where(r < post_share + 0.04, 2, 0))
    d["materialIndex"] = rng.integers(0, textures, instances)  # mostly textured
    d["materialIndex"][::9] = textures      # no texture
    d["materialIndex"][4::13] = textures + 1  # a texture id past the set
    d["materialIndex"][7::17] = len(m) + 3    # a material index past the table
    s["draws"], s["materials"] = d, m
    return s, tset


def textured_aligned_scene():
    """(scene, set): shadow_ref.aligned_scene with random texcoords, its boxes in the post pass (postPass 1, 0, 1), a material per draw and
    three random clear / solid textures: on edges and vertices T takes its fp64 branch and the barycentrics come from its values"""
    rng = np.random.default_rng(21)
    s = with_texcoords(SH.aligned_scene(), rng)
    s["draws"] = s["draws"].copy()
    s["draws"]["postPass"] = (1, 0, 1)
    s["draws"]["materialIndex"] = (0, 1, 2)
    t = texture_set(random_textures(rng, 3))
    s["materials"] = np.zeros(3, L.MATERIAL)
    s["materials"]["albedoTexture"] = (1, 2, 3)
    return s, t


def reference_masks(aref, scene, tset, launches, quality=1):
    """(masks, rejected), each (launches, n, n): the restatement's pass over a poisoned mask for every launch of shadow_ref.degenerate_launches"""
    out = SH.in_threads(lambda l: aref.shadow_trace(l[1], scene, tset, l[2], np.full(l[2].shape, SH.POISON, np.uint8), quality), launches)
    return np.stack([m for m, _ in out]), np.stack([r for _, r in out])


def layered_scene(box=False):
    """(scene, set): a cut-out wall (postPass 1, an 8 x 8 alpha checker; the wall mesh is 4 x 4 quads with texcoords (x, y) * 0.5 + 0.5, so a
    checker cell is half a quad and a BLAS leaf's triangles straddle opaque and clear cells) at z = 6 above an opaque wall (postPass 0) that
    covers the half x < 0 at z = 3, both facing +z, over a receiver plane at z = 0.  box: a third draw, a tilted cut-out box (postPass 1, the
    same checker over texcoords skewed by z) above the open half: a ray through it crosses two of its faces, near an edge two triangles of
    one BLAS leaf"""
    meshes, indices, vertices = SH.geometry()
    v = vertices.copy()
    pos = np.stack([v["vx"], v["vy"], v["vz"]], -1).view(np.float16).astype(np.float32)
    uv = (np.stack([pos[:, 0] + 0.375 * pos[:, 2], pos[:, 1] + 0.625 * pos[:, 2]], -1) * 0.5 + 0.5).astype(np.float16)  # the wall lies in z = 0
    v["tu"], v["tv"] = uv[:, 0].view(np.uint16), uv[:, 1].view(np.uint16)
    draws = np.zeros(3 if box else 2, L.MESHDRAW)
    draws["orientation"] = (0.0, 0.0, 0.0, 1.0)
    draws["position"][:2] = [(0.0, 0.0, 6.0), (-4.0, 0.0, 3.0)]
    draws["scale"][:2] = (4.0, 4.0)
    draws["meshIndex"] = 0
    draws["postPass"][:2] = (1, 0)
    draws["materialIndex"][:2] = (0, 1)
    if box:
        q = np.array([0.3, -0.5, 0.2, 0.8])
        draws[2]["orientation"], draws[2]["position"], draws[2]["scale"] = (q / np.linalg.norm(q)).astype(np.float32), (2.0, -1.0, 9.0), 1.25
        draws[2]["meshIndex"], draws[2]["postPass"], draws[2]["materialIndex"] = 1, 1, 0
    m = np.zeros(2, L.MATERIAL)
    m["albedoTexture"] = (1, 1)  # the opaque wall names the cut-out texture too: postPass 0 never samples it
    y, x = np.mgrid[0:8, 0:8]
    img = np.full((8, 8, 4), 255, np.uint8)
    img[..., 3] = np.where((x + y) % 2 == 1, 0, 255)
    return dict(meshes=meshes, indices=indices, vertices=v, draws=draws, materials=m), texture_set([[img]])


def leaf_subscenes(blob, scene, draw):
    """one scene per BLAS leaf with two or more triangles of draw `draw`'s mesh: that draw alone, its mesh cut down to the leaf's triangles
    (positions and texcoords taken from the blob).  The restatement over such a scene says what one leaf holds for a ray"""
    h = blob[:64].view(np.uint32)
    table_off, blas_off, tri_off = int(h[8]), int(h[11]), int(h[12])
    mi = int(scene["draws"]["meshIndex"][draw])
    node_first, node_count, tri_first, _ = (int(x) for x in blob[table_off + 32 * mi:][:16].view(np.uint32))
    nodes = blob[blas_off + 32 * node_first:][:32 * node_count].view(np.uint32).reshape(-1, 8)
    tris = blob[tri_off + 48 * tri_first:].view(np.uint32)
    out = []
    for leaf in nodes[:, 7]:
        first, count = int(leaf) & ((1 << 29) - 1), int(leaf) >> 29
        if count < 2:
            continue
        c = tris[12 * first:12 * (first + count)].reshape(-1, 4)  # a corner per row: x, y, z bits, the texcoord word
        v = np.zeros(len(c), L.VERTEX)
        p = c[:, :3].copy().view(np.float32).astype(np.float16)
        v["vx"], v["vy"], v["vz"] = (p[:, k].view(np.uint16) for k in range(3))
        v["tu"], v["tv"] = c[:, 3] & 0xffff, c[:, 3] >> 16
        m = np.zeros(1, L.MESH)
        m["vertexCount"], m["lodCount"] = len(v), 1
        m["lods"]["indexCount"][0, 0] = len(v)
        d = scene["draws"][draw:draw + 1].copy()
        d["meshIndex"] = 0
        out.append(dict(meshes=m, indices=np.arange(len(v), dtype=np.uint32), vertices=v, draws=d, materials=scene["materials"]))
    return out


load.__test__ = False
