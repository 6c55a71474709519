"""ctypes loader of tests/shadow_ref.c, the BRUTE-FORCE CPU restatement of nv_shadow_trace (test infrastructure), and the inputs the shadow
trace tests share: the small instanced scene of the fuzz, its rays, the degenerate rays.

`load(directory)` compiles the restatement there with raster_ref.py's flags (fp32, -ffp-contract=off).  A "scene" is a dict with meshes
(layouts.MESH, the LODs' index ranges set), indices (u32), vertices (layouts.VERTEX) and draws (layouts.MESHDRAW)."""
import ctypes as C
import os
import subprocess

import numpy as np

import raster_ref as RR
from niagara_amd import layouts as L

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "shadow_ref.c")
TMIN, TMAX = 1e-2, 1e3  # shadow.comp.glsl:81


def _p(a):
    return None if a is None or a.size == 0 else C.c_void_p(a.ctypes.data)


def _scene_args(scene):
    m = np.ascontiguousarray(scene["meshes"], L.MESH)
    i = np.ascontiguousarray(scene["indices"], np.uint32)
    v = np.ascontiguousarray(scene["vertices"], L.VERTEX)
    d = np.ascontiguousarray(scene["draws"], L.MESHDRAW)
    return (m, i, v, d), (_p(m), C.c_uint32(len(m)), _p(i), C.c_uint32(len(i)), _p(v), C.c_uint32(len(v)), _p(d), C.c_uint32(len(d)))


class ShadowRef:
    def __init__(self, so):
        self.lib = C.CDLL(so)
        for f in ("shr_rays", "shr_trace", "shr_shadow_trace"):
            getattr(self.lib, f).restype = None
        assert self.lib.shr_sizes_ok() == 1

    def rays(self, sd, depth):
        """(origins, dirs), each (h, w, 3) f32: the ray of every pixel of the full-resolution image"""
        h, w = depth.shape
        sd = np.ascontiguousarray(sd, L.SHADOWDATA)
        d = np.ascontiguousarray(depth, np.float32)
        o, r = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 3), np.float32)
        self.lib.shr_rays(_p(sd), _p(d), C.c_uint32(w), C.c_uint32(h), _p(o), _p(r))
        return o, r

    def trace(self, scene, origins, dirs, quality, tmin=TMIN, tmax=TMAX):
        """the mask bytes (0 = occluded, 255 = not) of (n, 3) rays: every casting triangle of every casting instance is tested"""
        keep, args = _scene_args(scene)
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        r = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        out = np.zeros(len(o), np.uint8)
        self.lib.shr_trace(*args, _p(o), _p(r), C.c_uint64(len(o)), C.c_float(tmin), C.c_float(tmax), C.c_int(quality), _p(out))
        del keep
        return out

    def shadow_trace(self, sd, scene, depth, shadow, quality):
        """the pass over a copy of `shadow` (h, w) u8: texels no invocation owns keep their bytes"""
        h, w = depth.shape
        keep, args = _scene_args(scene)
        sd = np.ascontiguousarray(sd, L.SHADOWDATA)
        d = np.ascontiguousarray(depth, np.float32)
        s = np.ascontiguousarray(shadow, np.uint8).reshape(h, w).copy()
        self.lib.shr_shadow_trace(_p(sd), *args, _p(d), _p(s), C.c_uint32(w), C.c_uint32(h), C.c_int(quality))
        del keep
        return s


def load(directory):
    so = os.path.join(str(directory), "libshadow_ref.so")
    if not os.path.exists(so):
        subprocess.check_call(["gcc"] + RR.FLAGS + ["-Wall", "-shared", "-fPIC", "-o", so, SRC, "-lm"])
    return ShadowRef(so)


def geometry():
    """two meshes for the instanced scenes: 0 = a wall (a 4 x 4 grid of quads over [-1, 1]^2 at z = 0, 32 triangles), 1 = a closed box
    ([-1, 1]^3, 2 x 2 quads per face, 48 triangles); every coordinate is -1, -0.5, 0, 0.5 or 1.  Returns (meshes, indices, vertices)"""
    import oracle
    from niagara_amd import synth
    grid_pos, grid_tris = synth._grid_meshlets(4, 4, 2)
    box_pos, box_tris = synth._box_faces(2)
    meshes, meshlets, data, vertices = synth._pack_meshes(((grid_pos, grid_tris, 0), (box_pos, box_tris, 1)), oracle.meshlet_bounds)
    indices, meshes = synth.indexed_geometry(meshes, meshlets, data)
    return meshes, indices, vertices


def _rotate(v, q):
    """rotateQuat in fp64: v (n, 3), q (4,) or (n, 4) as x, y, z, w"""
    q = np.broadcast_to(np.asarray(q, np.float64), (len(v), 4))
    t = np.cross(q[:, :3], v) + q[:, 3:] * v
    return v + 2.0 * np.cross(q[:, :3], t)


def fuzz_scene(instances=20, seed=11, radius=300.0):
    """the small instanced scene of the fuzz: box and wall instances with random unit quaternions, scales in [0.25, 8], positions within
    +-radius, postPass 0 / 1 / 2"""
    rng = np.random.default_rng(seed)
    meshes, indices, vertices = geometry()
    draws = np.zeros(instances, dtype=L.MESHDRAW)
    q = rng.normal(size=(instances, 4))
    draws["orientation"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    draws["scale"] = np.exp(rng.uniform(np.log(0.25), np.log(8.0), instances)).astype(np.float32)
    draws["position"] = rng.uniform(-radius, radius, (instances, 3)).astype(np.float32)
    draws["meshIndex"] = rng.integers(0, 2, instances)
    draws["postPass"] = np.arange(instances) % 3
    return dict(meshes=meshes, indices=indices, vertices=vertices, draws=draws)


def surface_points(scene, which, rng):
    """one random world-space point (fp64) on a random triangle of each draw in `which`"""
    m, idx, v, d = scene["meshes"], scene["indices"].astype(np.int64), scene["vertices"], scene["draws"]
    pos = np.stack([v[k].view(np.float16).astype(np.float64) for k in ("vx", "vy", "vz")], 1)
    which = np.asarray(which)
    mi = d["meshIndex"][which]
    rt = m["lodRT"][mi]
    first, count = m["lods"]["indexOffset"][mi, rt].astype(np.int64), m["lods"]["indexCount"][mi, rt].astype(np.int64) // 3
    t = np.minimum((rng.random(len(which)) * count).astype(np.int64), count - 1)
    corners = idx[first[:, None] + 3 * t[:, None] + np.arange(3)] + m["vertexOffset"][mi].astype(np.int64)[:, None]
    b = rng.dirichlet((1.0, 1.0, 1.0), len(which))
    out = (b[:, :, None] * pos[corners]).sum(1)
    world = d["position"][which].astype(np.float64) + d["scale"][which, None].astype(np.float64) * _rotate(out, d["orientation"][which].astype(np.float64))
    return world


def fuzz_rays(scene, n, seed=12):
    """n rays against fuzz_scene: a third from free space at a surface point, a third from a surface point at another surface point (origins
    on surfaces, grazing their own triangle), a third from a surface point in a random direction; directions are normalised in fp32 as the
    pass's are, a few are left unnormalised"""
    rng = np.random.default_rng(seed)
    nd = len(scene["draws"])
    a, b = rng.integers(0, nd, n), rng.integers(0, nd, n)
    target, other = surface_points(scene, a, rng), surface_points(scene, b, rng)
    free = target + rng.normal(size=(n, 3)) * np.exp(rng.uniform(np.log(0.05), np.log(200.0), (n, 1)))
    kind = np.arange(n) % 3
    origin = np.where((kind == 0)[:, None], free, other)
    rnd = rng.normal(size=(n, 3))
    direction = np.where((kind == 2)[:, None], rnd, target - origin)
    direction = direction / np.maximum(np.linalg.norm(direction, axis=1, keepdims=True), 1e-30)
    direction[::17] *= rng.uniform(0.1, 10.0, (len(direction[::17]), 1))
    return origin.astype(np.float32), direction.astype(np.float32)


def aligned_scene():
    """instances whose world coordinates are exact: a box and a wall with the identity orientation, power-of-two scales and integer
    positions, one of them in the post pass.  Box planes, triangle edges and vertices lie on multiples of 0.25."""
    meshes, indices, vertices = geometry()
    draws = np.zeros(3, dtype=L.MESHDRAW)
    draws["orientation"] = (0.0, 0.0, 0.0, 1.0)
    draws["position"] = [(0.0, 0.0, 0.0), (8.0, 0.0, -4.0), (-6.0, 2.0, 3.0)]
    draws["scale"] = (1.0, 2.0, 0.5)
    draws["meshIndex"] = (1, 0, 1)
    draws["postPass"] = (0, 0, 1)
    return dict(meshes=meshes, indices=indices, vertices=vertices, draws=draws)


def degenerate_rays(scene):
    """axis-aligned rays with exact zero components through a lattice of step 0.25 s around every instance of aligned_scene (origins exactly on
    box planes, on triangle edges and on vertices: U, V or W is 0 and the fp64 branch runs), the same lattice along the face diagonals,
    origins ON the surfaces, and rays with non-finite components"""
    o, d = [], []
    axes = np.eye(3)
    for dr in scene["draws"]:
        p, s = dr["position"].astype(np.float64), float(dr["scale"])
        g = np.arange(-5, 6) * 0.25 * s
        for k in range(3):
            u, v = np.meshgrid(g, g)
            for start in (-3.0 * s, -1.0 * s, 0.0, 1.0 * s):  # in front of the instance, on its planes, inside it
                for sign in (1.0, -1.0):
                    pts = np.zeros((u.size, 3))
                    pts[:, (k + 1) % 3], pts[:, (k + 2) % 3], pts[:, k] = u.reshape(-1), v.reshape(-1), start * sign
                    o.append(pts + p)
                    d.append(np.broadcast_to(axes[k] * sign, pts.shape))
        for diag in ((1, 1, 0), (1, -1, 0), (0, 1, 1), (1, 0, -1), (1, 1, 1)):
            pts = np.stack(np.meshgrid(g[::2], g[::2], g[::2]), -1).reshape(-1, 3)
            o.append(pts + p)
            d.append(np.broadcast_to(np.asarray(diag, np.float64), pts.shape))
    o, d = np.concatenate(o).astype(np.float32), np.concatenate(d).astype(np.float32)
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    bo, bd = [], []
    for k in range(3):
        for b in bad:
            x = np.array([0.25, 0.25, -5.0], np.float32)
            x[k] = b
            bo.append(x), bd.append(np.array([0, 0, 1], np.float32))
            y = np.array([0.0, 0.0, 1.0], np.float32)
            y[k] = b
            bo.append(np.array([0.25, 0.25, -5.0], np.float32)), bd.append(y)
    bo.append(np.array([0.25, 0.25, -5.0], np.float32)), bd.append(np.zeros(3, np.float32))  # a zero direction
    return np.concatenate([o, np.stack(bo)]), np.concatenate([d, np.stack(bd)])


load.__test__ = False
