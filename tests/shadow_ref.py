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
        self.lib.shr_fp64_rays.restype = self.lib.shr_fp64_decided_rays.restype = C.c_uint64
        assert self.lib.shr_sizes_ok() == 1

    def fp64_rays(self):
        """the rays since the last call for which T took its fp64 branch against a casting triangle (before the ray was decided)"""
        return int(self.lib.shr_fp64_rays())

    def fp64_decided_rays(self):
        """those among them for which the branch turned an fp32 zero of U, V or W into a number with a sign"""
        return int(self.lib.shr_fp64_decided_rays())

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


# ---- the same rays as LAUNCHES of the pass: rt_pixel_ray is affine in (cx, cy, depth) once the matrix's last row is (0, 0, 0, 1), so a
# hand-made inverseViewProjection turns the n x n invocations of nv_shadow_trace* into a chosen lattice of rays.  The CPU tests and
# tests/test_shadow_degenerate_gpu.py share everything below.

LATTICE_N = 16  # 16 x 16: four 8 x 8 tiles, one workgroup whose four waves have all 64 lanes live


def affine_launch(base, ex, ey, k, third, sun, jitter=0.0, n=LATTICE_N, checkerboard=0):
    """(sd, depth) of an n x n launch (n a power of two) whose pixel (px, py) starts at base + ex (px - n / 2) + ey (py - n / 2) in the two
    components other than k (ex and ey have none along k) and at its depth texel `third` (a scalar or an (n, n) array, any fp32 value) in
    component k, and runs along normalize(sun) plus the jitter.  cx = (2 px + 1 - n) / n, so the column ex n / 2 gives ex (px - n / 2) +
    ex / 2 and the translation takes the half steps back; with few-bit values every product and sum of rt_unproject is exact"""
    assert n >= 2 and n & (n - 1) == 0
    base, ex, ey = (np.asarray(v, np.float64) for v in (base, ex, ey))
    assert ex[k] == 0 and ey[k] == 0
    m = np.zeros((4, 4), np.float64)  # m[column, row]: column-major
    m[0, :3], m[1, :3], m[2, k] = ex * n / 2, -ey * n / 2, 1.0
    m[3, :3], m[3, 3] = base - ex / 2 - ey / 2, 1.0
    m[3, k] = 0.0
    sd = np.zeros(1, L.SHADOWDATA)
    sd["sunDirection"], sd["sunJitter"], sd["inverseViewProjection"] = np.asarray(sun, np.float32), np.float32(jitter), m.reshape(-1).astype(np.float32)
    sd["imageSize"], sd["checkerboard"] = (n, n), checkerboard
    depth = np.ascontiguousarray(np.broadcast_to(np.asarray(third, np.float32), (n, n)))
    return sd, depth


def lattice_launch(p, s, k, third, sun, jitter=0.0, n=LATTICE_N, checkerboard=0):
    """affine_launch for the lattice of step 0.25 s around p: component a = (k + 1) % 3 is p[a] + step (px - n / 2), component b = (k + 2) % 3
    is p[b] + step (py - n / 2).  With p on integers and s a power of two the construction is exact"""
    a, b = (k + 1) % 3, (k + 2) % 3
    step = 0.25 * float(s)
    return affine_launch(p, step * np.eye(3)[a], step * np.eye(3)[b], k, third, sun, jitter, n, checkerboard)


GRAZE_SUNS = ((1, 3, 5), (-3, 1, -5), (3, -2, 7), (-1, -2, 3))  # (a, b, k) components: nothing about them is exact once normalised


def graze_launch(p, s, k, sun_abk, n=LATTICE_N, checkerboard=0):
    """a launch whose every ray, in exact arithmetic, passes through one SILHOUETTE edge of the box [-1, 1]^3 s + p: the edge along k at the
    corner (sign(da), -sign(db)) of the other two axes, where the face a = +-1 is left and the face b = -+1 would be entered.  Pixel px sets
    the distance u = (px + 1) / 8 back from the edge along the direction, py where along the edge the ray passes.  The normalised direction
    and Sx, Sy are rounded, so the fp32 products of U, V, W nearly cancel: where they cancel to exactly 0, T's fp64 branch finds the sign"""
    a, b = (k + 1) % 3, (k + 2) % 3
    da, db, dk = (float(v) for v in sun_abk)
    p = np.asarray(p, np.float64)
    corner = np.zeros(3)
    corner[a], corner[b] = np.sign(da), -np.sign(db)
    step = np.zeros(3)
    step[a], step[b] = -da * s / 8, -db * s / 8
    base = p + s * corner + step * (n // 2 + 1)  # px = n / 2: u = (n / 2 + 1) / 8
    px, py = np.meshgrid(np.arange(n), np.arange(n))
    third = p[k] + s * (((py - n // 2) / 16 + 1 / 32) - dk * (px + 1) / 8)
    sun = np.zeros(3)
    sun[a], sun[b], sun[k] = da, db, dk
    return affine_launch(base, step, np.zeros(3), k, third, sun, 0.0, n, checkerboard)


def lattice_points(p, s, k, third, n=LATTICE_N):
    """the origins lattice_launch intends, (n, n, 3) in fp64"""
    a, b = (k + 1) % 3, (k + 2) % 3
    px, py = np.meshgrid(np.arange(n), np.arange(n))
    o = np.zeros((n, n, 3))
    o[..., a], o[..., b] = float(p[a]) + 0.25 * float(s) * (px - n // 2), float(p[b]) + 0.25 * float(s) * (py - n // 2)
    o[..., k] = np.broadcast_to(np.asarray(third, np.float32), (n, n))
    return o


AXIS_STARTS = (-3.0, -1.0, 0.0, 1.0)          # x s: in front of the instance, on its planes, inside it (degenerate_rays' starts)
AXIS_JITTERS = (0.0, 1e-2, 1e-30, 1e-42)      # 1e-42 is an fp32 denormal: a direction component, and Sx, Sy of T, that a flush would erase
DIAG_SUNS = ((1, 1, 0), (1, -1, 0), (0, 1, 1), (1, 0, -1), (1, 1, 1), (1, 1e-20, 0), (1, 1e-40, 1e-42))
DIAG_THIRDS = (-4, -2, 0, 2, 4)               # x 0.25 s
BAD_SUNS = ((0, 0, 0), (0, np.nan, 1), (np.inf, 0, 1), (0, 1, -np.inf), (3e38, 3e38, 3e38), (1e-30, 0, 0), (1e-45, 0, 0))
ODD_DEPTHS = (np.nan, np.inf, -np.inf, 3e38, -0.0, 1e-40)


def odd_depth_image(finite, n=LATTICE_N):
    """an (n, n) depth image: the texels whose index is 0 .. 5 modulo 12 hold NaN, +inf, -inf, 3e38, -0.0 and 1e-40, the others `finite`.
    A non-finite texel makes the whole origin non-finite (0 x inf in the rows that do not carry it)"""
    depth = np.full(n * n, finite, np.float32)
    for j, v in enumerate(ODD_DEPTHS):
        depth[j::12] = v
    return depth.reshape(n, n)


def degenerate_launches(scene, instances=None, checkerboard=0, families=("axis", "diag", "origins", "suns", "graze")):
    """the degenerate rays as launches around every instance of the scene (or those listed): a list of (name, sd, depth).  The name starts
    with its family: "axis" (k, sign, start, jitter), "diag" (the diagonal and nearly-axis suns), "origins" (a depth image that mixes
    odd_depth_image's texels among finite ones), "suns" (directions that normalise to something non-finite, or to zero) and "graze"
    (graze_launch: rays along a silhouette edge of the instance's box)"""
    out = []
    axes = np.eye(3)
    for i in range(len(scene["draws"])) if instances is None else instances:
        dr = scene["draws"][i]
        p, s = dr["position"].astype(np.float64), float(dr["scale"])
        if "axis" in families:
            for k in range(3):
                for sign in (1.0, -1.0):
                    for start in AXIS_STARTS:
                        for jitter in AXIS_JITTERS:
                            name = "axis jitter %g: instance %d k %d sign %+d start %g" % (jitter, i, k, sign, start)
                            out.append((name,) + lattice_launch(p, s, k, p[k] + sign * start * s, axes[k] * sign, jitter, checkerboard=checkerboard))
        if "diag" in families:
            for k in range(3):
                for sun in DIAG_SUNS:
                    for third in DIAG_THIRDS:
                        name = "diag: instance %d k %d sun %s third %d" % (i, k, sun, third)
                        out.append((name,) + lattice_launch(p, s, k, p[k] + third * 0.25 * s, sun, checkerboard=checkerboard))
        if "origins" in families:
            out.append(("origins: instance %d" % i,) + lattice_launch(p, s, 2, odd_depth_image(p[2] - 3.0 * s), axes[2], checkerboard=checkerboard))
        if "suns" in families:
            for sun in BAD_SUNS:
                out.append(("suns: instance %d sun %s" % (i, sun),) + lattice_launch(p, s, 2, p[2] - 3.0 * s, sun, checkerboard=checkerboard))
        if "graze" in families:
            for k in range(3):
                for sun in GRAZE_SUNS:
                    out.append(("graze: instance %d k %d sun %s" % (i, k, sun),) + graze_launch(p, s, k, sun, checkerboard=checkerboard))
    return out


def family(name):
    return name.split(":")[0]


POISON = 0x5A  # the byte the masks hold before a launch: neither 0 nor 255


def in_threads(f, items, threads=8):
    """[f(item)] in order; the restatements are plain C behind ctypes (the lock is released during a call) and share nothing they write"""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(threads) as pool:
        return list(pool.map(f, items))


def reference_masks(shref, scene, launches, quality):
    """(launches, n, n) u8: the restatement's pass over a poisoned mask for every launch"""
    return np.stack(in_threads(lambda l: shref.shadow_trace(l[1], scene, l[2], np.full(l[2].shape, POISON, np.uint8), quality), launches))


def launch_rays(shref, launches):
    """(origins, dirs, families): the rays of every pixel of every launch, (launches * n * n, 3) each, and the family of each ray"""
    rays = [shref.rays(sd, depth) for _, sd, depth in launches]
    fam = np.repeat([family(name) for name, _, _ in launches], [r[0].shape[0] * r[0].shape[1] for r in rays])
    return np.concatenate([r[0].reshape(-1, 3) for r in rays]), np.concatenate([r[1].reshape(-1, 3) for r in rays]), fam


def in_chunks(f, o, d, chunk=1 << 14):
    """f(origins, dirs) -> an array per ray, over chunks of the rays in threads"""
    return np.concatenate(in_threads(lambda i: f(o[i:i + chunk], d[i:i + chunk]), range(0, len(o), chunk)))


def input_conditions(name, o, d, fam, masks):
    """the conditions under which equality on the degenerate launches is not vacuous, asserted on the RESTATEMENT's masks alone (masks:
    quality -> the mask of every ray of launch_rays).  Prints each count before it asserts"""
    finite = np.isfinite(o).all(1) & np.isfinite(d).all(1)
    for q, want in sorted(masks.items()):
        a0, a42 = want[fam == "axis jitter 0"], want[fam == "axis jitter 1e-42"]
        dark, lit, erased = int((a0 == 0).sum()), int((a0 == 255).sum()), int((a0 != a42).sum())
        print("%s quality %d: axis jitter 0: %d rays, %d occluded, %d lit; the jitter 1e-42 masks differ from them in %d texels" % (name, q, a0.size, dark, lit, erased))
        print("%s quality %d: %d non-finite rays, %d of them lit; %d rays of the bad suns, %d lit" % (name, q, int((~finite).sum()), int((want[~finite] == 255).sum()),
                                                                                                 int((fam == "suns").sum()), int((want[fam == "suns"] == 255).sum())))
        for f in sorted(set(fam.tolist())):
            print("%s quality %d: %-18s %7d rays, %6d occluded, %5d non-finite" % (name, q, f, int((fam == f).sum()), int((want[fam == f] == 0).sum()), int((~finite[fam == f]).sum())))
        assert dark >= 1000 and lit >= 1000
        assert erased >= 200  # what a denormal flush would erase
        assert (~finite).sum() >= 100 and (want[~finite] == 255).all()
        assert (want[fam == "suns"] == 255).all()
        assert set(np.unique(want).tolist()) == {0, 255}


def closed_box_launches(scene):
    """(the scene of instance 0 alone, which is the unit box at the origin; the six axis launches from outside it with jitter 0)"""
    d = scene["draws"][0]
    assert d["position"].tolist() == [0.0, 0.0, 0.0] and float(d["scale"]) == 1.0 and int(d["meshIndex"]) == 1 and int(d["postPass"]) == 0
    alone = dict(scene, draws=scene["draws"][:1])
    launches = [l for l in degenerate_launches(alone, families=("axis",)) if l[0].startswith("axis jitter 0:") and l[0].endswith("start -3")]
    assert len(launches) == 6
    return alone, launches


def closed_box_property(name, masks):
    """from outside, a ray through a shared edge or vertex of the closed box is not lost between its triangles: the texels whose lattice
    point lies in the closed face are 0, the others 255"""
    face = closed_face()
    masks = np.asarray(masks)
    print("%s: closed box: %d launches, %d texels in the closed face of each, %d of them occluded; %d outside it, %d of them lit" % (
        name, len(masks), int(face.sum()), int((masks[:, face] == 0).sum()), int((~face).sum()), int((masks[:, ~face] == 255).sum())))
    assert face.sum() == 81 and (masks[:, face] == 0).all() and (masks[:, ~face] == 255).all()


def extreme_scene():
    """aligned_scene plus five box instances at integer positions 16 and more apart (their lattices do not meet): 3 = the singular map
    (orientation (fp32(sqrt(1/2)), 0, 0, 0): rotateQuat projects onto x and the instance gets the "everything" TLAS box), 4 = the zero
    quaternion (the identity map), 5 = scale 2^-120 (the object-space ray overflows: eps and tau are not finite, nothing is culled), 6 = scale
    2^100 (a box that holds every other lattice), 7 = orientation (0.5, 0.5, 0.5, 0.5), an exact turn by 120 degrees"""
    base = aligned_scene()
    draws = np.zeros(8, dtype=L.MESHDRAW)
    draws[:3] = base["draws"]
    draws["orientation"][3:] = [(np.sqrt(0.5), 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0, 1.0), (0.5, 0.5, 0.5, 0.5)]
    draws["position"][3:] = [(0.0, 16.0, 0.0), (16.0, 16.0, 0.0), (0.0, -16.0, 0.0), (-16.0, -16.0, 8.0), (16.0, -16.0, -8.0)]
    draws["scale"][3:] = (1.0, 1.0, 2.0 ** -120, 2.0 ** 100, 1.0)
    draws["meshIndex"][3:] = 1
    draws["postPass"][3:] = (0, 1, 0, 1, 0)
    return dict(base, draws=draws)


def moved_exactly(scene):
    """the draws of aligned_scene or extreme_scene moved by exact amounts (integer positions, power-of-two scales): the lattices of
    degenerate_launches stay exact"""
    draws = scene["draws"].copy()
    draws["position"][:3] = [(2.0, 0.0, -1.0), (-8.0, 4.0, 4.0), (6.0, -2.0, 3.0)]
    draws["scale"][:3] = (2.0, 1.0, 0.5)
    draws["position"][3:] += np.array([4.0, -8.0, 32.0], np.float32)
    return draws


def infinite_leaves(nodes):
    """the TLAS leaves (tlas_ref.sections' nodes) whose box is (-inf, +inf) on every axis"""
    return np.flatnonzero((nodes["leaf"] != 0) & np.isneginf(nodes["lo"]).all(1) & np.isposinf(nodes["hi"]).all(1))


def closed_face(n=LATTICE_N):
    """the texels of an axis launch around the unit box at the origin whose lattice point lies in the box's closed face: |a|, |b| <= 1"""
    g = 0.25 * (np.arange(n) - n // 2)
    return (np.abs(g)[None, :] <= 1.0) & (np.abs(g)[:, None] <= 1.0)


load.__test__ = False
