"""ctypes loader of tests/visattr_ref.c, the CPU restatement of nv_visibility_attributes (test infrastructure), and the helpers that give
the synthetic scenes something to interpolate: packed normals, tangents and texcoords for their vertices and a material table.

`load(directory)` compiles the restatement there twice, with raster_ref.c's flags: as fp32 (the bits the kernel must write) and with
-DREAL=double (the same statements in fp64: the yardstick of the accuracy checks).  AttrRef.attributes(..., real="f32" / "f64")."""
import ctypes as C
import os
import subprocess

import numpy as np

import raster_ref as RR
from niagara_amd import layouts as L

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "visattr_ref.c")
SHADED, INVALID, DEGENERATE, CLIPPED, TEXTURED = 1, 2, 4, 8, 16
VALS = ("uv", "bary", "normal", "tangent", "wpos")  # the 14 values per pixel, in NvPixelAttributes' order without its two integer words
_SLICES = dict(uv=slice(0, 2), bary=slice(2, 4), normal=slice(4, 7), tangent=slice(7, 11), wpos=slice(11, 14))


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class AttrRef:
    def __init__(self, so32, so64):
        self.libs = {"f32": C.CDLL(so32), "f64": C.CDLL(so64)}
        for k, size in (("f32", 4), ("f64", 8)):
            self.libs[k].va_attributes.restype = None
            assert self.libs[k].va_real_bytes() == size

    def attributes(self, g, records, width, height, draws, meshlets, data, vertices, materials=None, real="f32", counts=None):
        """dict: vals (h * w, 14) of `real`, ids (h * w, 2) u32 {drawId, materialIndex}, gbuffer0 / gbuffer1 (h * w) u32, totals (4) u64, flags
        (h * w) u8 (SHADED | INVALID | DEGENERATE | CLIPPED | TEXTURED), chan (h * w, 8): the G-buffer channels before the pack; and, for
        real = "f32", attributes: the (h * w) PIXELATTR records.  counts: {"draws" / "meshlets" / "data" / "vertices" / "materials": n} overrides
        a capacity (the validation tests)"""
        rt = np.float32 if real == "f32" else np.float64
        n = width * height
        records = np.ascontiguousarray(records, L.VISRECORD).reshape(-1)
        assert len(records) == n
        draws, meshlets = np.ascontiguousarray(draws, L.MESHDRAW), np.ascontiguousarray(meshlets, L.MESHLET)
        data, vertices = np.ascontiguousarray(data, np.uint32), np.ascontiguousarray(vertices, L.VERTEX)
        mats = None if materials is None else np.ascontiguousarray(materials, L.MATERIAL)
        cnt = dict(draws=len(draws), meshlets=len(meshlets), data=len(data), vertices=len(vertices), materials=0 if mats is None else len(mats))
        cnt.update(counts or {})
        out = dict(vals=np.zeros((n, 14), rt), ids=np.zeros((n, 2), np.uint32), gbuffer0=np.zeros(n, np.uint32), gbuffer1=np.zeros(n, np.uint32),
                   totals=np.zeros(4, np.uint64), flags=np.zeros(n, np.uint8), chan=np.zeros((n, 8), rt))
        one = lambda a, dt: a if len(a) else np.zeros(1, dt)
        self.libs[real].va_attributes(_p(np.ascontiguousarray(g)), _p(records), C.c_uint32(width), C.c_uint32(height), _p(one(draws, L.MESHDRAW)),
                                      C.c_uint32(cnt["draws"]), _p(one(meshlets, L.MESHLET)), C.c_uint32(cnt["meshlets"]), _p(one(data, np.uint32)),
                                      C.c_uint32(cnt["data"]), _p(one(vertices, L.VERTEX)), C.c_uint32(cnt["vertices"]), _p(mats),
                                      C.c_uint32(cnt["materials"]), _p(out["vals"]), _p(out["ids"]), _p(out["gbuffer0"]), _p(out["gbuffer1"]),
                                      _p(out["totals"]), _p(out["flags"]), _p(out["chan"]))
        for name, sl in _SLICES.items():
            out[name] = out["vals"][:, sl]
        if real == "f32":
            a = np.zeros(n, L.PIXELATTR)
            for name in VALS:
                a[name] = out[name]
            a["drawId"], a["materialIndex"] = out["ids"][:, 0], out["ids"][:, 1]
            out["attributes"] = a
        return out


def load(directory):
    so32, so64 = (os.path.join(str(directory), "libvisattr_ref_%s.so" % k) for k in ("f32", "f64"))
    for so, extra in ((so32, []), (so64, ["-DREAL=double"])):
        if not os.path.exists(so):
            subprocess.check_call(["gcc"] + RR.FLAGS + extra + ["-Wall", "-Wno-unused-function", "-shared", "-fPIC", "-I", HERE, "-o", so, SRC, "-lm"])
    return AttrRef(so32, so64)


# ---- attributes for the synthetic scenes

def _encode_oct(v):
    """src/shaders/math.h:52-58 in fp64"""
    v = v / np.abs(v).sum(axis=1, keepdims=True)
    s = np.where(v[:, :2] >= 0, 1.0, -1.0)
    return np.where(v[:, 2:3] <= 0, (1.0 - np.abs(v[:, 1::-1])) * s, v[:, :2])


def decode_oct(e):
    """src/shaders/math.h:60-67 in fp64"""
    e = np.asarray(e, np.float64)
    v = np.concatenate([e, 1.0 - np.abs(e[:, :1]) - np.abs(e[:, 1:2])], axis=1)
    t = np.maximum(-v[:, 2], 0.0)
    v[:, 0] += np.where(v[:, 0] >= 0, -t, t)
    v[:, 1] += np.where(v[:, 1] >= 0, -t, t)
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def fill_attributes(vertices, meshlets, data):
    """np, tp, tu and tv of every vertex the meshlets use, from real unit vectors: the normal is the area-weighted mean of the vertex's
    triangles' normals (mesh-local, counter-clockwise = outward), the tangent a unit vector perpendicular to it, packed as the asset
    pipeline packs them (10 bits per normal component, the tangent octahedral in 2 x 8 bits, bit 30 of np = a mirrored bitangent); the
    texcoord is a planar map of the position.  Returns a copy of `vertices`."""
    v = vertices.copy()
    pos = np.stack([v["vx"], v["vy"], v["vz"]], -1).view(np.float16).astype(np.float64)
    nrm = np.zeros_like(pos)
    d16, d8 = data.view(np.uint16), data.view(np.uint8)
    for m in meshlets:
        vc, tc, off, short = int(m["vertexCount"]), min(int(m["triangleCount"]), 96), int(m["dataOffset"]), m["shortRefs"] == 1
        refs = (d16[off * 2:off * 2 + vc] if short else data[off:off + vc]).astype(np.int64) + int(m["baseVertex"])
        io = (off + ((vc + 1) // 2 if short else vc)) * 4
        idx = d8[io:io + 3 * tc].reshape(-1, 3).astype(np.int64)
        idx = idx[(idx < min(vc, 64)).all(axis=1)]
        tri = refs[idx]
        fn = np.cross(pos[tri[:, 1]] - pos[tri[:, 0]], pos[tri[:, 2]] - pos[tri[:, 0]])
        for k in range(3):
            np.add.at(nrm, tri[:, k], fn)
    ln = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where(ln > 1e-12, nrm / np.maximum(ln, 1e-300), np.array([0.0, 0.0, 1.0]))
    axis = np.eye(3)[np.argmin(np.abs(nrm), axis=1)]  # the axis the normal is least aligned with
    tan = np.cross(axis, nrm)
    tan /= np.linalg.norm(tan, axis=1, keepdims=True)
    q = np.clip(np.rint((nrm + 1.0) * 511.0), 0, 1022).astype(np.uint32)
    mirrored = (pos[:, 0] + pos[:, 1] + pos[:, 2] < 0).astype(np.uint32)  # by region: a triangle mostly has one sign
    v["np"] = q[:, 0] | q[:, 1] << 10 | q[:, 2] << 20 | mirrored << 30
    e = np.clip(np.rint((_encode_oct(tan) + 1.0) * 127.0), 0, 254).astype(np.uint16)
    v["tp"] = e[:, 0] | e[:, 1] << 8
    uv = np.stack([pos[:, 0] + 0.25 * pos[:, 2], pos[:, 1] - 0.25 * pos[:, 2]], -1) * 0.5 + 0.5
    h = uv.astype(np.float16)
    v["tu"], v["tv"] = h[:, 0].view(np.uint16), h[:, 1].view(np.uint16)
    return v


def make_materials(n=5):
    """a material table of n >= 4 entries; entry 2 names textures (the library shades it from its factors and counts its pixels)"""
    rng = np.random.default_rng(12)
    m = np.zeros(n, L.MATERIAL)
    m["diffuseFactor"] = rng.uniform(0.05, 1.0, (n, 4)).astype(np.float32)
    m["specularFactor"] = rng.uniform(0.0, 1.0, (n, 4)).astype(np.float32)
    m["emissiveFactor"] = rng.uniform(0.0, 2.0, (n, 3)).astype(np.float32) * (np.arange(n) % 2)[:, None]
    m["diffuseFactor"][0] = (1.0, 0.0, 0.5, 1.0)  # the ends of the range
    m[2]["albedoTexture"], m[2]["normalTexture"], m[2]["specularTexture"], m[2]["emissiveTexture"] = 3, 4, 0, 7
    return m


def with_attributes(scene, n_materials=5):
    """a copy of a synth scene dict with its vertices' attribute fields filled, draws spread over a material table ("materials")"""
    s = dict(scene)
    s["vertices"] = fill_attributes(scene["vertices"], scene["meshlets"], scene["data"])
    s["draws"] = scene["draws"].copy()
    s["draws"]["materialIndex"] = np.arange(len(s["draws"])) % n_materials
    s["materials"] = make_materials(n_materials)
    return s


def kitten_scene(viewport=(320, 192), n_draws=7, meshlet_bounds=None):
    """niagara's own asset (tests/golden/mesh/kitten.npz) as a scene of the closed loop: one mesh of one LOD, its faces cut into meshlets in
    Morton order of their centroids, `n_draws` instances at several sizes and orientations in front of the default camera"""
    from meshlet_builder import build_meshlets
    from niagara_amd import host
    k = np.load(os.path.join(HERE, "golden", "mesh", "kitten.npz"))
    pos, faces = k["positions"], k["corners"][:, 0].astype(np.int64).reshape(-1, 3)
    cen = pos[faces].mean(axis=1)
    g = np.clip(((cen - cen.min(0)) / (np.ptp(cen, axis=0) + 1e-9) * 1023).astype(np.int64), 0, 1023)

    def spread(v):
        v = (v | (v << 16)) & 0x030000FF
        v = (v | (v << 8)) & 0x0300F00F
        v = (v | (v << 4)) & 0x030C30C3
        return (v | (v << 2)) & 0x09249249
    order = np.argsort(spread(g[:, 0]) | (spread(g[:, 1]) << 1) | (spread(g[:, 2]) << 2), kind="stable")
    meshlets, data, vertices = build_meshlets(pos, faces[order])
    meshlet_bounds(vertices, data, meshlets)
    hp = pos.astype(np.float16).astype(np.float32)
    meshes = np.zeros(1, L.MESH)
    meshes[0]["center"], meshes[0]["radius"] = host.mesh_bounds(hp)
    meshes[0]["vertexCount"], meshes[0]["lodCount"] = len(pos), 1
    meshes[0]["lods"][0]["meshletCount"], meshes[0]["lods"][0]["indexCount"] = len(meshlets), 3 * len(faces)
    radius = float(meshes[0]["radius"])
    rng = np.random.default_rng(31)
    draws = np.zeros(n_draws, L.MESHDRAW)
    for i in range(n_draws):
        q = rng.normal(size=4)
        draws[i]["orientation"] = q / np.linalg.norm(q)
        draws[i]["scale"] = (1.7 if i == 0 else rng.uniform(0.7, 1.2)) / radius
        draws[i]["position"] = (0.0, 0.0, -2.2) if i == 0 else (rng.uniform(-3.0, 3.0), rng.uniform(-1.5, 1.5), -rng.uniform(3.0, 6.0))
    slots, _ = host.assign_visibility_offsets(draws, meshes)
    pw, ph = host.previous_pow2(viewport[0]), host.previous_pow2(viewport[1])
    cd = host.build_cull_data(viewport=viewport, pyramid=(pw, ph), draw_count=n_draws, cullingEnabled=1, lodEnabled=1, occlusionEnabled=1,
                              clusterOcclusionEnabled=1, clusterBackfaceEnabled=1)
    return dict(meshes=meshes, meshlets=meshlets, draws=draws, data=data, vertices=vertices, cull=cd, viewport=viewport, slots=slots)


def reference_frame(scene, near_clip, vref, aref, frames=2, materials=True):
    """The closed-loop frame on the CPU through the existing references (visbuffer_ref.oracle_frames with the post pass, then its resolve),
    then the attribute pass: (the last frame's record with "resolve" added, the f32 attribute output)"""
    import visbuffer_ref as VB
    rec = VB.oracle_frames(scene, frames, True, vref, near_clip)[-1]
    rec["resolve"] = vref.resolve(scene["cull"], rec["visibility"], rec["draws"], scene["meshes"], len(rec["post"]["mvb"]))
    w, h = scene["viewport"]
    g = RR.globals_for(scene["cull"], (w, h))
    out = aref.attributes(g, rec["resolve"]["records"], w, h, rec["draws"], scene["meshlets"], scene["data"], scene["vertices"],
                          scene["materials"] if materials else None)
    return rec, out
