"""oracle.ref — ctypes binding over oracle/_ref/libniagara_ref.so: the reference's own shader sources
(translated syntactically by oracle/ref_translate.py) executing on the CPU.  TEST INFRASTRUCTURE ONLY.

The library is built by `make -C oracle ref` where /root/reference exists; the prebuilt .so travels to the
GPU box with the snapshot.  available() is False when neither is possible.
"""
import ctypes as C
import os

import numpy as np

_SO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_ref", "libniagara_ref.so")
_lib = None


def available():
    return os.path.exists(_SO)


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(_SO)
        _lib.ref_occlusion_mip.restype = C.c_float
        _lib.ref_sizeof.restype = C.c_uint32
        _lib.ref_previous_pow2.restype = C.c_uint32
        _lib.ref_image_mip_levels.restype = C.c_uint32
        _lib.ref_rand32.restype = C.c_uint32
        _lib.ref_rand01.restype = C.c_double
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _pyr(p):
    return None if p is None else p.ref()  # same struct layout as oracle.Pyramid


def drawcull(cd, late, task, draws, meshes, commands, count4, dvb, pyr=None):
    lib().ref_drawcull(_p(cd), int(late), int(task), _p(draws), _p(meshes), _p(commands), _p(count4), _p(dvb), _pyr(pyr))


def tasksubmit(count4, commands):
    lib().ref_tasksubmit(_p(count4), _p(commands))


def clustercull(cd, late, commands, count4, draws, meshlets, mvb, pyr, cib, cc4):
    lib().ref_clustercull(_p(cd), int(late), _p(commands), _p(count4), _p(draws), _p(meshlets), _p(mvb), _pyr(pyr), _p(cib), _p(cc4))


def meshlet_mesh(globals_, commands, draws, meshlets, meshlet_data, vertices, cib, cc4, masks, totals3):
    """src/shaders/meshlet.mesh.glsl (MESH_CULL = 1, TASK = false) over the grid in cc4; see oracle/ref_runner.cpp"""
    lib().ref_meshlet_mesh(_p(globals_), _p(commands), _p(draws), _p(meshlets), _p(meshlet_data), _p(vertices), _p(cib), _p(cc4), _p(masks),
                           C.c_uint32(len(masks)), _p(totals3))


def meshlet_task(cd, late, commands, count4, draws, meshlets, mvb, pyr, payloads, payload_counts):
    """src/shaders/meshlet.task.glsl (TASK_CULL = 1) over the grid in count4; see oracle/ref_runner.cpp"""
    lib().ref_meshlet_task(_p(cd), int(late), _p(commands), _p(count4), _p(draws), _p(meshlets), _p(mvb), _pyr(pyr), _p(payloads), _p(payload_counts))


def mesh_bounds(positions):
    """src/scene.cpp:207-220 (mean centre, max distance) over an (n, 3) float32 array -> (center[3], radius)"""
    import numpy as np
    pos = np.ascontiguousarray(positions, np.float32)
    center, radius = np.zeros(3, np.float32), np.zeros(1, np.float32)
    lib().ref_mesh_bounds(_p(pos), C.c_uint32(len(pos)), _p(center), _p(radius))
    return center, radius[0]


def clustersubmit(cc4, cib):
    lib().ref_clustersubmit(_p(cc4), _p(cib))


def depthreduce(depth, pyr):
    h, w = depth.shape
    offs = (C.c_uint32 * 16)(*pyr.mip_offset)
    lib().ref_depthreduce(_p(depth), C.c_uint32(w), C.c_uint32(h), _p(pyr.data), C.c_uint32(pyr.width), C.c_uint32(pyr.height),
                          C.c_uint32(pyr.levels), offs)


def rotate_quat(v, q):
    out = np.zeros(3, np.float32)
    lib().ref_rotate_quat(_p(np.asarray(v, np.float32)), _p(np.asarray(q, np.float32)), _p(out))
    return out


def project_sphere(c, r, znear, p00, p11):
    aabb = np.zeros(4, np.float32)
    ok = lib().ref_project_sphere(_p(np.asarray(c, np.float32)), C.c_float(r), C.c_float(znear), C.c_float(p00), C.c_float(p11), _p(aabb))
    return bool(ok), aabb


def occlusion_mip(aabb, pw, ph):
    return float(lib().ref_occlusion_mip(_p(np.asarray(aabb, np.float32)), C.c_float(pw), C.c_float(ph)))


def cone_cull(c, r, axis, cutoff):
    return bool(lib().ref_cone_cull(_p(np.asarray(c, np.float32)), C.c_float(r), _p(np.asarray(axis, np.float32)), C.c_float(cutoff)))


# ---- the reference's scene-cache code (src/scenecache.cpp compiled in place, oracle/ref_scenecache.cpp) ----
def scene_sizeof(what):
    lib().ref_scene_sizeof.restype = C.c_uint32
    return int(lib().ref_scene_sizeof(int(what)))


def save_scene_cache(path, meshes, meshlets, draws, *, vertex_count=100, index_count=300, meshletdata_count=500, meshletvtx0_count=64,
                     material_count=3, light_count=2, animation_count=1, keyframe_count=4, texture_paths=2,
                     camera=((1.0, 2.0, 3.0), (0.0, 0.0, 0.0, 1.0), 1.2, 0.5), sun=(0.0, -1.0, 0.0), hash_meta=0x1122334455667788, clrt_mode=False,
                     omm_states=0):
    """saveSceneCache (src/scenecache.cpp:120-260) itself, uncompressed (the codecs are meshoptimizer's: not vendored)"""
    cam = np.array(list(camera[0]) + list(camera[1]) + [camera[2], camera[3]], np.float32)
    s3 = np.array(sun, np.float32)
    rc = lib().ref_save_scene_cache(os.fsencode(str(path)), _p(np.ascontiguousarray(meshes)), C.c_uint32(len(meshes)), _p(np.ascontiguousarray(meshlets)),
                                    C.c_uint32(len(meshlets)), _p(np.ascontiguousarray(draws)), C.c_uint32(len(draws)), C.c_uint32(vertex_count),
                                    C.c_uint32(index_count), C.c_uint32(meshletdata_count), C.c_uint32(meshletvtx0_count), C.c_uint32(material_count),
                                    C.c_uint32(light_count), C.c_uint32(animation_count), C.c_uint32(keyframe_count), C.c_uint32(texture_paths), _p(cam), _p(s3),
                                    C.c_uint64(hash_meta), int(bool(clrt_mode)), C.c_uint32(omm_states))
    if rc:
        raise RuntimeError("saveSceneCache failed")


def load_scene_cache(path, mesh_dtype, meshlet_dtype, draw_dtype, hash_meta=0x1122334455667788, clrt_mode=False, omm_states=0):
    """loadSceneCache (src/scenecache.cpp:273-370) itself -> (meshes, meshlets, draws, camera9, sun3), or None if it rejects the file"""
    counts, cam, sun = np.zeros(3, np.uint32), np.zeros(9, np.float32), np.zeros(3, np.float32)
    rc = lib().ref_load_scene_cache(os.fsencode(str(path)), C.c_uint64(hash_meta), int(bool(clrt_mode)), int(omm_states), _p(counts), _p(cam), _p(sun))
    if rc:
        return None
    meshes, meshlets, draws = np.zeros(counts[0], mesh_dtype), np.zeros(counts[1], meshlet_dtype), np.zeros(counts[2], draw_dtype)
    lib().ref_loaded_arrays(_p(meshes), _p(meshlets), _p(draws))
    return meshes, meshlets, draws, cam, sun


# ---- the shading end of the frame (shadowfill, shadowblur, final, bloom, mesh.frag and the helpers of src/shaders/math.h:51-109) ----
def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def stats(shader):
    """the shim's counters of `shader` ("shadowfill", "shadowblur", "final", "bloom") since the last call: dict(outside: fetches outside the
    image, dropped: stores outside it, dropped_at_width: those with x == width, edges: texture() taps clamped left / right / top / bottom)"""
    out = np.zeros(7, np.uint32)
    getattr(lib(), "ref_stats_" + shader)(_p(out))
    return dict(outside=int(out[0]), dropped=int(out[1]), dropped_at_width=int(out[2]), edges=out[3:].astype(np.int64))


def shadow_fill(shadow, depth, checkerboard):
    """shadowfill.comp.glsl over its dispatch, in place on a copy -> (filled (h, w) u8, handed (h, w, 4) f32: the vec4 each store was given,
    zeros where nothing was stored)"""
    h, w = shadow.shape
    s, d = np.ascontiguousarray(shadow, np.uint8).copy(), _f32(depth).reshape(h, w)
    handed = np.zeros((h, w, 4), np.float32)
    lib().ref_shadowfill(_p(s), _p(d), C.c_uint32(w), C.c_uint32(h), C.c_int(checkerboard), _p(handed))
    return s, handed


def shadow_blur(shadow, depth, direction, znear):
    """shadowblur.comp.glsl (BLUR 1) -> (out (h, w) u8, handed (h, w, 4) f32)"""
    h, w = shadow.shape
    s, d = np.ascontiguousarray(shadow, np.uint8), _f32(depth).reshape(h, w)
    out, handed = np.zeros((h, w), np.uint8), np.zeros((h, w, 4), np.float32)
    lib().ref_shadowblur(_p(out), _p(s), _p(d), C.c_uint32(w), C.c_uint32(h), C.c_float(direction), C.c_float(znear), _p(handed))
    return out, handed


def final(sd, gbuffer0, gbuffer1, depth, shadow=None, bloom0=None):
    """final.comp.glsl -> (colour (h, w) u32, handed (h, w, 4) f32).  sd: the 112-byte ShadeData record; bloom0: level 0 of the bloom target
    ((h + 1) // 2, (w + 1) // 2) u32, all zero when None"""
    h, w = depth.shape
    sdw = np.frombuffer(np.ascontiguousarray(sd).tobytes(), np.float32).copy()
    g0 = np.ascontiguousarray(gbuffer0).view(np.uint32).reshape(h, w)
    g1 = np.ascontiguousarray(gbuffer1).view(np.uint32).reshape(h, w)
    b = np.zeros(((h + 1) // 2, (w + 1) // 2), np.uint32) if bloom0 is None else np.ascontiguousarray(bloom0, np.uint32)
    s = None if shadow is None else np.ascontiguousarray(shadow, np.uint8).reshape(h, w)
    out, handed = np.zeros((h, w), np.uint32), np.zeros((h, w, 4), np.float32)
    lib().ref_final(_p(sdw), _p(g0), _p(g1), _p(_f32(depth)), _p(s), _p(b), C.c_uint32(b.shape[1]), C.c_uint32(b.shape[0]), _p(out), C.c_uint32(w),
                    C.c_uint32(h), _p(handed))
    return out, handed


RAY_INFO = ("queries", "flags", "opaque_commits", "candidates", "confirmed", "committed_instance")


def has_shadow():
    """True when the built library holds shadow.comp.glsl.  One built before that shader was translated does not: an out-of-date build, which
    tests/test_shadow_vs_ref.py reports as a failure that names `make -C oracle ref`, not as a skip"""
    return available() and hasattr(lib(), "ref_shadow")


def shadow(sd, depth, meshes, indices, vertices, draws, materials=None, textures=None, quality=0, prefill=0):
    """shadow.comp.glsl over its dispatch (src/niagara.cpp:1797-1817) against the CPU ray query of oracle/glsl_rayquery_shim.h.  sd: the 96-byte
    ShadowData record; meshes / draws / vertices / materials in the C ABI's layouts (208 / 48 / 16 / 64 bytes); textures: None, or a dict with
    "descs" (four words per texture: offset, width, height, levels; entry 0 reserved) and "texels" (uint32, decoded RGBA8).  Returns a dict:
      mask    (h, w) u8      texels no invocation stored to keep the prefill byte
      handed  (h, w, 4) f32  the vec4 given to each store (zeros where nothing was stored)
      rays    (h, w, 8) f32  origin, direction, tmin, tmax of the storing invocation's query
      queries, flags, opaque_commits, candidates, confirmed, committed_instance  (h, w) u32 each; rejected = candidates - confirmed;
              queries == 0 where no invocation stored; committed_instance is 0xffffffff where nothing was committed
      samples (n, 8) f32     id, u, v, the alpha returned, and the candidate's instance, primitive and barycentrics, of every textureLod call in
              order
      dropped, dropped_at_width  stores outside the image, and those of them with x == width inside the rows"""
    h, w = depth.shape
    sdw = np.frombuffer(np.ascontiguousarray(sd).tobytes(), np.float32).copy()
    assert sdw.size == 24
    m, i, v, d = (np.ascontiguousarray(a) for a in (meshes, indices, vertices, draws))
    assert m.dtype.itemsize == 208 and v.dtype.itemsize == 16 and d.dtype.itemsize == 48 and i.dtype == np.uint32
    mt = np.zeros(0, np.dtype([("w", np.uint32, 16)])) if materials is None else np.ascontiguousarray(materials)
    assert mt.dtype.itemsize == 64
    descs = np.zeros(0, np.uint32) if textures is None else np.ascontiguousarray(textures["descs"]).view(np.uint32).reshape(-1, 4)
    texels = np.zeros(0, np.uint32) if textures is None else np.ascontiguousarray(textures["texels"], np.uint32)
    mask = np.full((h, w), prefill, np.uint8)
    handed, rays, info = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 8), np.float32), np.zeros((h, w, 6), np.uint32)
    room = 1 << 16
    while True:
        stats("shadow")  # reset the shim's counters
        samples, count = np.zeros((room, 8), np.float32), C.c_uint64(0)
        mask[...] = prefill
        lib().ref_shadow(_p(sdw), _p(_f32(depth)), C.c_uint32(w), C.c_uint32(h), _p(m), C.c_uint32(len(m)), _p(i), C.c_uint32(len(i)), _p(v), C.c_uint32(len(v)),
                         _p(d), C.c_uint32(len(d)), _p(mt), C.c_uint32(len(mt)), _p(descs), C.c_uint32(len(descs)), _p(texels), C.c_uint64(len(texels)),
                         C.c_int(quality), _p(mask), _p(handed), _p(rays), _p(info), _p(samples), C.c_uint64(room), C.byref(count))
        if count.value <= room:
            break
        room = int(count.value)
    st = stats("shadow")
    out = dict(mask=mask, handed=handed, rays=rays, samples=samples[:count.value], dropped=st["dropped"], dropped_at_width=st["dropped_at_width"])
    out.update({name: info[..., k] for k, name in enumerate(RAY_INFO)})
    return out


def bloom_pass(which, src, dst_shape, radius=0.0, dst=None):
    """one dispatch of bloom.comp.glsl: which 0 (src = gbuffer0 words), 1, 2 (src = a bloom level; dst = the level accumulated into)
    -> (level (h, w) u32, handed (h, w, 4) f32)"""
    s = np.ascontiguousarray(src).view(np.uint32)
    h, w = dst_shape
    d = np.zeros((h, w), np.uint32) if dst is None else np.ascontiguousarray(dst, np.uint32).copy()
    handed = np.zeros((h, w, 4), np.float32)
    lib().ref_bloom_pass(C.c_int(which), _p(s), C.c_uint32(s.shape[1]), C.c_uint32(s.shape[0]), C.c_int(1 if which == 0 else 0), _p(d), C.c_uint32(w),
                         C.c_uint32(h), C.c_float(radius), _p(handed))
    return d, handed


def bloom(gbuffer0, width, height, levels, offsets, total):
    """the loop of src/niagara.cpp:1873-1901 over one linear bloom target -> (total,) u32"""
    g0 = np.ascontiguousarray(gbuffer0).view(np.uint32)
    target, off = np.zeros(total, np.uint32), np.ascontiguousarray(offsets, np.uint32)
    lib().ref_bloom(_p(g0), C.c_uint32(g0.shape[1]), C.c_uint32(g0.shape[0]), _p(target), C.c_uint32(width), C.c_uint32(height), C.c_uint32(levels), _p(off))
    return target


def mesh_frag(records, width, draws, materials, taps=None, post=0):
    """mesh.frag.glsl per fragment of `records` (64-byte NvPixelAttributes) -> dict(gbuffer0, gbuffer1 (n) u32, discard (n) bool,
    written (n, 8) f32).  taps: (n, 4, 4) f32, the texel of the albedo / normal / specular / emissive slot per fragment"""
    rec = np.ascontiguousarray(records).reshape(-1)
    n = len(rec)
    assert rec.dtype.itemsize == 64 and draws.dtype.itemsize == 48 and materials.dtype.itemsize == 64
    dr, mt = np.ascontiguousarray(draws), np.ascontiguousarray(materials)
    t = None if taps is None else _f32(taps).reshape(n, 4, 4)
    g0, g1, disc, written = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros((n, 8), np.float32)
    lib().ref_mesh_frag(_p(rec), C.c_uint32(n), C.c_uint32(width), _p(dr), _p(mt), C.c_uint32(len(mt)), _p(t), C.c_int(post), _p(g0), _p(g1), _p(disc),
                        _p(written))
    return dict(gbuffer0=g0, gbuffer1=g1, discard=disc.astype(bool), written=written)


def encode_oct(v):
    v = _f32(v).reshape(-1, 3)
    out = np.zeros((len(v), 2), np.float32)
    lib().ref_encode_oct(_p(v), C.c_uint32(len(v)), _p(out))
    return out


def decode_oct(e):
    e = _f32(e).reshape(-1, 2)
    out = np.zeros((len(e), 3), np.float32)
    lib().ref_decode_oct(_p(e), C.c_uint32(len(e)), _p(out))
    return out


def _colour(which, c, width):
    c = _f32(c).reshape(-1, width)
    out = np.zeros_like(c)
    lib().ref_colour(C.c_int(which), _p(c), C.c_uint32(len(c)), _p(out))
    return out


def tosrgb(c):
    return _colour(0, c, 3)


def fromsrgb(c):
    return _colour(1, c, 3)


def tonemap(c):
    return _colour(2, c, 3)


def tosrgb4(c):
    return _colour(3, c, 4)


def fromsrgb4(c):
    return _colour(4, c, 4)


def gradient_noise(uv):
    uv = _f32(uv).reshape(-1, 2)
    out = np.zeros(len(uv), np.float32)
    lib().ref_gradient_noise(_p(uv), C.c_uint32(len(uv)), _p(out))
    return out


def unpack_tbn(np_codes, tp_codes):
    a, b = np.ascontiguousarray(np_codes, np.uint32).reshape(-1), np.ascontiguousarray(tp_codes, np.uint32).reshape(-1)
    assert len(a) == len(b)
    normal, tangent = np.zeros((len(a), 3), np.float32), np.zeros((len(a), 4), np.float32)
    lib().ref_unpack_tbn(_p(a), _p(b), C.c_uint32(len(a)), _p(normal), _p(tangent))
    return normal, tangent
