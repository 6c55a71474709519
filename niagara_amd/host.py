"""Host-side helpers (no device work): numpy views over the C ABI's host functions.

Mirrors the parts of niagara's main() that prepare cull inputs: CullData (src/niagara.cpp:1487-1516), the depth
pyramid geometry (:1340-1344), the synthetic scene (:969-998) and the visibility-slot prefix (:1002-1020).
"""
import ctypes as C
import os

import numpy as np

from . import layouts as L
from ._lib import BloomDesc, PyramidDesc, check, lib


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def previous_pow2(v):
    return int(lib.nv_previous_pow2(v))


def image_mip_levels(w, h):
    return int(lib.nv_image_mip_levels(w, h))


def pyramid_desc(depth_w, depth_h):
    d = PyramidDesc()
    check(lib.nv_pyramid_desc_init(C.byref(d), depth_w, depth_h), "nv_pyramid_desc_init")
    return d


def bloom_desc(width, height):
    """NvBloomDesc of a width x height image (src/niagara.cpp:1331-1333): half-resolution level 0, at most 8 levels, one linear buffer"""
    d = BloomDesc()
    check(lib.nv_bloom_desc_init(C.byref(d), int(width), int(height)), "nv_bloom_desc_init")
    return d


def build_cull_data(cam_pos=(0, 0, 0), cam_quat=(0, 0, 0, 1), fovy=float(np.radians(70.0)), znear=0.1, draw_distance=200.0,
                    viewport=(1024, 768), pyramid=(512, 512), draw_count=0, lod_step=0, **flags):
    """defaults = niagara's camera (src/niagara.cpp:836-837,1000,1184)"""
    cd = np.zeros(1, dtype=L.CULLDATA)
    pos = np.asarray(cam_pos, dtype=np.float32)
    q = np.asarray(cam_quat, dtype=np.float32)
    check(lib.nv_build_cull_data(_p(cd), _p(pos), _p(q), fovy, znear, draw_distance, viewport[0], viewport[1], pyramid[0], pyramid[1],
                                 draw_count, lod_step), "nv_build_cull_data")
    for k, v in flags.items():
        cd[k] = v
    return cd


def build_shade_data(globals_, camera_position=(0, 0, 0), sun_direction=(0, 1, 0), shadows_enabled=0, width=None, height=None):
    """NvShadeData of nv_shade_final (src/niagara.cpp:1917-1922) from the frame's globals (synth.make_globals): inverseViewProjection =
    inverse(projection * view) in fp64, rounded once; width / height default to the globals' screen size"""
    sd = np.zeros(1, dtype=L.SHADEDATA)
    g = np.ascontiguousarray(globals_)
    w = int(g["screenWidth"][0]) if width is None else int(width)
    h = int(g["screenHeight"][0]) if height is None else int(height)
    pos = np.ascontiguousarray(camera_position, dtype=np.float32)
    sun = np.ascontiguousarray(sun_direction, dtype=np.float32)
    check(lib.nv_build_shade_data(_p(sd), _p(g), _p(pos), _p(sun), int(shadows_enabled), w, h), "nv_build_shade_data")
    return sd


def build_shadow_data(globals_, sun_direction=(0, 1, 0), sun_jitter=0.0, checkerboard=0, width=None, height=None):
    """NvShadowData of nv_shadow_trace (src/niagara.cpp:1810-1815) from the frame's globals: inverseViewProjection as build_shade_data
    computes it; niagara's sun_jitter is 1e-2 when the shadow blur is on, else 0; width / height default to the globals' screen size"""
    sd = np.zeros(1, dtype=L.SHADOWDATA)
    g = np.ascontiguousarray(globals_)
    w = int(g["screenWidth"][0]) if width is None else int(width)
    h = int(g["screenHeight"][0]) if height is None else int(height)
    sun = np.ascontiguousarray(sun_direction, dtype=np.float32)
    check(lib.nv_build_shadow_data(_p(sd), _p(g), _p(sun), float(sun_jitter), int(checkerboard), w, h), "nv_build_shadow_data")
    return sd


RT_TMIN, RT_TMAX = 1e-2, 1e3  # shadow.comp.glsl:81


def rt_scene_build(meshes, indices, vertices, draws, texcoords=False):
    """The scene blob of the ray-traced shadow pass (nv_rt_scene_build; host only): one BLAS per mesh with triangles (lods[lodRT], through the
    index buffer of the classic path) and one TLAS over the casting draws.  texcoords: nv_rt_scene_build_textured, the blob the alpha-tested
    trace walks (the corners' fp16 texcoords in the triangles' w words, header flag bit 0).  Returns a 16-byte aligned uint8 array"""
    build = lib.nv_rt_scene_build_textured if texcoords else lib.nv_rt_scene_build
    name = "nv_rt_scene_build_textured" if texcoords else "nv_rt_scene_build"
    m = np.ascontiguousarray(meshes, L.MESH)
    i = np.ascontiguousarray(indices, np.uint32)
    v = np.ascontiguousarray(vertices, L.VERTEX)
    d = np.ascontiguousarray(draws, L.MESHDRAW)
    args = (_p(m) if len(m) else None, len(m), _p(i) if len(i) else None, len(i), _p(v) if len(v) else None, len(v), _p(d) if len(d) else None, len(d))
    n = C.c_uint64(0)
    check(build(*args, None, C.byref(n)), name)
    raw = np.zeros(n.value + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    blob = raw[off:off + n.value]
    room = C.c_uint64(n.value)
    check(build(*args, _p(blob), C.byref(room)), name)
    assert room.value == n.value
    return blob


def _aligned_bytes(n):
    """a zeroed uint8 array of n bytes whose data is 16-byte aligned"""
    raw = np.zeros(n + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + n]


def rt_tlas_build_host(blob, draws):
    """The host twin of nv_rt_tlas_build (nv_rt_tlas_build_host; no device work): a canonical blob with `blob`'s BLAS side and the TLAS of
    DESIGN.md §4.17 over the casting draws of `draws`.  Returns a 16-byte aligned uint8 array"""
    d = np.ascontiguousarray(draws, L.MESHDRAW)
    args = (_p(blob), blob.nbytes, _p(d) if len(d) else None, len(d))
    n = C.c_uint64(0)
    check(lib.nv_rt_tlas_build_host(*args, None, C.byref(n)), "nv_rt_tlas_build_host")
    out = _aligned_bytes(n.value)
    room = C.c_uint64(n.value)
    check(lib.nv_rt_tlas_build_host(*args, _p(out), C.byref(room)), "nv_rt_tlas_build_host")
    assert room.value == n.value
    return out


def rt_scene_validate(blob):
    """True when nv_rt_scene_validate accepts the blob (a uint8 array whose data is 16-byte aligned)"""
    return lib.nv_rt_scene_validate(_p(blob), blob.nbytes) == 0


def rt_scene_stats(blob):
    from ._lib import RtSceneStats
    st = RtSceneStats()
    check(lib.nv_rt_scene_stats(_p(blob), blob.nbytes, C.byref(st)), "nv_rt_scene_stats")
    return {n: int(getattr(st, n)) for n, _ in RtSceneStats._fields_}


def rt_scene_trace_host(blob, origins, dirs, quality=1, tmin=RT_TMIN, tmax=RT_TMAX):
    """nv_shadow_trace's traversal on the CPU for (n, 3) float32 rays: the mask's bytes, 0 = occluded, 255 = not"""
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    assert o.shape == d.shape
    out = np.zeros(len(o), np.uint8)
    check(lib.nv_rt_scene_trace_host_rays(_p(blob), _p(o), _p(d), len(o), float(tmin), float(tmax), int(quality), _p(out)), "nv_rt_scene_trace_host_rays")
    return out


def rt_scene_trace_host_textured(blob, origins, dirs, draws, materials, textures, texels, quality=1, tmin=RT_TMIN, tmax=RT_TMAX, texel_words=None):
    """nv_shadow_trace_textured's traversal on the CPU (nv_rt_scene_trace_host_textured_rays) for (n, 3) float32 rays over a blob built with
    texcoords=True: draws (layouts.MESHDRAW), materials (layouts.MATERIAL), textures (layouts.TEXTUREDESC, entry 0 reserved) and texels
    (uint32, the decoded RGBA8 set) are host arrays; texel_words defaults to len(texels).  The mask's bytes, 0 = occluded, 255 = not"""
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    assert o.shape == d.shape
    dr, m = np.ascontiguousarray(draws, L.MESHDRAW), np.ascontiguousarray(materials, L.MATERIAL)
    t, x = np.ascontiguousarray(textures, L.TEXTUREDESC), np.ascontiguousarray(texels, np.uint32)
    out = np.zeros(len(o), np.uint8)
    opt = lambda a: _p(a) if len(a) else None
    check(lib.nv_rt_scene_trace_host_textured_rays(_p(blob), _p(o), _p(d), len(o), float(tmin), float(tmax), int(quality), opt(dr), len(dr), opt(m), len(m),
                                                   opt(t), len(t), opt(x), len(x) if texel_words is None else int(texel_words), _p(out)),
          "nv_rt_scene_trace_host_textured_rays")
    return out


def rt_alpha_sample_host(desc, texels, uv):
    """(four_tap, sampler): the alpha-tested trace's four-tap alpha and textureLod(..., 0).w of the full sampler at (n, 2) float32 uv
    (nv_rt_alpha_sample_host; a test accessor: the two agree bit for bit)"""
    d, x = np.ascontiguousarray(desc, L.TEXTUREDESC).reshape(1), np.ascontiguousarray(texels, np.uint32)
    u = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
    a, b = np.zeros(len(u), np.float32), np.zeros(len(u), np.float32)
    check(lib.nv_rt_alpha_sample_host(_p(d), _p(x), len(x), _p(u), len(u), _p(a), _p(b)), "nv_rt_alpha_sample_host")
    return a, b


def synth_draws(n, mesh_count, scene_radius=300.0):
    d = np.zeros(n, dtype=L.MESHDRAW)
    check(lib.nv_synth_draws(_p(d), n, mesh_count, scene_radius), "nv_synth_draws")
    return d


def assign_visibility_offsets(draws, meshes):
    slots, mask = C.c_uint32(0), C.c_uint32(0)
    check(lib.nv_assign_visibility_offsets(_p(draws), len(draws), _p(meshes), len(meshes), C.byref(slots), C.byref(mask)),
          "nv_assign_visibility_offsets")
    return slots.value, mask.value


def assign_triangle_offsets(draws, meshes):
    """the names of the triangles of indexed draws (nv_assign_triangle_offsets): len(draws) + 1 u64, the prefix of the draws' widest LODs'
    triangle counts; NvError past 2^34 - 2 triangles"""
    offsets = np.zeros(len(draws) + 1, np.uint64)
    check(lib.nv_assign_triangle_offsets(_p(draws), len(draws), _p(meshes), len(meshes), _p(offsets)), "nv_assign_triangle_offsets")
    return offsets


def shard_range(total, rank, world):
    b, e = C.c_uint64(0), C.c_uint64(0)
    lib.nv_shard_range(total, rank, world, C.byref(b), C.byref(e))
    return b.value, e.value


def scenecache_info(path):
    """header of a niagara .cache file (src/scenecache.cpp:16-55) + where its Meshlet / Mesh / MeshDraw arrays sit"""
    from ._lib import SceneCacheInfo
    info = SceneCacheInfo()
    check(lib.nv_scenecache_info(os.fsencode(path), C.byref(info)), "nv_scenecache_info")
    return info


def scenecache_texture_paths(path):
    """the texture paths a niagara .cache file ends with (src/scenecache.cpp:192-197): textures[i + 1] is the DDS file paths[i] names"""
    info = scenecache_info(path)
    buf = (C.c_char * 256 * max(1, info.texturePathCount))()
    check(lib.nv_scenecache_texture_paths(os.fsencode(path), C.byref(info), C.cast(buf, C.c_void_p)), "nv_scenecache_texture_paths")
    return [os.fsdecode(bytes(buf[i]).split(b"\0", 1)[0]) for i in range(info.texturePathCount)]


def dds_parse(data):
    """nv_dds_parse of a DDS file image (bytes): a dict of format (layouts.FORMAT_*), width, height, levels, blockBytes, payloadOffset,
    payloadBytes and levelOffset (one byte offset per level, from payloadOffset).  Raises NvError(NV_EFORMAT) where niagara's loadImage refuses"""
    info = _dds_info(data)
    d = {n: int(getattr(info, n)) for n in ("format", "width", "height", "levels", "blockBytes", "payloadOffset", "payloadBytes")}
    d["levelOffset"] = [int(info.levelOffset[i]) for i in range(info.levels)]
    return d


def _dds_info(data):
    from ._lib import DdsInfo
    info = DdsInfo()
    data = bytes(data)
    check(lib.nv_dds_parse(data, len(data), C.byref(info)), "nv_dds_parse")
    return info


def texture_set_layout(files):
    """nv_texture_set_layout over DDS file images: (descs, texel_words, infos) — descs a layouts.TEXTUREDESC array of len(files) + 1 entries
    (entry 0 reserved), texel_words the size of the set's RGBA8 buffer in 32-bit words"""
    from ._lib import DdsInfo
    infos = (DdsInfo * max(1, len(files)))()
    for i, data in enumerate(files):
        infos[i] = _dds_info(data)
    descs = np.zeros(len(files) + 1, L.TEXTUREDESC)
    words = C.c_uint64(0)
    check(lib.nv_texture_set_layout(infos, len(files), _p(descs), C.byref(words)), "nv_texture_set_layout")
    return descs, int(words.value), infos


def texture_decode_host(files):
    """the whole set decoded on the CPU (nv_texture_decode_host, the text the kernel runs): (descs, texels uint32 array)"""
    descs, words, infos = texture_set_layout(files)
    texels = np.zeros(max(1, words), np.uint32)
    for i, data in enumerate(files):
        payload = np.frombuffer(bytes(data), np.uint8)[infos[i].payloadOffset:].copy()
        check(lib.nv_texture_decode_host(C.byref(infos[i]), _p(payload), _p(descs[i + 1:i + 2]), _p(texels), words), "nv_texture_decode_host")
    return descs, texels[:words]


def texture_sample_host(descs, texels, tex_id, uv, duvdx=(0.0, 0.0), duvdy=(0.0, 0.0)):
    """one sample of textures[tex_id] on the CPU (nv_texture_sample_host): four float32"""
    descs = np.ascontiguousarray(descs, L.TEXTUREDESC)
    texels = np.ascontiguousarray(texels, np.uint32)
    a, b, c = (np.asarray(v, np.float32).copy() for v in (uv, duvdx, duvdy))
    out = np.zeros(4, np.float32)
    check(lib.nv_texture_sample_host(_p(descs), len(descs), _p(texels), len(texels), int(tex_id), _p(a), _p(b), _p(c), _p(out)), "nv_texture_sample_host")
    return out


def texture_block_layout(files):
    """nv_texture_block_layout over DDS file images: (descs, units16, infos) — descs a layouts.TEXTUREBLOCKDESC array of len(files) + 1 entries
    (entry 0 reserved), units16 the size of the set's block buffer in 16-byte units"""
    from ._lib import DdsInfo
    infos = (DdsInfo * max(1, len(files)))()
    for i, data in enumerate(files):
        infos[i] = _dds_info(data)
    descs = np.zeros(len(files) + 1, L.TEXTUREBLOCKDESC)
    units = C.c_uint64(0)
    check(lib.nv_texture_block_layout(infos, len(files), _p(descs), C.byref(units)), "nv_texture_block_layout")
    return descs, int(units.value), infos


def texture_blocks_host(files):
    """the block-resident form of a set on the CPU: (descs, blocks uint8 array of 16 * units16 bytes) — each file's payload copied verbatim to
    byte 16 * offset"""
    descs, units, infos = texture_block_layout(files)
    blocks = np.zeros(max(1, units) * 16, np.uint8)
    for i, data in enumerate(files):
        at = int(descs[i + 1]["offset"]) * 16
        payload = np.frombuffer(bytes(data), np.uint8)[infos[i].payloadOffset:]
        blocks[at:at + len(payload)] = payload
    return descs, blocks[:units * 16] if units else blocks[:0]


def texture_block_fetch_host(desc, blocks, level, x, y, units16=None):
    """the RGBA8 code of one texel decoded from its block (nv_texture_block_fetch_host)"""
    d = np.ascontiguousarray(desc, L.TEXTUREBLOCKDESC).reshape(1)
    blocks = np.ascontiguousarray(blocks, np.uint8)
    out = np.zeros(1, np.uint32)
    check(lib.nv_texture_block_fetch_host(_p(d), _p(blocks), len(blocks) // 16 if units16 is None else int(units16), int(level), int(x), int(y), _p(out)),
          "nv_texture_block_fetch_host")
    return int(out[0])


def texture_block_sample_host(descs, blocks, tex_id, uv, duvdx=(0.0, 0.0), duvdy=(0.0, 0.0)):
    """texture_sample_host over a block-resident set (nv_texture_block_sample_host): the same four float32, bit for bit"""
    descs = np.ascontiguousarray(descs, L.TEXTUREBLOCKDESC)
    blocks = np.ascontiguousarray(blocks, np.uint8)
    a, b, c = (np.asarray(v, np.float32).copy() for v in (uv, duvdx, duvdy))
    out = np.zeros(4, np.float32)
    check(lib.nv_texture_block_sample_host(_p(descs), len(descs), _p(blocks), len(blocks) // 16, int(tex_id), _p(a), _p(b), _p(c), _p(out)),
          "nv_texture_block_sample_host")
    return out


def texture_block_decode_host(fmt, lo, hi):
    """(alpha, split): per texel of one block the alpha-only decode and the RGBA8 code through the BC7 header / per-texel split
    (nv_texture_block_decode_host); 16 uint32 each"""
    alpha, split = np.zeros(16, np.uint32), np.zeros(16, np.uint32)
    check(lib.nv_texture_block_decode_host(int(fmt), int(lo), int(hi), _p(alpha), _p(split)), "nv_texture_block_decode_host")
    return alpha, split


def scenecache_read(path):
    """(info, meshes, meshlets, draws) of a niagara .cache file; the arrays are the raw struct arrays of the file"""
    info = scenecache_info(path)
    meshes = np.zeros(info.meshCount, dtype=L.MESH)
    meshlets = np.zeros(info.meshletCount, dtype=L.MESHLET)
    draws = np.zeros(info.drawCount, dtype=L.MESHDRAW)
    check(lib.nv_scenecache_read(os.fsencode(path), C.byref(info), _p(meshes), _p(meshlets), _p(draws)), "nv_scenecache_read")
    return info, meshes, meshlets, draws


def scenecache_animations(path):
    """(lights, animations, keyframes) of a niagara .cache file (layouts.LIGHT / ANIMATION / KEYFRAME): the three raw arrays behind its
    draws (nv_scenecache_animations)"""
    info = scenecache_info(path)
    lights = np.zeros(info.lightCount, dtype=L.LIGHT)
    animations = np.zeros(info.animationCount, dtype=L.ANIMATION)
    keyframes = np.zeros(info.keyframeCount, dtype=L.KEYFRAME)
    check(lib.nv_scenecache_animations(os.fsencode(path), C.byref(info), _p(lights), _p(animations), _p(keyframes)), "nv_scenecache_animations")
    return lights, animations, keyframes


ANIM_REASONS = ("ok", "no_keyframes", "keyframe_range", "period", "draw_index", "light_index", "duplicate_draw", "duplicate_light")  # NV_ANIM_*


def animation_validate(animations, keyframe_count, draw_count, light_count=0):
    """(reason, index) of nv_animation_validate_host: reason is one of ANIM_REASONS ("ok" for a table nv_upload_animations accepts), index the
    first animation it holds for"""
    a = np.ascontiguousarray(animations, L.ANIMATION)
    reason, index = C.c_uint32(0), C.c_uint32(0)
    rc = lib.nv_animation_validate_host(_p(a), len(a), int(keyframe_count), int(draw_count), int(light_count), C.byref(reason), C.byref(index))
    if rc != 0 and reason.value == 0:
        check(rc, "nv_animation_validate_host")
    return ANIM_REASONS[reason.value], index.value


def animation_phase(animations, which, times):
    """the time statements of nv_animate_draws alone (nv_animation_phase_host), one sample per (animations[which[i]], times[i]): (skipped bool,
    index0, index1, t float32); the entries of a skipped sample are zero"""
    a = np.ascontiguousarray(animations, L.ANIMATION)
    which, times = np.ascontiguousarray(which, np.uint32), np.ascontiguousarray(times, np.float64)
    if len(which) != len(times) or (len(which) and int(which.max()) >= len(a)):
        raise ValueError("animation_phase: one time per sampled animation, every index inside the table")
    n = len(which)
    skipped, i0, i1, t = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.float32)
    check(lib.nv_animation_phase_host(_p(a), _p(which), _p(times), n, _p(skipped), _p(i0), _p(i1), _p(t)), "nv_animation_phase_host")
    return skipped.astype(bool), i0, i1, t


def animate_draws_host(time, animations, keyframes, draws, lights=None, draw_count=None, light_count=None):
    """the host twin of Context.animate_draws (nv_animate_draws_host, the kernel's text): rewrites `draws` (layouts.MESHDRAW, or None) and
    `lights` (layouts.LIGHT, or None) IN PLACE.  draw_count / light_count: the bounds the indices are validated against where the array is
    None (its targets are then skipped)"""
    a = np.ascontiguousarray(animations, L.ANIMATION)
    k = np.ascontiguousarray(keyframes, L.KEYFRAME)
    for arr, dt in ((draws, L.MESHDRAW), (lights, L.LIGHT)):
        if arr is not None and not (arr.dtype == dt and arr.flags.c_contiguous and arr.flags.writeable):
            raise ValueError("animate_draws_host rewrites its arrays in place: contiguous, writeable arrays of the layout's dtype")
    check(lib.nv_animate_draws_host(float(time), _p(a), len(a), _p(k), len(k), None if draws is None else _p(draws), int(draw_count or 0) if draws is None else len(draws),
                                    None if lights is None else _p(lights), int(light_count or 0) if lights is None else len(lights)),
          "nv_animate_draws_host")


def mesh_bounds(positions):
    """Mesh.center / Mesh.radius of src/scene.cpp:207-220 over an (n, 3) float32 array"""
    pos = np.ascontiguousarray(positions, np.float32)
    center, radius = np.zeros(3, np.float32), np.zeros(1, np.float32)
    check(lib.nv_mesh_bounds(_p(pos), len(pos), _p(center), _p(radius)), "nv_mesh_bounds")
    return center, radius[0]
