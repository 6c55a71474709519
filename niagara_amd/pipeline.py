"""Host-side mirror of niagara's cull/render/pyramid lambdas (src/niagara.cpp:1530-1611,1703-1733,1765-1788)
driving the HIP passes through the C ABI.  torch is plumbing only: device memory, streams, torch.distributed.

Buffer names follow the reference (src/niagara.cpp:1027-1093):
    mb meshes · mlb meshlets · db draws · dvb drawVisibility · dcb draw/task commands · dccb command count + indirect
    args · mvb meshletVisibility · cib clusterIndices · ccb cluster count + indirect args
"""
import ctypes as C

import numpy as np
import torch

from . import host
from . import synth
from . import layouts as L
from ._lib import PROF_NAMES, VARIANT_NAMES, NvError, PyramidDesc, check, lib


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def to_device(arr, device):
    """numpy (structured) array -> flat uint8 device tensor with the same bytes"""
    a = np.ascontiguousarray(arr)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(device)


def from_device(t, dtype, count=None):
    a = t.detach().cpu().numpy().view(np.uint8).reshape(-1)
    out = a.view(dtype)
    return out[:count] if count is not None else out


NV_OPT_FUSED_COUNT_RESET = 1
NV_OPT_FUSED_SUBMIT = 2
NV_OPT_CULL_WORKGROUPS_PER_CU = 3
NV_OPT_SCATTER_WAVES = 4
NV_OPT_CULL_FORM = 5
NV_OPT_CULL_RING = 6
NV_OPT_TASK_EMIT = 7
NV_OPT_DRAW_RECORDS = 8
NV_OPT_RASTER_SMALL_LIMIT = 9
NV_OPT_RASTER_NEAR_CLIP = 10
NV_OPT_RASTER_VISIBILITY_ID = 11
NV_OPT_BLOOM_FUSED_TAIL = 12


class Context:
    """one nv_context per device; not re-entrant (one stream at a time)"""

    def __init__(self, device=None):
        if not torch.cuda.is_available():
            raise NvError("niagara_amd needs a HIP device: torch.cuda.is_available() is False and there is no CPU path")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        h = C.c_void_p()
        check(lib.nv_create(C.byref(h), self.device.index), "nv_create")
        self.h = h

    def close(self):
        if self.h:
            lib.nv_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def status(self):
        check(lib.nv_status(self.h, _stream()), "nv_status")

    def set_option(self, option, value):
        check(lib.nv_set_option(self.h, int(option), int(value)), "nv_set_option")

    def reserve(self, max_draws, max_commands=0):
        """scratch for passes over up to max_draws draws (nv_create reserves 1 M): pass entry points never allocate"""
        check(lib.nv_reserve(self.h, int(max_draws), int(max_commands)), "nv_reserve")

    def share_scene(self, other):
        """use `other`'s scene mirrors (meshlet SoA, draw mirror, mesh table) instead of building this context's own"""
        check(lib.nv_share_scene(self.h, other.h), "nv_share_scene")

    def profile(self, enabled):
        check(lib.nv_profile_enable(self.h, int(enabled)), "nv_profile_enable")

    def profile_read(self):
        """{slot: (total_ms, launches)} for every slot of _lib.PROF_NAMES"""
        ms, cnt = (C.c_float * len(PROF_NAMES))(), (C.c_uint32 * len(PROF_NAMES))()
        check(lib.nv_profile_read(self.h, C.byref(ms), C.byref(cnt)), "nv_profile_read")
        return {n: (float(ms[i]), int(cnt[i])) for i, n in enumerate(PROF_NAMES)}

    VARIANTS = VARIANT_NAMES

    def profile_variants(self):
        """{variant: launches since the last call}: which kernel form the host's per-launch choices resolved to (non-zero entries only)"""
        cnt = (C.c_uint32 * len(self.VARIANTS))()
        check(lib.nv_profile_variants(self.h, C.byref(cnt)), "nv_profile_variants")
        return {n: int(cnt[i]) for i, n in enumerate(self.VARIANTS) if cnt[i]}

    # ---- passes (argument order = descriptor order of the reference dispatches)
    def upload_meshlets(self, mlb, count):
        check(lib.nv_upload_meshlets(self.h, _stream(), _ptr(mlb), count), "nv_upload_meshlets")

    def upload_meshes(self, mb, count):
        check(lib.nv_upload_meshes(self.h, _stream(), _ptr(mb), count), "nv_upload_meshes")

    def meshlet_bounds(self, vertices, meshlet_data, mlb, count, bounds8=None):
        """src/scene.cpp:69-85 on the GPU: fills center / radius / cone of the Meshlet records in `mlb` (parity unpinned: header)"""
        check(lib.nv_meshlet_bounds(self.h, _stream(), _ptr(vertices), _ptr(meshlet_data), _ptr(mlb), count, _ptr(bounds8)), "nv_meshlet_bounds")

    def upload_draws(self, db, count, mb=None):
        """mirror of what a draw decision reads: world-space spheres (mesh bounds of table `mb` folded in), scale, meshIndex,
        postPass (None, 0 drops the registration)"""
        check(lib.nv_upload_draws(self.h, _stream(), _ptr(db), count, _ptr(mb)), "nv_upload_draws")

    def update_draws(self, db, first, count):
        """re-transposes draws [first, first + count) after the caller rewrote them (animation, src/niagara.cpp:1385-1391)"""
        check(lib.nv_update_draws(self.h, _stream(), _ptr(db), first, count), "nv_update_draws")

    def upload_animations(self, animations, keyframes, draw_count, light_count=0):
        """validate the host tables (layouts.ANIMATION / KEYFRAME; host.animation_validate names a refusal's reason) and keep context-owned
        device copies for animate_draws (nv_upload_animations: load time, synchronises).  draw_count / light_count: the bounds the target
        indices are checked against.  animations=None drops the copies"""
        if animations is None:
            check(lib.nv_upload_animations(self.h, _stream(), None, 0, None, 0, 0, 0), "nv_upload_animations")
            return
        a = np.ascontiguousarray(animations, L.ANIMATION)
        k = np.ascontiguousarray(keyframes, L.KEYFRAME)
        keep = np.zeros(1, L.KEYFRAME)  # an empty table is still a table: a non-NULL pointer with count 0
        check(lib.nv_upload_animations(self.h, _stream(), C.c_void_p(a.ctypes.data if len(a) else keep.ctypes.data), len(a),
                                       C.c_void_p(k.ctypes.data if len(k) else keep.ctypes.data), len(k), int(draw_count), int(light_count)),
              "nv_upload_animations")

    def animate_draws(self, time, db, draw_count, lights=None, light_count=0):
        """src/niagara.cpp:1368-1409 on the device (nv_animate_draws): evaluates the uploaded animations at `time` and rewrites position, scale
        and orientation of their target draws in the device buffer `db` (and the position of their target lights in `lights`, a device buffer
        of layouts.LIGHT, when given); when `db` is the buffer registered by upload_draws the cull mirror is rewritten in the same launch.  One
        launch, can be captured; `time` travels by value"""
        check(lib.nv_animate_draws(self.h, _stream(), float(time), _ptr(db), int(draw_count), _ptr(lights), int(light_count)), "nv_animate_draws")

    def drawcull(self, cull, late, task, db, mb, dcb, dccb, dvb, pyramid=None):
        check(lib.nv_drawcull(self.h, _stream(), C.c_void_p(cull.ctypes.data), int(late), int(task), _ptr(db), _ptr(mb), _ptr(dcb),
                              _ptr(dccb), _ptr(dvb), None if pyramid is None else C.byref(pyramid)), "nv_drawcull")

    def reset_count(self, a, b=None):
        check(lib.nv_reset_count(self.h, _stream(), _ptr(a), _ptr(b)), "nv_reset_count")

    def tasksubmit(self, dccb, dcb):
        check(lib.nv_tasksubmit(self.h, _stream(), _ptr(dccb), _ptr(dcb)), "nv_tasksubmit")

    def clustercull(self, cull, late, dcb, dccb, db, mlb, mvb, pyramid, cib, ccb):
        check(lib.nv_clustercull(self.h, _stream(), C.c_void_p(cull.ctypes.data), int(late), _ptr(dcb), _ptr(dccb), _ptr(db), _ptr(mlb),
                                 _ptr(mvb), None if pyramid is None else C.byref(pyramid), _ptr(cib), _ptr(ccb)), "nv_clustercull")

    def bind_clustercull(self, stream, cull, late, dcb, dccb, db, mlb, mvb, pyramid, cib, ccb):
        """nv_clustercull with every argument marshalled once: returns a zero-argument callable that launches the pass on
        `stream` (a torch.cuda.Stream, or None for the current one).  For callers that issue many passes back to back: the
        per-call marshalling (stream lookup, data_ptr() of eight tensors) costs more host time than a 25 us pass leaves."""
        st = C.c_void_p((torch.cuda.current_stream() if stream is None else stream).cuda_stream)
        keep = (stream, cull, dcb, dccb, db, mlb, mvb, pyramid, cib, ccb)  # the closure keeps the buffers alive
        args = (self.h, st, C.c_void_p(cull.ctypes.data), int(late), _ptr(dcb), _ptr(dccb), _ptr(db), _ptr(mlb), _ptr(mvb),
                None if pyramid is None else C.byref(pyramid), _ptr(cib), _ptr(ccb))
        fn = lib.nv_clustercull

        def launch(_keep=keep):
            rc = fn(*args)
            if rc:
                check(rc, "nv_clustercull")
        return launch

    def clustersubmit(self, ccb, cib):
        check(lib.nv_clustersubmit(self.h, _stream(), _ptr(ccb), _ptr(cib)), "nv_clustersubmit")

    def taskcull(self, cull, late, dcb, dccb, db, mlb, mvb, pyramid, payloads, payload_counts):
        check(lib.nv_taskcull(self.h, _stream(), C.c_void_p(cull.ctypes.data), int(late), _ptr(dcb), _ptr(dccb), _ptr(db), _ptr(mlb),
                              _ptr(mvb), None if pyramid is None else C.byref(pyramid), _ptr(payloads), _ptr(payload_counts)), "nv_taskcull")

    def cluster_expand(self, dcb, mlb, cib, ccb, records, capacity, totals3):
        check(lib.nv_cluster_expand(self.h, _stream(), _ptr(dcb), _ptr(mlb), _ptr(cib), _ptr(ccb), _ptr(records), capacity, _ptr(totals3)),
              "nv_cluster_expand")

    def trianglecull(self, globals_, dcb, db, mlb, meshlet_data, vertices, cib, ccb, masks, capacity, totals3):
        """meshlet.mesh.glsl:91-198 with MESH_CULL = 1: one NvTriangleMask per slot of the consumer's grid"""
        check(lib.nv_trianglecull(self.h, _stream(), C.c_void_p(globals_.ctypes.data), _ptr(dcb), _ptr(db), _ptr(mlb), _ptr(meshlet_data), _ptr(vertices),
                                  _ptr(cib), _ptr(ccb), _ptr(masks), capacity, _ptr(totals3)), "nv_trianglecull")

    def rasterdepth(self, globals_, dcb, db, mlb, meshlet_data, vertices, cib, ccb, depth, width, height, visibility=None, totals4=None):
        """depth-only raster of the clusters in cib / ccb into `depth` (fp32 width x height, reverse-Z, atomic max: the caller clears it);
        visibility (optional, width x height u64): max of bits(z) << 32 | slot << 7 | triangle, or with NV_OPT_RASTER_VISIBILITY_ID 1 of the
        stable form bits(z) << 34 | ((mvi << 7 | triangle) + 1); totals4 (optional, accumulated):
        clusters, triangles, triangles rasterised, samples covered"""
        check(lib.nv_rasterdepth(self.h, _stream(), C.c_void_p(globals_.ctypes.data), _ptr(dcb), _ptr(db), _ptr(mlb), _ptr(meshlet_data), _ptr(vertices),
                                 _ptr(cib), _ptr(ccb), _ptr(depth), int(width), int(height), _ptr(visibility), _ptr(totals4)), "nv_rasterdepth")

    def rasterdepth_textured(self, globals_, dcb, db, mlb, meshlet_data, vertices, cib, ccb, depth, width, height, visibility=None, totals4=None,
                             materials=None, material_count=0, textures=None, texture_count=0, texels=None, texel_words=0, alpha_totals2=None):
        """rasterdepth whose covered samples of a post-pass launch (globals' postPass != 0, with `materials`) also pass the fragment's alpha
        test against the albedo texture (nv_rasterdepth_textured, mesh.frag.glsl:88): a sample with albedo.a < 0.5 touches neither target.
        materials = a device table of layouts.MATERIAL, textures / texels = texture_decode's set; totals4[3] counts the samples kept,
        alpha_totals2 (optional, accumulated): samples dropped, samples unevaluated"""
        self._rasterdepth_set("nv_rasterdepth_textured", globals_, dcb, db, mlb, meshlet_data, vertices, cib, ccb, depth, width, height, visibility, totals4,
                              materials, material_count, textures, texture_count, alpha_totals2, texels, texel_words)

    # The three passes that read a texture set exist once per residency of the set (decoded RGBA8 words: *_textured; BC blocks: *_blocks) with
    # one signature that differs in the set's last two values, its buffer and the buffer's size: each pair marshals through one helper
    def _rasterdepth_set(self, entry, globals_, dcb, db, mlb, meshlet_data, vertices, cib, ccb, depth, width, height, visibility, totals4, materials,
                         material_count, textures, texture_count, alpha_totals2, buffer, size):
        check(getattr(lib, entry)(self.h, _stream(), C.c_void_p(globals_.ctypes.data), _ptr(dcb), _ptr(db), _ptr(mlb), _ptr(meshlet_data), _ptr(vertices),
                                  _ptr(cib), _ptr(ccb), _ptr(depth), int(width), int(height), _ptr(visibility), _ptr(totals4), _ptr(materials),
                                  int(material_count), _ptr(textures), int(texture_count), _ptr(buffer), int(size), _ptr(alpha_totals2)), entry)

    def _visibility_attributes_set(self, entry, globals_, records, width, height, db, draw_count, mlb, meshlet_count, meshlet_data, data_words, vertices,
                                   vertex_count, materials, material_count, attributes, gbuffer0, gbuffer1, totals4, textures, texture_count, buffer, size):
        check(getattr(lib, entry)(self.h, _stream(), C.c_void_p(globals_.ctypes.data), _ptr(records), int(width), int(height), _ptr(db), int(draw_count),
                                  _ptr(mlb), int(meshlet_count), _ptr(meshlet_data), int(data_words), _ptr(vertices), int(vertex_count), _ptr(materials),
                                  int(material_count), _ptr(attributes), _ptr(gbuffer0), _ptr(gbuffer1), _ptr(totals4), _ptr(textures),
                                  int(texture_count), _ptr(buffer), int(size)), entry)

    def _shadow_trace_set(self, entry, shadow_data, depth, shadow, width, height, quality, draws, draw_count, materials, material_count, textures,
                          texture_count, buffer, size):
        check(getattr(lib, entry)(self.h, _stream(), C.c_void_p(shadow_data.ctypes.data) if shadow_data is not None else None, _ptr(depth), _ptr(shadow),
                                  int(width), int(height), int(quality), _ptr(draws), int(draw_count), _ptr(materials), int(material_count),
                                  _ptr(textures), int(texture_count), _ptr(buffer), int(size)), entry)

    def rasterdepth_indexed(self, globals_, dcb, dccb, db, draw_count, ib, index_capacity, vertices, vertex_capacity, depth, width, height,
                            totals4=None):
        """depth-only raster of the indexed draws dcb[0, min(dccb[0], draw_count)) (vkCmdDrawIndexedIndirectCount with maxDrawCount = draw_count)
        into `depth` (fp32 width x height, reverse-Z, atomic max: the caller clears it); ib holds index_capacity u32 indices, vertices
        vertex_capacity records; totals4 (optional, accumulated): commands drawn, triangles, triangles rasterised, samples covered"""
        check(lib.nv_rasterdepth_indexed(self.h, _stream(), C.c_void_p(globals_.ctypes.data), _ptr(dcb), _ptr(dccb), _ptr(db), int(draw_count), _ptr(ib),
                                         int(index_capacity), _ptr(vertices), int(vertex_capacity), _ptr(depth), int(width), int(height), _ptr(totals4)),
              "nv_rasterdepth_indexed")

    def rasterdepth_indexed_visibility(self, globals_, dcb, dccb, db, draw_count, ib, index_capacity, vertices, vertex_capacity, depth, width, height,
                                       triangle_offsets, visibility, totals4=None):
        """rasterdepth_indexed, and per covered sample the atomic maximum of bits(z) << 34 | (triangle_offsets[drawId] + t + 1) into `visibility`
        (u64 width x height: the caller clears it) — nv_rasterdepth_indexed_visibility.  triangle_offsets: draw_count + 1 u64 on the device
        (host.assign_triangle_offsets); on a shard, the full array sliced at the rank's first draw"""
        check(lib.nv_rasterdepth_indexed_visibility(self.h, _stream(), C.c_void_p(globals_.ctypes.data), _ptr(dcb), _ptr(dccb), _ptr(db), int(draw_count),
                                                    _ptr(ib), int(index_capacity), _ptr(vertices), int(vertex_capacity), _ptr(depth), int(width),
                                                    int(height), _ptr(totals4), _ptr(triangle_offsets), _ptr(visibility)),
              "nv_rasterdepth_indexed_visibility")

    def visibility_resolve_indexed(self, cull, visibility, width, height, db, draw_count, mb, mesh_count, triangle_offsets, records=None,
                                   draw_pixels=None, totals4=None):
        """rasterdepth_indexed_visibility's target back to {draw, index position, vertex offset, depth bits} per pixel
        (nv_visibility_resolve_indexed).  db / mb / triangle_offsets: the FULL arrays; cull: the CullData of the frame that was rasterised.
        records (width * height layouts.VISINDEXEDRECORD), draw_pixels (draw_count u32, accumulated) and totals4 (u64: covered, unresolved, 0,
        0, accumulated) are each optional"""
        check(lib.nv_visibility_resolve_indexed(self.h, _stream(), C.c_void_p(cull.ctypes.data), _ptr(visibility), int(width), int(height), _ptr(db),
                                                int(draw_count), _ptr(mb), int(mesh_count), _ptr(triangle_offsets), _ptr(records), _ptr(draw_pixels),
                                                _ptr(totals4)), "nv_visibility_resolve_indexed")

    def visibility_attributes_indexed(self, globals_, records, width, height, db, draw_count, ib, index_capacity, vertices, vertex_capacity,
                                      materials=None, material_count=0, attributes=None, gbuffer0=None, gbuffer1=None, totals4=None):
        """visibility_attributes over visibility_resolve_indexed's records (nv_visibility_attributes_indexed): the corners are
        vertices[ib[indexPosition + k] + vertexOffset]; outputs, totals and the material rule as visibility_attributes"""
        check(lib.nv_visibility_attributes_indexed(self.h, _stream(), C.c_void_p(globals_.ctypes.data), _ptr(records), int(width), int(height), _ptr(db),
                                                   int(draw_count), _ptr(ib), int(index_capacity), _ptr(vertices), int(vertex_capacity),
                                                   _ptr(materials), int(material_count), _ptr(attributes), _ptr(gbuffer0), _ptr(gbuffer1),
                                                   _ptr(totals4)), "nv_visibility_attributes_indexed")

    # ---- the classic path over a texture set: one pair per pass, marshalled like the cluster path's pairs above
    def _rasterdepth_indexed_set(self, entry, globals_, dcb, dccb, db, draw_count, ib, index_capacity, vertices, vertex_capacity, depth, width, height,
                                 totals4, triangle_offsets, visibility, materials, material_count, textures, texture_count, alpha_totals2, buffer, size):
        check(getattr(lib, entry)(self.h, _stream(), C.c_void_p(globals_.ctypes.data), _ptr(dcb), _ptr(dccb), _ptr(db), int(draw_count), _ptr(ib),
                                  int(index_capacity), _ptr(vertices), int(vertex_capacity), _ptr(depth), int(width), int(height), _ptr(totals4),
                                  _ptr(triangle_offsets), _ptr(visibility), _ptr(materials), int(material_count), _ptr(textures), int(texture_count),
                                  _ptr(buffer), int(size), _ptr(alpha_totals2)), entry)

    def rasterdepth_indexed_textured(self, globals_, dcb, dccb, db, draw_count, ib, index_capacity, vertices, vertex_capacity, depth, width, height,
                                     triangle_offsets=None, visibility=None, totals4=None, materials=None, material_count=0, textures=None,
                                     texture_count=0, texels=None, texel_words=0, alpha_totals2=None):
        """rasterdepth_indexed_visibility (triangle_offsets / visibility optional as a pair: without them rasterdepth_indexed) whose covered
        samples of a post-pass launch (globals' postPass != 0, with `materials`) also pass the fragment's alpha test against the albedo
        texture (nv_rasterdepth_indexed_textured): a sample with albedo.a < 0.5 touches neither target.  totals4[3] counts the samples kept,
        alpha_totals2 (optional, accumulated): samples dropped, samples unevaluated"""
        self._rasterdepth_indexed_set("nv_rasterdepth_indexed_textured", globals_, dcb, dccb, db, draw_count, ib, index_capacity, vertices,
                                      vertex_capacity, depth, width, height, totals4, triangle_offsets, visibility, materials, material_count, textures,
                                      texture_count, alpha_totals2, texels, texel_words)

    def rasterdepth_indexed_blocks(self, globals_, dcb, dccb, db, draw_count, ib, index_capacity, vertices, vertex_capacity, depth, width, height,
                                   triangle_offsets=None, visibility=None, totals4=None, materials=None, material_count=0, textures=None,
                                   texture_count=0, blocks=None, units16=0, alpha_totals2=None):
        """rasterdepth_indexed_textured over a block-resident set (nv_rasterdepth_indexed_blocks): the same targets and counters bit for bit"""
        self._rasterdepth_indexed_set("nv_rasterdepth_indexed_blocks", globals_, dcb, dccb, db, draw_count, ib, index_capacity, vertices,
                                      vertex_capacity, depth, width, height, totals4, triangle_offsets, visibility, materials, material_count, textures,
                                      texture_count, alpha_totals2, blocks, units16)

    def _visibility_attributes_indexed_set(self, entry, globals_, records, width, height, db, draw_count, ib, index_capacity, vertices, vertex_capacity,
                                           materials, material_count, attributes, gbuffer0, gbuffer1, totals4, textures, texture_count, buffer, size):
        check(getattr(lib, entry)(self.h, _stream(), C.c_void_p(globals_.ctypes.data), _ptr(records), int(width), int(height), _ptr(db), int(draw_count),
                                  _ptr(ib), int(index_capacity), _ptr(vertices), int(vertex_capacity), _ptr(materials), int(material_count),
                                  _ptr(attributes), _ptr(gbuffer0), _ptr(gbuffer1), _ptr(totals4), _ptr(textures), int(texture_count), _ptr(buffer),
                                  int(size)), entry)

    def visibility_attributes_indexed_textured(self, globals_, records, width, height, db, draw_count, ib, index_capacity, vertices, vertex_capacity,
                                               materials, material_count, attributes=None, gbuffer0=None, gbuffer1=None, totals4=None, textures=None,
                                               texture_count=0, texels=None, texel_words=0):
        """visibility_attributes_indexed with the complete fragment stage (nv_visibility_attributes_indexed_textured): the set as
        visibility_attributes_textured takes it; totals4[3] counts the pixels whose material names a texture the pass could not sample"""
        self._visibility_attributes_indexed_set("nv_visibility_attributes_indexed_textured", globals_, records, width, height, db, draw_count, ib,
                                                index_capacity, vertices, vertex_capacity, materials, material_count, attributes, gbuffer0, gbuffer1,
                                                totals4, textures, texture_count, texels, texel_words)

    def visibility_attributes_indexed_blocks(self, globals_, records, width, height, db, draw_count, ib, index_capacity, vertices, vertex_capacity,
                                             materials, material_count, attributes=None, gbuffer0=None, gbuffer1=None, totals4=None, textures=None,
                                             texture_count=0, blocks=None, units16=0):
        """visibility_attributes_indexed_textured over a block-resident set (nv_visibility_attributes_indexed_blocks): the same outputs bit for bit"""
        self._visibility_attributes_indexed_set("nv_visibility_attributes_indexed_blocks", globals_, records, width, height, db, draw_count, ib,
                                                index_capacity, vertices, vertex_capacity, materials, material_count, attributes, gbuffer0, gbuffer1,
                                                totals4, textures, texture_count, blocks, units16)

    def depth_merge(self, dst, srcs, width, height):
        """dst = element-wise maximum of dst and every target of `srcs` on the bit patterns (nv_depth_merge): the depth composite of shards
        that live on one device, and the fold of a received target into the local one"""
        ptrs = (C.c_void_p * len(srcs))(*[None if t is None else t.data_ptr() for t in srcs])
        check(lib.nv_depth_merge(self.h, _stream(), _ptr(dst), ptrs if len(srcs) else None, len(srcs), int(width), int(height)), "nv_depth_merge")

    def visibility_merge(self, dst, srcs, width, height):
        """dst = element-wise unsigned 64-bit maximum of dst and every visibility target of `srcs` (nv_visibility_merge): the composite of
        stable-form visibility buffers of shards that live on one device"""
        ptrs = (C.c_void_p * len(srcs))(*[None if t is None else t.data_ptr() for t in srcs])
        check(lib.nv_visibility_merge(self.h, _stream(), _ptr(dst), ptrs if len(srcs) else None, len(srcs), int(width), int(height)), "nv_visibility_merge")

    def visibility_resolve(self, cull, visibility, width, height, db, draw_count, mb, mesh_count, records=None, meshlet_seen=None, draw_pixels=None,
                           totals4=None):
        """the stable-form visibility buffer back to {draw, meshlet, triangle, depth bits} per pixel (nv_visibility_resolve).  db / mb: the FULL
        draw array and the Mesh table; cull: the CullData of the frame that was rasterised (the LOD is selected again from it).  records
        (width * height NvVisRecord), meshlet_seen (mvb layout, OR-ed), draw_pixels (draw_count u32, accumulated) and totals4 (u64:
        covered, unresolved, 0, 0, accumulated) are each optional"""
        check(lib.nv_visibility_resolve(self.h, _stream(), C.c_void_p(cull.ctypes.data), _ptr(visibility), int(width), int(height), _ptr(db),
                                        int(draw_count), _ptr(mb), int(mesh_count), _ptr(records), _ptr(meshlet_seen), _ptr(draw_pixels),
                                        _ptr(totals4)), "nv_visibility_resolve")

    def visibility_attributes(self, globals_, records, width, height, db, draw_count, mlb, meshlet_count, meshlet_data, data_words, vertices,
                              vertex_count, materials=None, material_count=0, attributes=None, gbuffer0=None, gbuffer1=None, totals4=None):
        """the attribute pass over nv_visibility_resolve's records (nv_visibility_attributes): per pixel the varyings of the triangle it names
        (attributes: width * height NvPixelAttributes) and, with a material table, the two G-buffer words (gbuffer0 R8G8B8A8_UNORM, gbuffer1
        A2B10G10R10_UNORM_PACK32; width * height u32 each).  db: the FULL draw array; globals_: the frame's projection and view.  totals4 (u64,
        accumulated): shaded, invalid, degenerate, pixels whose material names a texture.  Every output is optional"""
        check(lib.nv_visibility_attributes(self.h, _stream(), C.c_void_p(globals_.ctypes.data), _ptr(records), int(width), int(height), _ptr(db),
                                           int(draw_count), _ptr(mlb), int(meshlet_count), _ptr(meshlet_data), int(data_words), _ptr(vertices),
                                           int(vertex_count), _ptr(materials), int(material_count), _ptr(attributes), _ptr(gbuffer0), _ptr(gbuffer1),
                                           _ptr(totals4)), "nv_visibility_attributes")

    def visibility_attributes_textured(self, globals_, records, width, height, db, draw_count, mlb, meshlet_count, meshlet_data, data_words, vertices,
                                       vertex_count, materials, material_count, attributes=None, gbuffer0=None, gbuffer1=None, totals4=None,
                                       textures=None, texture_count=0, texels=None, texel_words=0):
        """visibility_attributes with the complete fragment stage (nv_visibility_attributes_textured): textures = a device table of
        layouts.TEXTUREDESC (entry 0 reserved), texels = the decoded set (texture_decode).  totals4[3] counts the pixels whose material names a
        texture the pass could not sample: 0 on a complete set"""
        self._visibility_attributes_set("nv_visibility_attributes_textured", globals_, records, width, height, db, draw_count, mlb, meshlet_count,
                                        meshlet_data, data_words, vertices, vertex_count, materials, material_count, attributes, gbuffer0, gbuffer1,
                                        totals4, textures, texture_count, texels, texel_words)

    def rasterdepth_blocks(self, globals_, dcb, db, mlb, meshlet_data, vertices, cib, ccb, depth, width, height, visibility=None, totals4=None,
                           materials=None, material_count=0, textures=None, texture_count=0, blocks=None, units16=0, alpha_totals2=None):
        """rasterdepth_textured over a block-resident set (nv_rasterdepth_blocks): textures = a device table of
        layouts.TEXTUREBLOCKDESC, blocks = texture_blocks' buffer of units16 16-byte units.  The same targets and counters bit for bit"""
        self._rasterdepth_set("nv_rasterdepth_blocks", globals_, dcb, db, mlb, meshlet_data, vertices, cib, ccb, depth, width, height, visibility, totals4,
                              materials, material_count, textures, texture_count, alpha_totals2, blocks, units16)

    def shadow_trace_blocks(self, shadow_data, depth, shadow, width, height, quality, draws, draw_count, materials, material_count, textures,
                            texture_count, blocks, units16):
        """shadow_trace_textured over a block-resident set (nv_shadow_trace_blocks): the same mask byte for byte"""
        self._shadow_trace_set("nv_shadow_trace_blocks", shadow_data, depth, shadow, width, height, quality, draws, draw_count, materials, material_count,
                               textures, texture_count, blocks, units16)

    def visibility_attributes_blocks(self, globals_, records, width, height, db, draw_count, mlb, meshlet_count, meshlet_data, data_words, vertices,
                                     vertex_count, materials, material_count, attributes=None, gbuffer0=None, gbuffer1=None, totals4=None,
                                     textures=None, texture_count=0, blocks=None, units16=0):
        """visibility_attributes_textured over a block-resident set (nv_visibility_attributes_blocks): textures = a device table
        of layouts.TEXTUREBLOCKDESC (entry 0 reserved), blocks = texture_blocks' buffer of units16 16-byte units.  The same outputs bit for bit"""
        self._visibility_attributes_set("nv_visibility_attributes_blocks", globals_, records, width, height, db, draw_count, mlb, meshlet_count,
                                        meshlet_data, data_words, vertices, vertex_count, materials, material_count, attributes, gbuffer0, gbuffer1,
                                        totals4, textures, texture_count, blocks, units16)

    # ---- material textures; the three host functions need no device and are host.py's
    dds_parse = staticmethod(host.dds_parse)
    texture_set_layout = staticmethod(host.texture_set_layout)
    scenecache_texture_paths = staticmethod(host.scenecache_texture_paths)

    def texture_decode(self, files):
        """decode a texture set on the device (nv_texture_decode, one launch per texture): files = DDS file images (bytes).  Returns (descs:
        host layouts.TEXTUREDESC array with the reserved entry 0, texels: int32 device tensor of the set's RGBA8 words)"""
        from ._lib import TextureDesc
        descs, words, infos = host.texture_set_layout(files)
        texels = torch.zeros(max(1, words), dtype=torch.int32, device=self.device)
        for i, data in enumerate(files):
            info = infos[i]
            payload = np.frombuffer(bytes(data), np.uint8)[info.payloadOffset:]
            blocks = to_device(np.ascontiguousarray(payload), self.device)
            d = TextureDesc(*[int(descs[i + 1][k]) for k in ("offset", "width", "height", "levels")])
            check(lib.nv_texture_decode(self.h, _stream(), _ptr(blocks), info.format, info.width, info.height, info.levels, _ptr(texels), C.byref(d)),
                  "nv_texture_decode")
        return descs, texels

    texture_block_layout = staticmethod(host.texture_block_layout)

    def texture_blocks(self, files):
        """the block-resident form of a texture set: files = DDS file images (bytes).  Returns (descs: host
        layouts.TEXTUREBLOCKDESC array with the reserved entry 0, blocks: uint8 device tensor of 16 * units16 bytes holding the payloads verbatim).
        A plain copy: no kernel and no decode launch"""
        descs, blocks = host.texture_blocks_host(files)
        return descs, to_device(blocks if len(blocks) else np.zeros(16, np.uint8), self.device)

    def shadow_fill(self, shadow, depth, width, height, checkerboard):
        """shadowfill.comp.glsl in place (nv_shadow_fill): the texels of one checkerboard parity of the u8 shadow image become the
        depth-weighted mean of their four neighbours; the other parity keeps its bytes"""
        check(lib.nv_shadow_fill(self.h, _stream(), _ptr(shadow), _ptr(depth), int(width), int(height), int(checkerboard)), "nv_shadow_fill")

    def shadow_blur(self, out, shadow, depth, width, height, direction, znear):
        """shadowblur.comp.glsl (nv_shadow_blur): the 21-tap depth-aware filter of the u8 shadow image along one axis into `out` (another
        image); direction 1 = horizontal, 0 = vertical"""
        check(lib.nv_shadow_blur(self.h, _stream(), _ptr(out), _ptr(shadow), _ptr(depth), int(width), int(height), int(direction), float(znear)),
              "nv_shadow_blur")

    def rt_scene_build(self, meshes, indices, vertices, draws, texcoords=False):
        """the scene blob of the shadow trace (host.rt_scene_build; host only); texcoords: the blob shadow_trace_textured walks"""
        return host.rt_scene_build(meshes, indices, vertices, draws, texcoords=texcoords)

    def rt_scene_upload(self, blob):
        """validate the blob and keep a context-owned device copy (nv_rt_scene_upload: load time, synchronises); None drops it"""
        if blob is None:
            check(lib.nv_rt_scene_upload(self.h, _stream(), None, 0), "nv_rt_scene_upload")
        else:
            check(lib.nv_rt_scene_upload(self.h, _stream(), C.c_void_p(blob.ctypes.data), blob.nbytes), "nv_rt_scene_upload")

    def rt_scene_reserve_dynamic(self, max_draws):
        """room for a TLAS over up to max_draws draws and the rebuild's scratch behind the uploaded scene (nv_rt_scene_reserve_dynamic: load
        time, allocates and synchronises); a later rt_scene_upload drops it"""
        check(lib.nv_rt_scene_reserve_dynamic(self.h, _stream(), int(max_draws)), "nv_rt_scene_reserve_dynamic")

    def rt_tlas_build(self, draws_device, count):
        """rebuild the TLAS of the reserved scene from the first `count` MeshDraw records of the device buffer, read when the launches run
        (nv_rt_tlas_build: only enqueues, can be captured); shadow_trace calls behind it walk the new TLAS"""
        check(lib.nv_rt_tlas_build(self.h, _stream(), _ptr(draws_device), int(count)), "nv_rt_tlas_build")

    def rt_scene_download(self):
        """the context's current scene as a canonical blob, a 16-byte aligned uint8 array (nv_rt_scene_download: synchronises; tests, tools)"""
        n = C.c_uint64(0)
        check(lib.nv_rt_scene_download(self.h, _stream(), None, C.byref(n)), "nv_rt_scene_download")
        out = host._aligned_bytes(n.value)
        room = C.c_uint64(n.value)
        check(lib.nv_rt_scene_download(self.h, _stream(), C.c_void_p(out.ctypes.data), C.byref(room)), "nv_rt_scene_download")
        assert room.value == n.value
        return out

    def shadow_trace_textured(self, shadow_data, depth, shadow, width, height, quality, draws, draw_count, materials, material_count, textures,
                              texture_count, texels, texel_words):
        """shadow_trace with the alpha test of shadow.comp.glsl:86-123 (nv_shadow_trace_textured): at quality 1 a hit on a post-pass instance
        counts only where its material's albedo texture has alpha >= 0.5.  The uploaded scene was built with texcoords=True; draws = the device
        draw array its instances index, materials = a device table of layouts.MATERIAL, textures / texels = texture_decode's set.  One launch,
        can be captured"""
        self._shadow_trace_set("nv_shadow_trace_textured", shadow_data, depth, shadow, width, height, quality, draws, draw_count, materials,
                               material_count, textures, texture_count, texels, texel_words)

    def shadow_trace(self, shadow_data, depth, shadow, width, height, quality=1):
        """shadow.comp.glsl (nv_shadow_trace): the u8 sun shadow mask (0 = in shadow, 255 = lit) of the depth target from the uploaded scene;
        with shadow_data["checkerboard"] > 0 only one parity of the texels is written (shadow_fill fills the other)"""
        check(lib.nv_shadow_trace(self.h, _stream(), C.c_void_p(shadow_data.ctypes.data), _ptr(depth), _ptr(shadow), int(width), int(height), int(quality)),
              "nv_shadow_trace")

    def shade_final(self, shade_data, gbuffer0, gbuffer1, depth, shadow, color, width, height):
        """final.comp.glsl without the bloom term (nv_shade_final): the R8G8B8A8 colour (R in the low byte) of every pixel from the two
        G-buffer words, the depth target and, with shade_data["shadowsEnabled"] == 1, the u8 shadow image (None otherwise)"""
        check(lib.nv_shade_final(self.h, _stream(), C.c_void_p(shade_data.ctypes.data), _ptr(gbuffer0), _ptr(gbuffer1), _ptr(depth), _ptr(shadow),
                                 _ptr(color), int(width), int(height)), "nv_shade_final")

    def bloom_extract(self, gbuffer0, width, height, bloom, desc):
        """bloom.comp.glsl pass 0 (nv_bloom_extract): the emissive term of the full-resolution gbuffer0 into level 0 of the bloom target
        (desc.totalTexels B10G11R11 words; desc = host.bloom_desc(width, height))"""
        check(lib.nv_bloom_extract(self.h, _stream(), _ptr(gbuffer0), int(width), int(height), _ptr(bloom), None if desc is None else C.byref(desc)),
              "nv_bloom_extract")

    def bloom_downsample(self, bloom, desc, level):
        """bloom.comp.glsl pass 1 (nv_bloom_downsample): the 13-tap downsample of level - 1 into level"""
        check(lib.nv_bloom_downsample(self.h, _stream(), _ptr(bloom), None if desc is None else C.byref(desc), int(level)), "nv_bloom_downsample")

    def bloom_upsample(self, bloom, desc, level, radius=2.0):
        """bloom.comp.glsl pass 2 (nv_bloom_upsample): the 9-tap tent of level + 1 added to level in place"""
        check(lib.nv_bloom_upsample(self.h, _stream(), _ptr(bloom), None if desc is None else C.byref(desc), int(level), float(radius)),
              "nv_bloom_upsample")

    def bloom(self, gbuffer0, width, height, bloom, desc):
        """the whole chain of src/niagara.cpp:1873-1901 (nv_bloom): extract, downsample 1 .. levels - 1, upsample levels - 2 .. 0 with radius 2"""
        check(lib.nv_bloom(self.h, _stream(), _ptr(gbuffer0), int(width), int(height), _ptr(bloom), None if desc is None else C.byref(desc)), "nv_bloom")

    def shade_final_bloom(self, shade_data, gbuffer0, gbuffer1, depth, shadow, color, width, height, bloom, desc):
        """final.comp.glsl complete (nv_shade_final_bloom): shade_final plus texture(bloomImage, uv) * 0.1 from level 0 of the bloom target"""
        check(lib.nv_shade_final_bloom(self.h, _stream(), C.c_void_p(shade_data.ctypes.data), _ptr(gbuffer0), _ptr(gbuffer1), _ptr(depth), _ptr(shadow),
                                       _ptr(color), int(width), int(height), _ptr(bloom), None if desc is None else C.byref(desc)), "nv_shade_final_bloom")

    def depthreduce(self, depth, width, height, pyramid):
        check(lib.nv_depthreduce(self.h, _stream(), _ptr(depth), width, height, C.byref(pyramid)), "nv_depthreduce")

    def set_counts_sink(self, out3):
        """the next clustercull calls also write {0, dccb[0], cluster count} (3 x u64) to out3; None turns it off"""
        check(lib.nv_set_counts_sink(self.h, _ptr(out3)), "nv_set_counts_sink")

    def pack_counts(self, a, b, c, out3):
        check(lib.nv_pack_counts(self.h, _stream(), _ptr(a), _ptr(b), _ptr(c), _ptr(out3)), "nv_pack_counts")

    def probe_cluster_scalars(self, cull, dcb, command_count, db, mlb, pyramid=None):
        out = torch.zeros((command_count, 64, 16), dtype=torch.float32, device=self.device)
        check(lib.nv_probe_cluster_scalars(self.h, _stream(), C.c_void_p(cull.ctypes.data), _ptr(dcb), command_count, _ptr(db), _ptr(mlb),
                                           None if pyramid is None else C.byref(pyramid), _ptr(out)), "nv_probe_cluster_scalars")
        return out


class DepthPyramid:
    """replaces the R32F mip-chain image + MIN sampler (src/niagara.cpp:629,1339-1350)"""

    def __init__(self, device, depth_w, depth_h):
        self.desc = host.pyramid_desc(depth_w, depth_h)
        self.data = torch.zeros(self.desc.totalTexels, dtype=torch.float32, device=device)
        self.desc.d_base = self.data.data_ptr()
        self.width, self.height, self.levels = self.desc.width, self.desc.height, self.desc.levels
        self.mip_offset = [int(x) for x in self.desc.mipOffset]

    def level(self, i):
        w, h = max(1, self.width >> i), max(1, self.height >> i)
        return self.data[self.mip_offset[i]:self.mip_offset[i] + w * h].view(h, w)


class VisibilityPipeline:
    """niagara's GPU-driven visibility front-end for one scene on one device."""

    def __init__(self, meshes, meshlets, draws, depth_size, ctx=None, task_capacity=None, cluster_capacity=None, use_soa=True, fused=False,
                 meshlet_data=None, vertices=None, indices=None, near_clip=False, share=None, stable_ids=False):
        self.ctx = ctx or Context()
        # share: a pipeline of the SAME scene on the same device whose scene buffers (meshes, meshlets, draws, geometry) and library
        # mirrors this one uses instead of uploading its own (nv_share_scene); everything a pass writes stays this pipeline's own
        # near_clip=True: both depth rasterisers clip triangles at the near plane instead of dropping them (NV_OPT_RASTER_NEAR_CLIP), so
        # that surfaces the camera stands on or next to occlude in frame()'s late passes
        self.near_clip = bool(near_clip)
        self.ctx.set_option(NV_OPT_RASTER_NEAR_CLIP, int(self.near_clip))
        # stable_ids=True: nv_rasterdepth names a cluster in the visibility word by its meshlet-visibility index instead of its slot in the
        # pass's list (NV_OPT_RASTER_VISIBILITY_ID), so that frame(visibility=) can keep one target over its passes and resolve() can read it
        self.stable_ids = bool(stable_ids)
        self.ctx.set_option(NV_OPT_RASTER_VISIBILITY_ID, int(self.stable_ids))
        # fused=True: the passes absorb the count-word resets and the tasksubmit / clustersubmit fix-ups (same buffer
        # contents, four launches less per phase); fused=False issues the reference's dispatch sequence one to one
        self.fused = bool(fused)
        self.ctx.set_option(NV_OPT_FUSED_COUNT_RESET, int(self.fused))
        self.ctx.set_option(NV_OPT_FUSED_SUBMIT, int(self.fused))
        dev = self.ctx.device
        self.mesh_count, self.meshlet_count, self.draw_count = len(meshes), len(meshlets), len(draws)
        self.draws_host = draws.copy()
        self.slots, self.post_mask = host.assign_visibility_offsets(self.draws_host, meshes)  # src/niagara.cpp:1002-1020
        if share is not None:
            self.mb, self.mlb, self.db = share.mb, share.mlb, getattr(share, "db_all", share.db)
        else:
            self.mb = to_device(meshes, dev)
            self.mlb = to_device(meshlets, dev)
            self.db = to_device(self.draws_host, dev)
        self.dvb = torch.zeros(max(1, self.draw_count), dtype=torch.int32, device=dev)         # zeroed once (:1450-1457)
        self.mvb = torch.zeros(max(1, (self.slots + 31) // 32 + 2), dtype=torch.int32, device=dev)  # (:1459-1468)
        tcap = task_capacity or L.TASK_WGLIMIT
        ccap = cluster_capacity or L.CLUSTER_LIMIT
        # The kernels clamp at the reference's limits (TASK_WGLIMIT commands, CLUSTER_LIMIT indices: the sizes niagara
        # allocates, src/niagara.cpp:1070,1088), not at the size of a smaller buffer.  Smaller buffers are accepted only when
        # no pass over this scene can fill them: every draw emitting its largest LOD (+ the submit kernels' padding).
        lod_counts = meshes["lods"]["meshletCount"].astype(np.int64)
        lod_valid = np.arange(lod_counts.shape[1])[None, :] < meshes["lodCount"][:, None]
        per_mesh = np.where(lod_valid, lod_counts, 0).max(axis=1) if len(meshes) else np.zeros(0, np.int64)
        mi = np.minimum(draws["meshIndex"].astype(np.int64), max(0, len(meshes) - 1))
        worst_meshlets = int(per_mesh[mi].sum()) if len(draws) and len(meshes) else 0
        worst_tasks = int(((per_mesh[mi] + 63) // 64).sum()) if len(draws) and len(meshes) else 0
        if tcap < min(worst_tasks, L.TASK_WGLIMIT) or ccap < min(worst_meshlets, L.CLUSTER_LIMIT):
            raise NvError("task_capacity %d / cluster_capacity %d cannot hold what this scene can emit (%d task commands, %d meshlets): the passes "
                          "drop output only at the reference's limits, never at a smaller buffer's end" % (tcap, ccap, worst_tasks, worst_meshlets))
        dcb_bytes = tcap * L.TASKCMD.itemsize + 64 * L.TASKCMD.itemsize
        if indices is not None:  # the classic path (frame(task=False)) also writes one MeshDrawCommand per draw into dcb
            dcb_bytes = max(dcb_bytes, max(1, self.draw_count) * L.DRAWCMD.itemsize)
            whole = L.TASKCMD.itemsize * L.DRAWCMD.itemsize  # a whole number of records of either kind (from_device views it as both)
            dcb_bytes = (dcb_bytes + whole - 1) // whole * whole
        self.dcb = torch.zeros(dcb_bytes, dtype=torch.uint8, device=dev)
        self.dccb = torch.zeros(4, dtype=torch.int32, device=dev)
        self.cib = torch.zeros(ccap + 256, dtype=torch.int32, device=dev)
        self.ccb = torch.zeros(4, dtype=torch.int32, device=dev)
        self.depth_w, self.depth_h = depth_size
        self.pyramid = DepthPyramid(dev, *depth_size)
        self.ctx.reserve(self.draw_count, tcap)
        if share is not None:
            self.ctx.share_scene(share.ctx)
        else:
            self.ctx.upload_meshes(self.mb, self.mesh_count)
            if use_soa and self.meshlet_count:
                self.ctx.upload_meshlets(self.mlb, self.meshlet_count)
            if use_soa and self.draw_count:
                self.ctx.upload_draws(self.db, self.draw_count, self.mb)
        self.draws_mirrored = share is None and bool(use_soa) and self.draw_count > 0  # move_draws keeps the mirror in step
        # geometry (meshlet payloads and / or the index buffer ib, + vertices, src/scene.cpp:24-47): with it the pipeline rasterises its own
        # depth target, through the clusters (meshlet_data) or through the indexed draws of the classic path (indices)
        self.mdb = self.vb = self.ib = self.depth = None
        self.bloom_image = self.bloom_desc = None  # shade(bloom=True)'s target, allocated on first use
        self.rt_dynamic = False                    # build_rt_scene(dynamic=True): move_draws rebuilds the TLAS
        self.rt_texcoords = False                  # build_rt_scene(texcoords=True): shade(shadow="trace", textures=True) can run its alpha test
        self.rt_scene = self.shadow_image = None   # build_rt_scene's blob; shade(shadow="trace")'s mask, allocated on first use
        self.texture_resident = None               # set_textures' residency: "decoded" or "blocks"
        self.index_count = self.vertex_count = 0
        if vertices is not None and (meshlet_data is not None or indices is not None):
            self.vertex_count = len(vertices)
            self.depth = torch.zeros((self.depth_h, self.depth_w), dtype=torch.float32, device=dev)
            if indices is not None:
                self.index_count = len(indices)
            if share is not None:
                self.vb, self.mdb, self.ib = share.vb, share.mdb if meshlet_data is not None else None, share.ib if indices is not None else None
            else:
                self.vb = to_device(vertices, dev) if len(vertices) else torch.zeros(L.VERTEX.itemsize, dtype=torch.uint8, device=dev)
                if meshlet_data is not None:
                    self.mdb = to_device(meshlet_data, dev) if len(meshlet_data) else torch.zeros(4, dtype=torch.uint8, device=dev)
                if indices is not None:
                    ind = np.ascontiguousarray(indices, np.uint32)
                    self.ib = to_device(ind, dev) if len(ind) else torch.zeros(4, dtype=torch.uint8, device=dev)
        # the names of the triangles of the classic path: with the index buffer and stable ids the indexed raster can write a
        # visibility target too (render_draws / frame(task=False, visibility=)).  The prefix is the scene's, also on a shard; it is built and
        # uploaded by the first call that needs it (_triangle_names), so a pipeline that never asks for it costs nothing and constructs as before
        self.tob = self.triangle_offsets = None
        self._meshes_host = meshes if self.ib is not None and self.stable_ids else None

    # src/niagara.cpp:1530-1574
    def cull(self, cull_data, late, task=True, post_pass=0):
        if not self.fused:
            self.ctx.reset_count(self.dccb)                         # vkCmdFillBuffer(dccb, 0, 4, 0)  (:1541)
        pass_data = cull_data.copy()
        pass_data["clusterBackfaceEnabled"] = 1 if post_pass == 0 else 0   # (:1549)
        pass_data["postPass"] = post_pass
        self.ctx.drawcull(pass_data, late, task, self.db, self.mb, self.dcb, self.dccb, self.dvb, self.pyramid.desc)
        if task and not self.fused:
            self.ctx.tasksubmit(self.dccb, self.dcb)                # (:1563-1568)

    # src/niagara.cpp:1582-1611 (cluster branch of render())
    def render_clusters(self, cull_data, late, post_pass=0):
        if not self.fused:
            self.ctx.reset_count(self.ccb)                          # vkCmdFillBuffer(ccb, 0, 4, 0)  (:1586)
        pass_data = cull_data.copy()
        pass_data["postPass"] = post_pass                           # (:1595-1596)
        self.ctx.clustercull(pass_data, late, self.dcb, self.dccb, self.db, self.mlb, self.mvb, self.pyramid.desc, self.cib, self.ccb)
        if not self.fused:
            self.ctx.clustersubmit(self.ccb, self.cib)

    # src/niagara.cpp:1703-1733
    def build_pyramid(self, depth):
        self.ctx.depthreduce(depth, self.depth_w, self.depth_h, self.pyramid.desc)

    def render_depth(self, cull_data, late, post_pass=0, visibility=None, totals4=None, textures=False, materials=None, alpha_totals2=None):
        """the raster of render() (src/niagara.cpp:1582-1611): the clusters of the last render_clusters into self.depth.  The early pass
        clears the target first (LOAD_OP_CLEAR, depthClear = 0), the late and post passes load it.  textures=True: the raster is
        nv_rasterdepth_textured over set_textures()'s set and `materials` (a host array of layouts.MATERIAL or a device tensor of them): the
        covered samples of a post pass also pass the alpha test of mesh.frag.glsl:88 (a pass with post_pass = 0 writes the same bits either way);
        alpha_totals2 (optional): samples dropped, samples unevaluated"""
        if self.mdb is None:
            raise NvError("render_depth needs the scene's geometry: VisibilityPipeline(..., meshlet_data=, vertices=)")
        if not late:
            self.depth.zero_()
            if visibility is not None and self.stable_ids:  # one target for the frame: cleared with the depth, loaded by late / post
                visibility.zero_()
        pass_data = cull_data.copy()
        pass_data["postPass"] = post_pass
        g = synth.make_globals(pass_data, (self.depth_w, self.depth_h))
        if textures:
            missing = [what for what, absent in (("set_textures()", self.texture_resident is None),
                                                 ("a material table (materials=)", materials is None)) if absent]
            if missing:
                raise NvError("render_depth(textures=True) needs " + ", ".join(missing))
            mat = to_device(np.ascontiguousarray(materials, L.MATERIAL), self.ctx.device) if isinstance(materials, np.ndarray) else materials
            form, tset = self._texture_set()
            getattr(self.ctx, "rasterdepth_" + form)(g, self.dcb, self.db, self.mlb, self.mdb, self.vb, self.cib, self.ccb, self.depth, self.depth_w,
                                                     self.depth_h, visibility, totals4, mat, mat.numel() * mat.element_size() // L.MATERIAL.itemsize,
                                                     *tset, alpha_totals2)
            return
        self.ctx.rasterdepth(g, self.dcb, self.db, self.mlb, self.mdb, self.vb, self.cib, self.ccb, self.depth, self.depth_w, self.depth_h,
                             visibility, totals4)

    def _triangle_names(self, what):
        """the scene's triangle offsets on the device (nv_assign_triangle_offsets), built on first use; NvError when the pipeline has no index
        buffer or no stable ids, or the scene holds more than 2^34 - 2 triangle names"""
        if self.tob is None:
            if self._meshes_host is None:
                raise NvError(what + " names triangles by a frame-stable id: VisibilityPipeline(..., indices=, vertices=, stable_ids=True)")
            self.triangle_offsets = host.assign_triangle_offsets(self.draws_host, self._meshes_host)
            self.tob = to_device(self.triangle_offsets, self.ctx.device)
        return self.tob

    def _draw_triangle_offsets(self):
        """the triangle offsets of the draws the passes run on (a shard: the scene's prefix from its first draw on)"""
        return self._triangle_names("render_draws(visibility=)")

    def render_draws(self, cull_data, late, post_pass=0, totals4=None, visibility=None, textures=False, materials=None, alpha_totals2=None):
        """the classic branch of render() (src/niagara.cpp:1680-1694): the MeshDrawCommands of the last cull(task=False) drawn from ib into
        self.depth.  The early pass clears the target first, the late and post passes load it.  visibility (stable_ids=True): a u64 target
        that takes the stable-form word of nv_rasterdepth_indexed_visibility, cleared and loaded with the depth; resolve(classic=True) reads it.
        textures=True: the raster is nv_rasterdepth_indexed_textured (or _blocks, by set_textures()'s residency) over `materials` (a host array
        of layouts.MATERIAL or a device tensor of them): the covered samples of a post pass also pass the alpha test of mesh.frag.glsl:88 (a
        pass with post_pass = 0 writes the same bits either way); alpha_totals2 (optional): samples dropped, samples unevaluated"""
        if self.ib is None:
            raise NvError("render_draws needs the index buffer: VisibilityPipeline(..., indices=, vertices=)")
        if textures:
            missing = [what for what, absent in (("set_textures()", self.texture_resident is None),
                                                 ("a material table (materials=)", materials is None)) if absent]
            if missing:
                raise NvError("render_draws(textures=True) needs " + ", ".join(missing))
        offsets = None if visibility is None else self._draw_triangle_offsets()  # (raises before anything is cleared)
        if not late:
            self.depth.zero_()
            if visibility is not None:
                visibility.zero_()
        pass_data = cull_data.copy()
        pass_data["postPass"] = post_pass
        g = synth.make_globals(pass_data, (self.depth_w, self.depth_h))
        if textures:
            mat = to_device(np.ascontiguousarray(materials, L.MATERIAL), self.ctx.device) if isinstance(materials, np.ndarray) else materials
            form, tset = self._texture_set()
            getattr(self.ctx, "rasterdepth_indexed_" + form)(g, self.dcb, self.dccb, self.db, self.draw_count, self.ib, self.index_count, self.vb,
                                                             self.vertex_count, self.depth, self.depth_w, self.depth_h, offsets, visibility, totals4, mat,
                                                             mat.numel() * mat.element_size() // L.MATERIAL.itemsize, *tset, alpha_totals2)
            return
        if visibility is not None:
            self.ctx.rasterdepth_indexed_visibility(g, self.dcb, self.dccb, self.db, self.draw_count, self.ib, self.index_count, self.vb,
                                                    self.vertex_count, self.depth, self.depth_w, self.depth_h, offsets, visibility, totals4)
            return
        self.ctx.rasterdepth_indexed(g, self.dcb, self.dccb, self.db, self.draw_count, self.ib, self.index_count, self.vb, self.vertex_count,
                                     self.depth, self.depth_w, self.depth_h, totals4)

    def new_visibility(self):
        """a cleared visibility target of the depth target's size (u64 words, held as int64)"""
        return torch.zeros((self.depth_h, self.depth_w), dtype=torch.int64, device=self.ctx.device)

    def resolve(self, cull_data, visibility, records=True, meshlet_seen=True, draw_pixels=True, classic=False):
        """nv_visibility_resolve of a frame's stable-form visibility target under the frame's CullData: a dict with "records" (uint8 tensor,
        height * width NvVisRecord), "meshlet_seen" (int32, mvb's size and layout), "draw_pixels" (int32 per draw of the whole scene) and
        "totals" (int64: covered, unresolved, 0, 0); an output switched off is None.  Draw ids are the scene's, also on a shard.
        classic=True: the target is a classic frame's (frame(task=False, visibility=)): nv_visibility_resolve_indexed, "records" are
        NvVisIndexedRecords and "meshlet_seen" is None (the classic path has no meshlets)"""
        if not self.stable_ids:
            raise NvError("resolve reads the stable form of the visibility word: VisibilityPipeline(..., stable_ids=True)")
        dev = self.ctx.device
        n_draws = getattr(self, "total_draws", self.draw_count)
        if classic:
            tob = self._triangle_names("resolve(classic=True)")
            out = dict(records=torch.zeros(self.depth_w * self.depth_h * L.VISINDEXEDRECORD.itemsize, dtype=torch.uint8, device=dev) if records else None,
                       meshlet_seen=None, draw_pixels=torch.zeros(max(1, n_draws), dtype=torch.int32, device=dev) if draw_pixels else None,
                       totals=torch.zeros(4, dtype=torch.int64, device=dev))
            self.ctx.visibility_resolve_indexed(cull_data, visibility, self.depth_w, self.depth_h, getattr(self, "db_all", self.db), n_draws, self.mb,
                                                self.mesh_count, tob, out["records"], out["draw_pixels"], out["totals"])
            return out
        out = dict(records=torch.zeros(self.depth_w * self.depth_h * L.VISRECORD.itemsize, dtype=torch.uint8, device=dev) if records else None,
                   meshlet_seen=torch.zeros_like(self.mvb) if meshlet_seen else None,
                   draw_pixels=torch.zeros(max(1, n_draws), dtype=torch.int32, device=dev) if draw_pixels else None,
                   totals=torch.zeros(4, dtype=torch.int64, device=dev))
        self.ctx.visibility_resolve(cull_data, visibility, self.depth_w, self.depth_h, getattr(self, "db_all", self.db), n_draws, self.mb, self.mesh_count,
                                    out["records"], out["meshlet_seen"], out["draw_pixels"], out["totals"])
        return out

    def set_textures(self, files, resident="decoded"):
        """the scene's material textures, once per scene: a list of DDS file images (bytes) or paths, in texturePaths order — textures[i + 1]
        is files[i], as niagara binds them (src/niagara.cpp:934).  resident="decoded": decoded on the device to RGBA8 mip chains;
        attributes(textures=True) samples them.  resident="blocks" (DESIGN.md §4.21): the DDS payloads stay as they are (4-8 x smaller) and
        attributes(textures=True), render_depth / frame(textures=True) and shade(shadow="trace", textures=True) decode each tap from its block,
        to the same bits.  texture_resident_bytes: the bytes of the set's device buffer"""
        if resident not in ("decoded", "blocks"):
            raise NvError("set_textures: resident is \"decoded\" or \"blocks\"")
        data = []
        for f in files:
            if isinstance(f, (bytes, bytearray, memoryview)):
                data.append(bytes(f))
            else:
                with open(f, "rb") as fh:
                    data.append(fh.read())
        self.texture_resident = resident
        if resident == "blocks":
            descs, self.texture_block_buffer = self.ctx.texture_blocks(data)
            self.texels = None
            self.texture_resident_bytes = int(self.texture_block_buffer.numel()) if len(data) else 0
        else:
            descs, self.texels = self.ctx.texture_decode(data)
            self.texture_block_buffer = None
            self.texture_resident_bytes = int(self.texels.numel()) * 4 if len(data) else 0
        self.texture_descs = descs
        self.texture_table = to_device(descs, self.ctx.device)

    def _texture_set(self):
        """what a pass over set_textures()'s set needs for the set's residency: the suffix of the Context method ("textured" or "blocks") and
        that method's last four set arguments (the descriptor table, its entries, the set's buffer, the buffer's size in words or 16-byte units)"""
        if self.texture_resident == "blocks":
            return "blocks", (self.texture_table, len(self.texture_descs), self.texture_block_buffer, self.texture_block_buffer.numel() // 16)
        return "textured", (self.texture_table, len(self.texture_descs), self.texels, self.texels.numel())

    def attributes(self, cull_data, records, materials=None, attributes=True, gbuffers=True, textures=False, classic=False):
        """nv_visibility_attributes over resolve()'s "records" under the frame's CullData: a dict with "attributes" (uint8 tensor, height *
        width NvPixelAttributes), "gbuffer0" / "gbuffer1" (int32, height x width; only with `materials`, a host array of layouts.MATERIAL or a
        device tensor of them) and "totals" (int64: shaded, invalid, degenerate, textured); an output switched off is None.  The records are
        global (the scene's draw ids), so this works unchanged on any rank of a sharded frame after the composite.  textures=True runs
        nv_visibility_attributes_textured over set_textures()'s set: the complete fragment stage; totals[3] then counts only the pixels whose
        material names a texture the set does not hold.  classic=True: `records` are resolve(classic=True)'s and the pass is
        nv_visibility_attributes_indexed, with textures=True nv_visibility_attributes_indexed_textured (or _blocks)"""
        if not self.stable_ids:
            raise NvError("attributes reads resolve()'s records: VisibilityPipeline(..., stable_ids=True)")
        if classic and self.ib is None:
            raise NvError("attributes(classic=True) needs the index buffer: VisibilityPipeline(..., indices=, vertices=)")
        if not classic and self.mdb is None:
            raise NvError("attributes needs the scene's geometry: VisibilityPipeline(..., meshlet_data=, vertices=)")
        dev = self.ctx.device
        n = self.depth_w * self.depth_h
        mat, n_mat = materials, 0
        if materials is not None:
            if isinstance(materials, np.ndarray):
                mat = to_device(np.ascontiguousarray(materials, L.MATERIAL), dev)
            n_mat = mat.numel() * mat.element_size() // L.MATERIAL.itemsize
        out = dict(attributes=torch.zeros(n * L.PIXELATTR.itemsize, dtype=torch.uint8, device=dev) if attributes else None,
                   gbuffer0=torch.zeros((self.depth_h, self.depth_w), dtype=torch.int32, device=dev) if gbuffers and mat is not None else None,
                   gbuffer1=torch.zeros((self.depth_h, self.depth_w), dtype=torch.int32, device=dev) if gbuffers and mat is not None else None,
                   totals=torch.zeros(4, dtype=torch.int64, device=dev))
        g = synth.make_globals(cull_data, (self.depth_w, self.depth_h))
        n_draws = getattr(self, "total_draws", self.draw_count)
        if textures:
            if self.texture_resident is None:
                raise NvError("attributes(textures=True) samples set_textures()'s set: call set_textures first")
            if mat is None:
                raise NvError("attributes(textures=True) needs the material table")
            form, tset = self._texture_set()
            if classic:
                getattr(self.ctx, "visibility_attributes_indexed_" + form)(g, records, self.depth_w, self.depth_h, getattr(self, "db_all", self.db), n_draws,
                                                                           self.ib, self.index_count, self.vb, self.vertex_count, mat, n_mat,
                                                                           out["attributes"], out["gbuffer0"], out["gbuffer1"], out["totals"], *tset)
                return out
            getattr(self.ctx, "visibility_attributes_" + form)(g, records, self.depth_w, self.depth_h, getattr(self, "db_all", self.db), n_draws, self.mlb,
                                                               self.meshlet_count, self.mdb, self.mdb.numel() * self.mdb.element_size() // 4, self.vb,
                                                               self.vertex_count, mat, n_mat, out["attributes"], out["gbuffer0"], out["gbuffer1"],
                                                               out["totals"], *tset)
            return out
        if classic:
            self.ctx.visibility_attributes_indexed(g, records, self.depth_w, self.depth_h, getattr(self, "db_all", self.db), n_draws, self.ib,
                                                   self.index_count, self.vb, self.vertex_count, mat, n_mat, out["attributes"], out["gbuffer0"],
                                                   out["gbuffer1"], out["totals"])
            return out
        self.ctx.visibility_attributes(g, records, self.depth_w, self.depth_h, getattr(self, "db_all", self.db), n_draws, self.mlb, self.meshlet_count,
                                       self.mdb, self.mdb.numel() * self.mdb.element_size() // 4, self.vb, self.vertex_count, mat, n_mat,
                                       out["attributes"], out["gbuffer0"], out["gbuffer1"], out["totals"])
        return out

    def build_rt_scene(self, meshes, indices, vertices, draws, dynamic=False, texcoords=False):
        """build the ray-tracing scene of shade(shadow="trace") on the host and upload it, once per scene (niagara builds its BLAS / TLAS at
        load time, src/scenert.cpp): `meshes` with their LODs' index ranges set (synth.indexed_geometry) and the index buffer of the classic
        path.  The scene is static: call again when draws move — or pass dynamic=True, which reserves room for a TLAS over the pipeline's
        draw count (nv_rt_scene_reserve_dynamic), and move the draws through move_draws, which rebuilds the TLAS on the device.
        texcoords=True builds the scene shade(shadow="trace", textures=True) needs (nv_rt_scene_build_textured).  Returns the blob"""
        if texcoords and isinstance(self, ShardedVisibilityPipeline):
            raise NvError("build_rt_scene(texcoords=True) is not available on a sharded pipeline")
        self.rt_scene = self.ctx.rt_scene_build(meshes, indices, vertices, draws, texcoords=texcoords)
        self.rt_texcoords = bool(texcoords)
        self.ctx.rt_scene_upload(self.rt_scene)
        if dynamic and isinstance(self, ShardedVisibilityPipeline):
            raise NvError("build_rt_scene(dynamic=True) is not available on a sharded pipeline")
        self.rt_dynamic = bool(dynamic) and self.draw_count > 0
        if self.rt_dynamic:
            self.ctx.rt_scene_reserve_dynamic(self.draw_count)
        return self.rt_scene

    def move_draws(self, first, records):
        """the animation path (src/niagara.cpp:1385-1400, :1482): copies `records` (layouts.MESHDRAW; the caller evaluates its keyframes) over
        the draws [first, first + len(records)) of the device draw buffer, keeping the pipeline's own visibility slots, re-evaluates the cull
        mirror (nv_update_draws) and, with a dynamic ray-tracing scene, rebuilds its TLAS from the whole draw buffer (nv_rt_tlas_build).  All
        in stream order: the next frame() and shade(shadow="trace") see the moved draws"""
        rec = np.ascontiguousarray(records, L.MESHDRAW).copy()
        first = int(first)
        if first < 0 or first + len(rec) > self.draw_count:
            raise NvError("move_draws: [%d, %d) is outside the pipeline's %d draws" % (first, first + len(rec), self.draw_count))
        if isinstance(self, ShardedVisibilityPipeline):
            raise NvError("move_draws is not available on a sharded pipeline")
        if len(rec) == 0:
            return
        rec["meshletVisibilityOffset"] = self.draws_host["meshletVisibilityOffset"][first:first + len(rec)]
        self.draws_host[first:first + len(rec)] = rec
        size = L.MESHDRAW.itemsize
        self.db.view(torch.uint8).reshape(-1)[first * size:(first + len(rec)) * size].copy_(to_device(rec, self.ctx.device).view(torch.uint8).reshape(-1))
        if self.draws_mirrored:
            self.ctx.update_draws(self.db, first, len(rec))
        if getattr(self, "rt_dynamic", False):
            self.ctx.rt_tlas_build(self.db, self.draw_count)

    def set_animations(self, animations, keyframes):
        """upload the scene's animations (layouts.ANIMATION / KEYFRAME, e.g. host.scenecache_animations' or synth.orbit_animations') for
        animate(); their drawIndex is checked against the pipeline's draw count, light targets are not driven here (light_count 0: an
        animation with lightIndex >= 0 is refused).  None drops them"""
        if isinstance(self, ShardedVisibilityPipeline):
            raise NvError("set_animations is not available on a sharded pipeline")
        self.ctx.upload_animations(animations, keyframes, self.draw_count, 0)

    def animate(self, time):
        """the animation path on the device (src/niagara.cpp:1362-1411, :1482): evaluates the uploaded animations at `time` into the device
        draw buffer (nv_animate_draws: the cull mirror is rewritten in the same launch) and, with a dynamic ray-tracing scene, rebuilds its TLAS
        (nv_rt_tlas_build).  All in stream order, nothing crosses the bus: the next frame() and shade(shadow="trace") see the moved draws.
        draws_host is NOT rewritten and goes stale: it keeps only what move_draws needs from it, the visibility offsets (which no animation
        changes); download_draws() returns the device records"""
        if isinstance(self, ShardedVisibilityPipeline):
            raise NvError("animate is not available on a sharded pipeline")
        self.ctx.animate_draws(time, self.db, self.draw_count)
        if getattr(self, "rt_dynamic", False):
            self.ctx.rt_tlas_build(self.db, self.draw_count)

    def download_draws(self):
        """the device draw records (layouts.MESHDRAW) as animate() / move_draws left them (synchronises)"""
        return from_device(self.db, L.MESHDRAW, self.draw_count).copy()

    def shade(self, cull_data, gbuffer0, gbuffer1, camera_position, sun_direction, shadow=None, blur=True, checkerboard=False, bloom=False, quality=1,
              textures=False, materials=None):
        """the shading end of the frame over attributes()'s G-buffer words and the pipeline's own depth target (src/niagara.cpp:1792-1850,
        1906-1925): returns the colour tensor (int32, height x width, R8G8B8A8 with R in the low byte).  shadow: a caller-supplied mask (uint8
        tensor, height x width) — it is filled in place when `checkerboard`, blurred horizontally into an image
        the pipeline owns and vertically back into the mask when `blur`, and final shades with shadows on; without a mask final runs
        with shadows off.  shadow="trace" (after build_rt_scene): the mask is ray traced first (nv_shadow_trace with `quality`, sunJitter 1e-2
        when `blur`, else 0, one checkerboard parity when `checkerboard`) into a mask the pipeline owns (self.shadow_image), then treated the
        same way.  textures=True (with shadow="trace"): the trace runs the alpha test of shadow.comp.glsl:86-123 (nv_shadow_trace_textured) over
        set_textures()'s set, `materials` (a host array of layouts.MATERIAL or a device tensor of them) and a scene built with
        build_rt_scene(..., texcoords=True); NvError names whichever of the three is missing.  bloom: run the bloom chain over gbuffer0 into a target the pipeline owns (self.bloom_image, self.bloom_desc) and
        add its term in final (src/niagara.cpp:1866-1904); the default leaves it out, as before"""
        if self.depth is None:
            raise NvError("shade reads the pipeline's depth target: VisibilityPipeline(..., meshlet_data=, vertices=)")
        w, h = self.depth_w, self.depth_h
        dev = self.ctx.device
        g = synth.make_globals(cull_data, (w, h))
        if isinstance(shadow, str):
            if shadow != "trace":
                raise NvError("shade: shadow is None, a mask or \"trace\"")
            if self.rt_scene is None:
                raise NvError("shade(shadow=\"trace\") walks the ray-tracing scene: build_rt_scene(meshes, indices, vertices, draws) first")
            if self.shadow_image is None:
                self.shadow_image = torch.zeros((h, w), dtype=torch.uint8, device=dev)
            shadow = self.shadow_image
            sh = host.build_shadow_data(g, sun_direction, 1e-2 if blur else 0.0, 1 if checkerboard else 0, w, h)  # src/niagara.cpp:1810-1815
            if textures:
                if isinstance(self, ShardedVisibilityPipeline):
                    raise NvError("shade(shadow=\"trace\", textures=True) is not available on a sharded pipeline")
                missing = [what for what, absent in (("set_textures()", self.texture_resident is None),
                                                     ("a material table (materials=)", materials is None),
                                                     ("a scene with texcoords (build_rt_scene(..., texcoords=True))", not getattr(self, "rt_texcoords", False)))
                           if absent]
                if missing:
                    raise NvError("shade(shadow=\"trace\", textures=True) needs " + ", ".join(missing))
                mat = to_device(np.ascontiguousarray(materials, L.MATERIAL), dev) if isinstance(materials, np.ndarray) else materials
                form, tset = self._texture_set()
                getattr(self.ctx, "shadow_trace_" + form)(sh, self.depth, shadow, w, h, quality, self.db, self.draw_count, mat,
                                                          mat.numel() * mat.element_size() // L.MATERIAL.itemsize, *tset)
            else:
                self.ctx.shadow_trace(sh, self.depth, shadow, w, h, quality)
        if shadow is not None:
            if shadow.dtype != torch.uint8 or shadow.numel() != w * h or not shadow.is_contiguous():
                raise NvError("shade: the shadow mask is a contiguous uint8 tensor of the depth target's size")
            if checkerboard:
                self.ctx.shadow_fill(shadow, self.depth, w, h, 1)
            if blur:
                if getattr(self, "shadow_blur_image", None) is None:
                    self.shadow_blur_image = torch.zeros((h, w), dtype=torch.uint8, device=dev)
                znear = float(cull_data["znear"][0])
                self.ctx.shadow_blur(self.shadow_blur_image, shadow, self.depth, w, h, 1, znear)  # src/niagara.cpp:1836-1850
                self.ctx.shadow_blur(shadow, self.shadow_blur_image, self.depth, w, h, 0, znear)
        sd = host.build_shade_data(g, camera_position, sun_direction, 1 if shadow is not None else 0, w, h)
        color = torch.zeros((h, w), dtype=torch.int32, device=dev)
        if bloom:
            if self.bloom_image is None:
                self.bloom_desc = host.bloom_desc(w, h)
                self.bloom_image = torch.zeros(self.bloom_desc.totalTexels, dtype=torch.int32, device=dev)
            self.ctx.bloom(gbuffer0, w, h, self.bloom_image, self.bloom_desc)
            self.ctx.shade_final_bloom(sd, gbuffer0, gbuffer1, self.depth, shadow, color, w, h, self.bloom_image, self.bloom_desc)
        else:
            self.ctx.shade_final(sd, gbuffer0, gbuffer1, self.depth, shadow, color, w, h)
        return color

    def frame(self, cull_data, post_pass=False, on_phase=None, task=True, visibility=None, textures=False, materials=None):
        """one frame of src/niagara.cpp:1765-1788 with the raster in place of the graphics passes: early cull -> clusters -> raster ->
        pyramid -> late cull -> clusters -> raster (-> post cull -> clusters -> raster).  task=False runs the classic path instead (no mesh
        shading): every cull writes MeshDrawCommands, render_draws rasterises them, and clusterOcclusionEnabled is 0 (src/niagara.cpp:1516).
        on_phase(name) is called after each phase's raster ("early", "late", "post").  visibility (stable_ids=True, task=True): a u64
        target of the depth target's size that the three rasters share (cleared before the early one); resolve() reads it — with task=False
        (and indices=) the indexed raster writes it and resolve(classic=True) / attributes(classic=True) read it.  textures=True
        (after set_textures, with `materials`): the post phase's raster is the alpha-tested one, render_depth(textures=True) or with task=False
        render_draws(textures=True); the early and late phases stay on the plain entry points (their bits are the same through either)"""
        if textures and not task:
            missing = [what for what, absent in (("the index buffer (indices=)", self.ib is None), ("set_textures()", self.texture_resident is None),
                                                 ("a material table (materials=)", materials is None)) if absent]
            if missing:  # (before the early phase clears or launches anything)
                raise NvError("frame(task=False, textures=True) needs " + ", ".join(missing))
        if visibility is not None and not self.stable_ids:
            raise NvError("frame(visibility=) needs stable ids: VisibilityPipeline(..., stable_ids=True) "
                          "(the slot index of the default visibility word does not outlive a pass)")
        if not task:
            cull_data = cull_data.copy()
            cull_data["clusterOcclusionEnabled"] = 0
        phases = [("early", False, 0), ("late", True, 0)] + ([("post", True, 1)] if post_pass else [])
        for name, late, pp in phases:
            if name == "late":
                self.build_pyramid(self.depth)
            self.cull(cull_data, late=late, task=task, post_pass=pp)
            if task:
                self.render_clusters(cull_data, late=late, post_pass=pp)
                if textures and pp:
                    self.render_depth(cull_data, late=late, post_pass=pp, visibility=visibility, textures=True, materials=materials)
                else:
                    self.render_depth(cull_data, late=late, post_pass=pp, visibility=visibility)
            elif textures and pp:
                self.render_draws(cull_data, late=late, post_pass=pp, visibility=visibility, textures=True, materials=materials)
            else:
                self.render_draws(cull_data, late=late, post_pass=pp, visibility=visibility)
            if on_phase is not None:
                on_phase(name)

    def visible_clusters(self):
        n = int(self.ccb[0].item())
        return self.cib[:min(n, L.CLUSTER_LIMIT)].cpu().numpy().view(np.uint32), n


class ShardedVisibilityPipeline(VisibilityPipeline):
    """One rank's share of VisibilityPipeline.frame, sharded by a contiguous range of draws.

    The scene is uploaded in full (draws replicated, no meshlet data exchanged); the passes run on d_draws + begin and
    d_drawVisibility + begin with CullData.drawCount = end - begin, so the rank's commands carry rank-local drawIds, while
    meshletVisibilityOffset stays the global prefix: the rank's full-size mvb only ever gets bits of its own draws.  After each phase's
    raster the ranks' depth targets are composited (element-wise maximum, in place on every rank), so every rank builds the unsharded
    frame's pyramid and takes the unsharded frame's decisions for its draws; shard.stitch_* reassemble the unsharded outputs.

    Two deployments:
      - one rank per process: ShardedVisibilityPipeline(..., rank=, world=, group=True or a process group); frame() composites with
        shard.composite_depth (one all_reduce(MAX) per phase on the pass stream);
      - several shards in one process on one device: ShardedVisibilityPipeline.local_shards(..., world=) returns a LocalShards, whose
        pipelines share one upload (nv_share_scene) and composite with nv_depth_merge.

    Equality with the unsharded frame holds while no rank, and not the unsharded frame, reaches NV_TASK_WGLIMIT / NV_CLUSTER_LIMIT (past
    them each rank drops its own tail).  With stable_ids=True frame(visibility=) also composites the visibility target (unsigned 64-bit
    maximum: every rank writes the same word for the same sample, so the composite is the unsharded buffer) and resolve() on any rank
    returns the unsharded frame's records with the scene's draw ids; without it the slot index of the word is rank-local and a
    visibility target is refused.

    Out of scope here: material textures (set_textures is refused; the textured pass is per pixel and works on any rank through the
    Context) and moving draws.  move_draws, set_animations / animate and build_rt_scene(dynamic=True) (the TLAS rebuilt on
    the device) are refused on a sharded pipeline: the ranks' draw buffers and mirrors would have to move together."""

    def set_textures(self, files):
        raise NvError("set_textures is not available on a sharded pipeline: decode the set with Context.texture_decode and run the textured "
                      "attribute pass (per pixel, on any rank) through Context.visibility_attributes_textured")

    def __init__(self, meshes, meshlets, draws, depth_size, rank=0, world=1, draw_range=None, weight="draws", group=None, **kw):
        from . import shard
        super().__init__(meshes, meshlets, draws, depth_size, **kw)
        self.rank, self.world, self.group = int(rank), int(world), group
        if draw_range is None:
            if not 0 <= self.rank < self.world:
                raise NvError("rank %d is not in [0, %d)" % (self.rank, self.world))
            draw_range = shard.draw_ranges(self.draws_host, meshes, self.world, weight)[self.rank]
        self.begin, self.end = int(draw_range[0]), int(draw_range[1])
        if not 0 <= self.begin < self.end <= len(draws):
            raise NvError("draw range [%d, %d) is empty or outside the scene's %d draws: use at most as many ranks as draws" %
                          (self.begin, self.end, len(draws)))
        if self.depth is None:
            raise NvError("a sharded frame rasterises its own depth: ShardedVisibilityPipeline(..., vertices=, meshlet_data= and / or indices=)")
        # the passes of the base class run on these: the rank's records inside the full buffers
        self.total_draws = self.draw_count
        self.db_all, self.dvb_all = self.db, self.dvb
        self.db = self.db_all[self.begin * L.MESHDRAW.itemsize:]
        self.dvb = self.dvb_all[self.begin:self.end]
        self.draw_count = self.end - self.begin

    @classmethod
    def local_shards(cls, meshes, meshlets, draws, depth_size, world, weight="draws", ranges=None, **kw):
        """`world` shards of one scene in this process on the current device: one upload, one context per shard (nv_share_scene)"""
        from . import shard
        draws = draws.copy()
        host.assign_visibility_offsets(draws, meshes)
        ranges = ranges or shard.draw_ranges(draws, meshes, world, weight)
        pipes = []
        try:
            for r, rng in enumerate(ranges):
                pipes.append(cls(meshes, meshlets, draws, depth_size, rank=r, world=len(ranges), draw_range=rng,
                                 share=pipes[0] if pipes else None, **kw))
        except Exception:
            for p in pipes:
                p.ctx.close()
            raise
        return LocalShards(pipes)

    def _local(self, cull_data):
        cd = cull_data.copy()
        cd["drawCount"] = self.draw_count
        return cd

    def cull(self, cull_data, late, task=True, post_pass=0):
        super().cull(self._local(cull_data), late, task, post_pass)

    def render_clusters(self, cull_data, late, post_pass=0):
        super().render_clusters(self._local(cull_data), late, post_pass)

    def render_depth(self, cull_data, late, post_pass=0, visibility=None, totals4=None, textures=False, **kw):
        if textures:
            raise NvError("render_depth(textures=True) is not available on a sharded pipeline")
        if visibility is not None and not self.stable_ids:
            raise NvError("a sharded frame has no visibility buffer: the slot index nv_rasterdepth writes is rank-local")
        super().render_depth(self._local(cull_data), late, post_pass, visibility, totals4)

    def _draw_triangle_offsets(self):
        return self._triangle_names("render_draws(visibility=)")[self.begin * 8:]  # (a byte tensor of u64) global values, rank-local drawIds: every rank writes the same words

    def render_draws(self, cull_data, late, post_pass=0, totals4=None, visibility=None):
        super().render_draws(self._local(cull_data), late, post_pass, totals4, visibility)

    PHASES = (("early", False, 0), ("late", True, 0), ("post", True, 1))

    def phase(self, cull_data, name, task=True, totals4=None, visibility=None):
        """one phase of frame() up to and including its raster; the composite is the caller's next step"""
        if visibility is not None and not self.stable_ids:
            raise NvError("a sharded frame has no visibility buffer: the slot index nv_rasterdepth writes is rank-local "
                          "(ShardedVisibilityPipeline(..., stable_ids=True) names clusters and triangles by a frame-stable id instead)")
        late, pp = {n: (l, p) for n, l, p in self.PHASES}[name]
        if not task:
            cull_data = cull_data.copy()
            cull_data["clusterOcclusionEnabled"] = 0
        if name == "late":
            self.build_pyramid(self.depth)
        self.cull(cull_data, late=late, task=task, post_pass=pp)
        if task:
            self.render_clusters(cull_data, late=late, post_pass=pp)
            self.render_depth(cull_data, late=late, post_pass=pp, totals4=totals4, visibility=visibility)
        else:
            self.render_draws(cull_data, late=late, post_pass=pp, totals4=totals4, visibility=visibility)

    def composite(self, visibility=None):
        """this rank's depth target (and stable-form visibility target) := the maximum over the ranks of the group (a no-op without a group)"""
        from . import shard
        shard.composite_depth(self.depth, self.group)
        if visibility is not None:
            shard.composite_visibility(visibility, self.group)

    def frame(self, cull_data, post_pass=False, on_phase=None, task=True, visibility=None, composite_last=True, on_raster=None, textures=False):
        """VisibilityPipeline.frame for this rank's draws, with the depth composite after each phase's raster.  on_raster(name) is called
        between a phase's raster and its composite (the rank's own depth), on_phase(name) after the composite.  composite_last=False skips
        the composite after the last phase: the rank's target then holds the earlier composites plus its own last raster"""
        if textures:
            raise NvError("frame(textures=True) is not available on a sharded pipeline")
        if visibility is not None and not self.stable_ids:
            raise NvError("a sharded frame has no visibility buffer: the slot index nv_rasterdepth writes is rank-local "
                          "(ShardedVisibilityPipeline(..., stable_ids=True) names clusters and triangles by a frame-stable id instead)")
        names = ["early", "late"] + (["post"] if post_pass else [])
        for name in names:
            self.phase(cull_data, name, task=task, visibility=visibility)
            if on_raster is not None:
                on_raster(name)
            if composite_last or name != names[-1]:
                # (the visibility target is only read after the frame: composited once, behind the last raster, would do as well; per
                # phase it stays the unsharded frame's at every on_phase, like the depth).  Without a target the call is composite(), as
                # before the argument existed: callers replace the method
                if visibility is None:
                    self.composite()
                else:
                    self.composite(visibility)
            if on_phase is not None:
                on_phase(name)

    def phase_counts(self, task=True):
        """int64 device tensor {visible draws or task commands, task groups, visible meshlets} of the last phase (shard.allreduce_counts
        sums it over the ranks)"""
        out = torch.zeros(3, dtype=torch.int64, device=self.ctx.device)
        self.ctx.pack_counts(self.dccb, None, self.ccb if task else None, out)
        if task:
            out[1] = (out[0] + 63) // 64
        return out


class LocalShards:
    """The shards of ShardedVisibilityPipeline.local_shards: frame() runs every shard's phase on the current stream, then composites their
    depth targets with nv_depth_merge (one launch folds all of them into the first shard's, which is then copied to the others), so that
    afterwards every shard holds the full target, as after the all-reduce of the one-rank-per-process deployment"""

    def __init__(self, pipes):
        self.pipes = pipes
        self.ranges = [(p.begin, p.end) for p in pipes]

    def composite(self, visibility=None):
        """visibility: one stable-form target per shard; folded with nv_visibility_merge like the depth targets"""
        first, rest = self.pipes[0], self.pipes[1:]
        if rest:
            first.ctx.depth_merge(first.depth, [p.depth for p in rest], first.depth_w, first.depth_h)
            for p in rest:
                p.depth.copy_(first.depth)
            if visibility is not None:
                first.ctx.visibility_merge(visibility[0], list(visibility[1:]), first.depth_w, first.depth_h)
                for v in visibility[1:]:
                    v.copy_(visibility[0])

    def new_visibility(self):
        return [p.new_visibility() for p in self.pipes]

    def frame(self, cull_data, post_pass=False, on_phase=None, task=True, composite_last=True, on_raster=None, visibility=None, textures=False):
        """visibility: a list with one u64 target per shard (new_visibility()); needs local_shards(..., stable_ids=True)"""
        if textures:
            raise NvError("frame(textures=True) is not available on a sharded pipeline")
        names = ["early", "late"] + (["post"] if post_pass else [])
        for name in names:
            for k, p in enumerate(self.pipes):
                p.phase(cull_data, name, task=task, visibility=None if visibility is None else visibility[k])
            if on_raster is not None:
                on_raster(name)
            if composite_last or name != names[-1]:
                if visibility is None:  # (composite() as before the argument existed: callers replace the method)
                    self.composite()
                else:
                    self.composite(visibility)
            if on_phase is not None:
                on_phase(name)

    def status(self):
        for p in self.pipes:
            p.ctx.status()

    def close(self):
        for p in self.pipes:
            p.ctx.close()
