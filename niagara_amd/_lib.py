"""ctypes binding of the C ABI in include/niagara_vis.h (niagara_amd/libniagara_vis.so).

The library is the product: there is no Python or CPU fallback.  If the shared object is missing this module raises
at import time, and every device entry point raises NvError on a non-zero status.
"""
import ctypes as C
import os

# The Python host layer hands torch-allocated device pointers and torch streams to the library, so both must sit on
# ONE HIP runtime.  torch bundles its own libamdhip64.so.7; loading it first makes the library's NEEDED entry resolve
# to that same copy (same SONAME).  A C++ host that does not use torch simply links /opt/rocm's runtime.
try:
    import torch  # noqa: F401
except ImportError:  # pragma: no cover - the C ABI itself does not need torch
    pass

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("NV_LIBRARY_PATH") or os.path.join(_HERE, "libniagara_vis.so")  # override: A/B builds during development


class NvError(RuntimeError):
    pass


class PyramidDesc(C.Structure):
    _fields_ = [("d_base", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("levels", C.c_uint32),
                ("mipOffset", C.c_uint32 * 16), ("totalTexels", C.c_uint32)]


class BloomDesc(C.Structure):
    """NvBloomDesc (include/niagara_vis.h): the bloom target's levels in one linear buffer of B10G11R11 words"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("levels", C.c_uint32), ("levelOffset", C.c_uint32 * 8), ("totalTexels", C.c_uint32)]


class RtSceneStats(C.Structure):
    """NvRtSceneStats (include/niagara_vis.h): what nv_rt_scene_stats reports of a scene blob"""
    _fields_ = [(n, C.c_uint32) for n in ("bytes", "instances", "tlasNodes", "tlasLeaves", "tlasMaxLeaf", "blasCount", "blasNodes", "blasLeaves",
                                          "blasMaxLeaf", "triangles")]


class SceneCacheInfo(C.Structure):
    """NvSceneCacheInfo (include/niagara_vis.h)"""
    _fields_ = ([(n, C.c_uint32) for n in ("version", "compressed", "clrtMode", "ommStates")] + [("hashMeta", C.c_uint64)] +
                [(n, C.c_uint32) for n in ("meshletMaxVertices", "meshletMaxTriangles", "vertexCount", "indexCount", "meshletCount",
                                           "meshletdataCount", "meshletvtx0Count", "meshCount", "materialCount", "drawCount",
                                           "texturePathCount", "lightCount", "animationCount", "keyframeCount")] +
                [("cameraPosition", C.c_float * 3), ("cameraOrientation", C.c_float * 4), ("cameraFovY", C.c_float),
                 ("cameraZnear", C.c_float), ("sunDirection", C.c_float * 3)] +
                [(n, C.c_uint64) for n in ("fileSize", "vertexOffset", "indexOffset", "meshletOffset", "meshletdataOffset", "meshOffset",
                                           "drawOffset", "vertexBytes", "indexBytes", "meshletdataBytes")])


class DdsInfo(C.Structure):
    """NvDdsInfo (include/niagara_vis.h): what nv_dds_parse reports of a DDS file image"""
    _fields_ = [(n, C.c_uint32) for n in ("format", "width", "height", "levels", "blockBytes", "payloadOffset")] + [
        ("payloadBytes", C.c_uint64), ("levelOffset", C.c_uint64 * 15)]


class TextureDesc(C.Structure):
    """NvTextureDesc (include/niagara_vis.h, layouts.TEXTUREDESC): one decoded texture of a set"""
    _fields_ = [(n, C.c_uint32) for n in ("offset", "width", "height", "levels")]


if not os.path.exists(SO_PATH):
    raise ImportError("niagara_amd: %s is missing — build it with `make -C niagara_amd/csrc` (or __graft_entry__.build()); "
                      "there is no fallback path" % SO_PATH)

lib = C.CDLL(SO_PATH)

# nv_profile_read: the NV_PROF_* slots of include/niagara_vis.h in their order (NV_PROF_SLOTS names); pipeline.Context.profile_read's keys
PROF_NAMES = ("cluster_cull", "cluster_scatter", "drawcull", "depthreduce", "cluster_hiz")
# nv_profile_variants: the NV_VARIANT_* slots of include/niagara_vis.h in their order (NV_VARIANT_SLOTS names); pipeline.Context.VARIANTS is this tuple
VARIANT_NAMES = ("cull_filter_ring4", "cull_filter_ring8", "cull_direct", "cull_lanes_bits", "cull_lanes", "cull_aos", "hiz_stage", "task_list", "task_per_draw", "cull_direct_packed")

_vp, _u32, _i, _f = C.c_void_p, C.c_uint32, C.c_int, C.c_float
_SIGS = {
    "nv_create": (_i, [C.POINTER(_vp), _i]),
    "nv_destroy": (None, [_vp]),
    "nv_version": (C.c_char_p, []),
    "nv_status": (_i, [_vp, _vp]),
    "nv_set_option": (_i, [_vp, _i, _i]),
    "nv_reserve": (_i, [_vp, _u32, _u32]),
    "nv_share_scene": (_i, [_vp, _vp]),
    "nv_profile_enable": (_i, [_vp, _i]),
    "nv_profile_read": (_i, [_vp, C.POINTER(C.c_float * len(PROF_NAMES)), C.POINTER(C.c_uint32 * len(PROF_NAMES))]),
    "nv_profile_variants": (_i, [_vp, C.POINTER(C.c_uint32 * len(VARIANT_NAMES))]),
    "nv_upload_meshlets": (_i, [_vp, _vp, _vp, _u32]),
    "nv_debug_block_table": (_i, [_vp, _vp, _u32, C.POINTER(_u32)]),
    "nv_upload_meshes": (_i, [_vp, _vp, _vp, _u32]),
    "nv_upload_draws": (_i, [_vp, _vp, _vp, _u32, _vp]),
    "nv_meshlet_bounds": (_i, [_vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "nv_update_draws": (_i, [_vp, _vp, _vp, _u32, _u32]),
    "nv_drawcull": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, C.POINTER(PyramidDesc)]),
    "nv_reset_count": (_i, [_vp, _vp, _vp, _vp]),
    "nv_tasksubmit": (_i, [_vp, _vp, _vp, _vp]),
    "nv_clustercull": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, C.POINTER(PyramidDesc), _vp, _vp]),
    "nv_clustersubmit": (_i, [_vp, _vp, _vp, _vp]),
    "nv_taskcull": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, C.POINTER(PyramidDesc), _vp, _vp]),
    "nv_cluster_expand": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "nv_trianglecull": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "nv_rasterdepth": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp]),
    "nv_rasterdepth_textured": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _u32, _vp, _u32, _vp, C.c_uint64, _vp]),
    "nv_rasterdepth_indexed": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _u32, _vp]),
    "nv_rasterdepth_indexed_visibility": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _u32, _vp, _vp, _vp]),
    "nv_visibility_resolve_indexed": (_i, [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _vp]),
    "nv_visibility_attributes_indexed": (_i, [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _vp]),
    "nv_rasterdepth_indexed_textured": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _u32, _vp, _u32,
                                             _vp, C.c_uint64, _vp]),
    "nv_rasterdepth_indexed_blocks": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _u32, _vp, _u32,
                                           _vp, C.c_uint64, _vp]),
    "nv_visibility_attributes_indexed_textured": (_i, [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _vp,
                                                       _vp, _u32, _vp, C.c_uint64]),
    "nv_visibility_attributes_indexed_blocks": (_i, [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _vp,
                                                     _vp, _u32, _vp, C.c_uint64]),
    "nv_assign_triangle_offsets": (_i, [_vp, _u32, _vp, _u32, _vp]),
    "nv_depthreduce": (_i, [_vp, _vp, _vp, _u32, _u32, C.POINTER(PyramidDesc)]),
    "nv_depth_merge": (_i, [_vp, _vp, _vp, C.POINTER(_vp), _u32, _u32, _u32]),
    "nv_visibility_merge": (_i, [_vp, _vp, _vp, C.POINTER(_vp), _u32, _u32, _u32]),
    "nv_visibility_resolve": (_i, [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _vp]),
    "nv_visibility_attributes": (_i, [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _vp]),
    "nv_visibility_attributes_textured": (_i, [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _vp,
                                               _vp, _u32, _vp, C.c_uint64]),
    "nv_dds_parse": (_i, [_vp, C.c_uint64, C.POINTER(DdsInfo)]),
    "nv_visibility_attributes_blocks": (_i, [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _vp,
                                             _vp, _u32, _vp, C.c_uint64]),
    "nv_rasterdepth_blocks": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _u32, _vp, _u32, _vp, C.c_uint64, _vp]),
    "nv_shadow_trace_blocks": (_i, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _i, _vp, _u32, _vp, _u32, _vp, _u32, _vp, C.c_uint64]),
    "nv_texture_block_layout": (_i, [C.POINTER(DdsInfo), _u32, _vp, C.POINTER(C.c_uint64)]),
    "nv_texture_block_fetch_host": (_i, [_vp, _vp, C.c_uint64, _u32, _u32, _u32, _vp]),
    "nv_texture_block_sample_host": (_i, [_vp, _u32, _vp, C.c_uint64, _u32, _vp, _vp, _vp, _vp]),
    "nv_texture_block_decode_host": (_i, [_u32, C.c_uint64, C.c_uint64, _vp, _vp]),
    "nv_texture_set_layout": (_i, [C.POINTER(DdsInfo), _u32, _vp, C.POINTER(C.c_uint64)]),
    "nv_texture_decode_host": (_i, [C.POINTER(DdsInfo), _vp, _vp, _vp, C.c_uint64]),
    "nv_texture_decode": (_i, [_vp, _vp, _vp, _u32, _u32, _u32, _u32, _vp, C.POINTER(TextureDesc)]),
    "nv_texture_sample_host": (_i, [_vp, _u32, _vp, C.c_uint64, _u32, _vp, _vp, _vp, _vp]),
    "nv_scenecache_texture_paths": (_i, [C.c_char_p, C.POINTER(SceneCacheInfo), _vp]),
    "nv_shadow_fill": (_i, [_vp, _vp, _vp, _vp, _u32, _u32, _i]),
    "nv_shadow_blur": (_i, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _i, _f]),
    "nv_shade_final": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32]),
    "nv_build_shade_data": (_i, [_vp, _vp, _vp, _vp, _i, _u32, _u32]),
    "nv_build_shadow_data": (_i, [_vp, _vp, _vp, _f, _i, _u32, _u32]),
    "nv_rt_scene_build": (_i, [_vp, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp, C.POINTER(C.c_uint64)]),
    "nv_rt_scene_build_textured": (_i, [_vp, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp, C.POINTER(C.c_uint64)]),
    "nv_rt_scene_trace_host_textured_rays": (_i, [_vp, _vp, _vp, C.c_uint64, _f, _f, _i, _vp, _u32, _vp, _u32, _vp, _u32, _vp, C.c_uint64, _vp]),
    "nv_rt_alpha_sample_host": (_i, [_vp, _vp, C.c_uint64, _vp, C.c_uint64, _vp, _vp]),
    "nv_shadow_trace_textured": (_i, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _i, _vp, _u32, _vp, _u32, _vp, _u32, _vp, C.c_uint64]),
    "nv_rt_scene_validate": (_i, [_vp, C.c_uint64]),
    "nv_rt_scene_stats": (_i, [_vp, C.c_uint64, C.POINTER(RtSceneStats)]),
    "nv_rt_scene_trace_host": (_i, [_vp, _vp, _vp, _f, _f, _i]),
    "nv_rt_scene_trace_host_rays": (_i, [_vp, _vp, _vp, C.c_uint64, _f, _f, _i, _vp]),
    "nv_rt_scene_upload": (_i, [_vp, _vp, _vp, C.c_uint64]),
    "nv_shadow_trace": (_i, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _i]),
    "nv_rt_tlas_build_host": (_i, [_vp, C.c_uint64, _vp, _u32, _vp, C.POINTER(C.c_uint64)]),
    "nv_rt_scene_reserve_dynamic": (_i, [_vp, _vp, _u32]),
    "nv_rt_tlas_build": (_i, [_vp, _vp, _vp, _u32]),
    "nv_rt_scene_download": (_i, [_vp, _vp, _vp, C.POINTER(C.c_uint64)]),
    "nv_bloom_desc_init": (_i, [C.POINTER(BloomDesc), _u32, _u32]),
    "nv_bloom_extract": (_i, [_vp, _vp, _vp, _u32, _u32, _vp, C.POINTER(BloomDesc)]),
    "nv_bloom_downsample": (_i, [_vp, _vp, _vp, C.POINTER(BloomDesc), _u32]),
    "nv_bloom_upsample": (_i, [_vp, _vp, _vp, C.POINTER(BloomDesc), _u32, _f]),
    "nv_bloom": (_i, [_vp, _vp, _vp, _u32, _u32, _vp, C.POINTER(BloomDesc)]),
    "nv_shade_final_bloom": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, C.POINTER(BloomDesc)]),
    "nv_previous_pow2": (_u32, [_u32]),
    "nv_division_magic": (_u32, [_u32]),
    "nv_image_mip_levels": (_u32, [_u32, _u32]),
    "nv_pyramid_desc_init": (_i, [C.POINTER(PyramidDesc), _u32, _u32]),
    "nv_build_cull_data": (_i, [_vp, _vp, _vp, _f, _f, _f, _u32, _u32, _u32, _u32, _u32, _i]),
    "nv_assign_visibility_offsets": (_i, [_vp, _u32, _vp, _u32, C.POINTER(_u32), C.POINTER(_u32)]),
    "nv_synth_draws": (_i, [_vp, _u32, _u32, _f]),
    "nv_mesh_bounds": (_i, [_vp, _u32, _vp, _vp]),
    "nv_shard_range": (None, [C.c_uint64, _u32, _u32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "nv_pack_counts": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "nv_set_counts_sink": (_i, [_vp, _vp]),
    "nv_scenecache_info": (_i, [C.c_char_p, C.POINTER(SceneCacheInfo)]),
    "nv_scenecache_read": (_i, [C.c_char_p, C.POINTER(SceneCacheInfo), _vp, _vp, _vp]),
    "nv_scenecache_animations": (_i, [C.c_char_p, C.POINTER(SceneCacheInfo), _vp, _vp, _vp]),
    "nv_animation_validate_host": (_i, [_vp, _u32, _u32, _u32, _u32, C.POINTER(_u32), C.POINTER(_u32)]),
    "nv_animation_phase_host": (_i, [_vp, _vp, _vp, C.c_uint64, _vp, _vp, _vp, _vp]),
    "nv_animate_draws_host": (_i, [C.c_double, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _u32]),
    "nv_upload_animations": (_i, [_vp, _vp, _vp, _u32, _vp, _u32, _u32, _u32]),
    "nv_animate_draws": (_i, [_vp, _vp, C.c_double, _vp, _u32, _vp, _u32]),
    "nv_probe_cluster_scalars": (_i, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, C.POINTER(PyramidDesc), _vp]),
}
EXPORTS = sorted(_SIGS)
for _name, (_res, _args) in _SIGS.items():
    _fn = getattr(lib, _name)  # AttributeError here = header/library mismatch, fail loudly
    _fn.restype = _res
    _fn.argtypes = _args


def check(rc, what):
    if rc != 0:
        names = {-1: "NV_EINVAL", -2: "NV_ENOMEM", -3: "NV_ESTATE", -4: "NV_ENODEV", -5: "NV_EIO", -6: "NV_EFORMAT", -7: "NV_ETEXFORMAT"}
        raise NvError("%s failed: %s" % (what, names.get(rc, "hipError %d" % rc)))
