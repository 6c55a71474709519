"""Byte layouts of the buffers crossing the boundary, as numpy structured dtypes.

Same bytes as the reference structs (src/scene.h:10-93, src/niagara.cpp:227-260, src/shaders/mesh.h:11-123) and
as include/niagara_vis.h; tests cross-check all three.
"""
import numpy as np

MESHLET = np.dtype([("center", "<u2", 3), ("radius", "<u2"), ("cone_axis", "i1", 3), ("cone_cutoff", "i1"),
                    ("dataOffset", "<u4"), ("baseVertex", "<u4"), ("vertexCount", "u1"), ("triangleCount", "u1"),
                    ("shortRefs", "u1"), ("padding", "u1")])
MESHDRAW = np.dtype([("position", "<f4", 3), ("scale", "<f4"), ("orientation", "<f4", 4), ("meshIndex", "<u4"),
                     ("meshletVisibilityOffset", "<u4"), ("postPass", "<u4"), ("materialIndex", "<u4")])
# src/scene.h:51-58, 119-136: the animation path (nv_upload_animations / nv_animate_draws); rotation is (x, y, z, w) like MESHDRAW.orientation
LIGHT = np.dtype([("position", "<f4", 3), ("range", "<f4"), ("color", "<f4", 3), ("intensity", "<f4")])
KEYFRAME = np.dtype([("translation", "<f4", 3), ("scale", "<f4"), ("rotation", "<f4", 4)])
ANIMATION = np.dtype([("drawIndex", "<i4"), ("lightIndex", "<i4"), ("startTime", "<f4"), ("period", "<f4"), ("keyframeOffset", "<u4"),
                      ("keyframeCount", "<u4")])
MESHLOD = np.dtype([("indexOffset", "<u4"), ("indexCount", "<u4"), ("meshletOffset", "<u4"), ("meshletCount", "<u4"),
                    ("error", "<f4")])
MESH = np.dtype([("center", "<f4", 3), ("radius", "<f4"), ("vertexOffset", "<u4"), ("vertexCount", "<u4"),
                 ("ommIndexData", "<u4"), ("ommIndexBase", "<u4"), ("lodCount", "<u4"), ("lodRT", "<u4"),
                 ("padding", "<u4", 2), ("lods", MESHLOD, 8)])
DRAWCMD = np.dtype([("drawId", "<u4"), ("indexCount", "<u4"), ("instanceCount", "<u4"), ("firstIndex", "<u4"),
                    ("vertexOffset", "<u4"), ("firstInstance", "<u4")])
TASKCMD = np.dtype([("drawId", "<u4"), ("taskOffset", "<u4"), ("taskCount", "<u4"), ("lateDrawVisibility", "<u4"),
                    ("meshletVisibilityOffset", "<u4")])
CULLDATA = np.dtype([("view", "<f4", 16), ("P00", "<f4"), ("P11", "<f4"), ("znear", "<f4"), ("zfar", "<f4"),
                     ("frustum", "<f4", 4), ("lodTarget", "<f4"), ("pyramidWidth", "<f4"), ("pyramidHeight", "<f4"),
                     ("drawCount", "<u4"), ("cullingEnabled", "<i4"), ("lodEnabled", "<i4"), ("occlusionEnabled", "<i4"),
                     ("clusterOcclusionEnabled", "<i4"), ("clusterBackfaceEnabled", "<i4"), ("postPass", "<u4"),
                     ("_pad", "<u4", 2)])

CLUSTERRECORD = np.dtype([("drawId", "<u4"), ("meshletIndex", "<u4"), ("vertexCount", "<u4"), ("triangleCount", "<u4"), ("vertexOffset", "<u4"),
                          ("indexOffset", "<u4"), ("baseVertex", "<u4"), ("shortRefs", "<u4")])
VERTEX = np.dtype([("vx", "<u2"), ("vy", "<u2"), ("vz", "<u2"), ("tp", "<u2"), ("np", "<u4"), ("tu", "<u2"), ("tv", "<u2")])  # src/shaders/mesh.h:3-9
GLOBALS = np.dtype([("projection", "<f4", 16), ("cullData", CULLDATA), ("screenWidth", "<f4"), ("screenHeight", "<f4"), ("_pad", "<f4", 2)])  # mesh.h:46-51
TRIMASK = np.dtype([("keep", "<u4", 3), ("counts", "<u4")])
assert (VERTEX.itemsize, GLOBALS.itemsize, TRIMASK.itemsize) == (16, 224, 16)
# NvVisRecord: one pixel of nv_visibility_resolve (no sample: drawId = 0xFFFFFFFF, the rest 0; unresolved: all ones)
VISRECORD = np.dtype([("drawId", "<u4"), ("meshletIndex", "<u4"), ("triangle", "<u4"), ("depthBits", "<u4")])
assert VISRECORD.itemsize == 16
# NvVisIndexedRecord: one pixel of nv_visibility_resolve_indexed (no sample: drawId = 0xFFFFFFFF, the rest 0; unresolved: all ones)
VISINDEXEDRECORD = np.dtype([("drawId", "<u4"), ("indexPosition", "<u4"), ("vertexOffset", "<u4"), ("depthBits", "<u4")])
assert VISINDEXEDRECORD.itemsize == 16
# NvMaterial (src/scene.h:25-37, src/shaders/mesh.h:80-90) and NvPixelAttributes, one pixel of nv_visibility_attributes (no sample and invalid
# records: all zero except drawId = 0xFFFFFFFF)
MATERIAL = np.dtype([("albedoTexture", "<u4"), ("normalTexture", "<u4"), ("specularTexture", "<u4"), ("emissiveTexture", "<u4"),
                     ("diffuseFactor", "<f4", 4), ("specularFactor", "<f4", 4), ("emissiveFactor", "<f4", 3), ("padding", "<u4")])
PIXELATTR = np.dtype([("uv", "<f4", 2), ("bary", "<f4", 2), ("normal", "<f4", 3), ("drawId", "<u4"), ("tangent", "<f4", 4), ("wpos", "<f4", 3),
                      ("materialIndex", "<u4")])
assert (MATERIAL.itemsize, PIXELATTR.itemsize) == (64, 64)
# NvShadeData (src/niagara.cpp:280-290), the push constants of final.comp.glsl: 104 bytes used, alignas(16) pads to 112
SHADEDATA = np.dtype([("cameraPosition", "<f4", 3), ("pad0", "<f4"), ("sunDirection", "<f4", 3), ("shadowsEnabled", "<i4"),
                      ("inverseViewProjection", "<f4", 16), ("imageSize", "<f4", 2), ("_pad", "<f4", 2)])
assert SHADEDATA.itemsize == 112
# NvShadowData (src/niagara.cpp:269-278), the push constants of shadow.comp.glsl: 92 bytes used, alignas(16) pads to 96
SHADOWDATA = np.dtype([("sunDirection", "<f4", 3), ("sunJitter", "<f4"), ("inverseViewProjection", "<f4", 16), ("imageSize", "<f4", 2),
                       ("checkerboard", "<i4"), ("_pad", "<u4")])
assert SHADOWDATA.itemsize == 96
# NvBloomDesc (src/niagara.cpp:1331-1333): level 0 size, level count and the levels' offsets (texels) in the one B10G11R11 buffer
BLOOMDESC = np.dtype([("width", "<u4"), ("height", "<u4"), ("levels", "<u4"), ("levelOffset", "<u4", 8), ("totalTexels", "<u4")])
assert BLOOMDESC.itemsize == 48
BLOOM_MAX_LEVELS = 8
# NvTextureDesc: one decoded texture of a set — the word offset of level 0 in the set's RGBA8 texel buffer, level 0's size, the level count
# (the levels follow one another, each row-major without padding).  Entry 0 of a table is the reserved "no texture" entry
TEXTUREDESC = np.dtype([("offset", "<u4"), ("width", "<u4"), ("height", "<u4"), ("levels", "<u4")])
assert TEXTUREDESC.itemsize == 16
TEXTURE_MAX_LEVELS = 15
# NvTextureBlockDesc: one block-resident texture of a set — the offset of its DDS payload in the set's block buffer in 16-byte
# units, level 0's size, and the level count (bits 0-7) with the format (layouts.FORMAT_*, bits 8-15).  Entry 0 is the reserved entry
TEXTUREBLOCKDESC = np.dtype([("offset", "<u4"), ("width", "<u4"), ("height", "<u4"), ("levelsFormat", "<u4")])
assert TEXTUREBLOCKDESC.itemsize == 16
FORMAT_BC1, FORMAT_BC2, FORMAT_BC3, FORMAT_BC4, FORMAT_BC5, FORMAT_BC6H, FORMAT_BC7 = 1, 2, 3, 4, 5, 6, 7
VIS_ID_BITS = 34  # the stable form of the visibility word: bits(z) << 34 | ((mvi << 7 | triangle) + 1)

TASK_WGSIZE = 64
TASK_WGLIMIT = 1 << 22
CLUSTER_LIMIT = 1 << 24
CLUSTER_TILE = 16

assert (MESHLET.itemsize, MESHDRAW.itemsize, MESHLOD.itemsize, MESH.itemsize) == (24, 48, 20, 208)
assert (DRAWCMD.itemsize, TASKCMD.itemsize, CULLDATA.itemsize) == (24, 20, 144)
