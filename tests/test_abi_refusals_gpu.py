"""What the C ABI refuses before its first launch (include/niagara_vis.h, niagara_amd/csrc/context.hip), one row per condition.

A row starts from a complete, valid argument tuple of one nv_* entry point over tiny real device buffers (an 8 x 4 image, 4 draws, 2 meshlets,
1 material, a 4 x 4 BC1 texture; every buffer 64 bytes longer than it has to be, so that a pointer moved by 1 .. 8 bytes stays inside it), changes
exactly one argument and names the status the call returns.  Every row is a condition the entry point tests before it enqueues anything, so no
kernel runs in this file; a row the library did NOT refuse would launch on a bad argument, so the first wrong status ends the file: no further
call is issued.  NV_LIBRARY_PATH selects the build, the table is the same for every build."""
import ctypes as C

import numpy as np
import pytest
import torch

import shadow_alpha_ref as SA
import texture_ref as TR
from niagara_amd import host, synth
from niagara_amd import layouts as L
from niagara_amd._lib import BloomDesc, PyramidDesc, TextureDesc, lib

OK, EINVAL, ENOMEM, ETEXFORMAT = 0, -1, -2, -7
W, H = 8, 4
N = W * H
SLACK = 64
DRAWS, MESHLETS, MATERIALS, MESHES, VERTICES, DATA_WORDS = 4, 2, 1, 1, 4, 16
RESERVED_DRAWS = 1 << 20  # what nv_create reserves (context.hip reserve_raster_scratch)

_stopped = []  # the label of the first row whose status was wrong


def run(rows):
    """calls the rows in order; the first wrong status fails the test and keeps every later row of the file from being called"""
    for label, fn, base, index, value, want in rows:
        if _stopped:
            pytest.fail("no further call after the row %r returned a wrong status" % _stopped[0])
        args = list(base)
        args[index] = value
        rc = getattr(lib, fn)(*args)
        if rc != want:
            _stopped.append("%s: %s" % (fn, label))
            pytest.fail("%s, %s: status %d, expected %d" % (fn, label, rc, want))


class Env:
    def __init__(self):
        from niagara_amd import pipeline as P
        self.P = P
        self.ctx = P.Context()
        self.h = self.ctx.h
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.keep = []
        cd = host.build_cull_data(viewport=(W, H), draw_count=DRAWS)
        self.cull = self.host(cd)
        self.globals = self.host(synth.make_globals(cd, (W, H)))
        self.globals_w = self.host(synth.make_globals(cd, (W + 1, H)))
        self.globals_h = self.host(synth.make_globals(cd, (W, H + 1)))
        g = synth.make_globals(cd, (W, H))
        self.shade = self.host(host.build_shade_data(g, shadows_enabled=1))
        self.shade_w = self.host(host.build_shade_data(g, shadows_enabled=1, width=W + 1))
        self.shade_h = self.host(host.build_shade_data(g, shadows_enabled=1, height=H + 1))
        self.shadow_data = self.host(host.build_shadow_data(g))
        self.shadow_data_w = self.host(host.build_shadow_data(g, width=W + 1))
        self.shadow_data_h = self.host(host.build_shadow_data(g, height=H + 1))

    def host(self, array):
        """a host struct the library reads during the call"""
        a = np.ascontiguousarray(array)
        self.keep.append(a)
        return C.c_void_p(a.ctypes.data)

    def dev(self, nbytes):
        """a zeroed device buffer of nbytes + SLACK bytes (torch aligns it to 512 bytes)"""
        t = torch.zeros(nbytes + SLACK, dtype=torch.uint8, device=self.ctx.device)
        assert t.data_ptr() % 256 == 0
        self.keep.append(t)
        return t.data_ptr()

    def upload(self, array):
        t = self.P.to_device(array, self.ctx.device)
        t = torch.cat([t, torch.zeros(SLACK, dtype=torch.uint8, device=self.ctx.device)])
        assert t.data_ptr() % 256 == 0
        self.keep.append(t)
        return t.data_ptr()

    def block_set(self):
        """the block-resident set of the file's 4 x 4 BC1 texture (Context.texture_blocks): table address, entries, buffer address, units16"""
        descs, blocks = self.ctx.texture_blocks([TR.dds_header(1, 4, 4, 1) + bytes(8)])
        units16 = int(blocks.numel()) // 16
        blocks = torch.cat([blocks, torch.zeros(SLACK, dtype=torch.uint8, device=self.ctx.device)])
        assert blocks.data_ptr() % 256 == 0 and (len(descs), units16) == (2, 1)
        self.keep.append(blocks)
        return self.upload(descs), len(descs), blocks.data_ptr(), units16


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.ctx.close()


def p(address, offset=0):
    return C.c_void_p(address + offset)


def null(fn, base, names):
    return [("%s NULL" % n, fn, base, i, None, EINVAL) for n, i in names.items()]


def misaligned(fn, base, name, index, mask):
    """one byte off, and the largest power of two that still violates the mask"""
    at = base[index].value
    return [("%s + %d" % (name, o), fn, base, index, p(at, o), EINVAL) for o in (1, (mask + 1) // 2)]


def sizes(fn, base, iw, ih):
    return [("width 0", fn, base, iw, 0, EINVAL), ("height 0", fn, base, ih, 0, EINVAL), ("width 16385", fn, base, iw, 16385, EINVAL),
            ("height 16385", fn, base, ih, 16385, EINVAL)]


# ---------------------------------------------------------------------------------------------------------------- options

@pytest.mark.gpu
def test_set_option(env):
    P = env.P
    table = {
        P.NV_OPT_FUSED_COUNT_RESET: ([-1, 2, 1, 0], []),  # any value: non-zero is on
        P.NV_OPT_FUSED_SUBMIT: ([-1, 2, 1, 0], []),
        P.NV_OPT_CULL_WORKGROUPS_PER_CU: ([1, 2, 3, 4, 5, 7, 8, 6], [0, 9, -1]),
        P.NV_OPT_SCATTER_WAVES: ([4, 8, 16], [3, 5, 7, 9, 15, 17, 0]),
        P.NV_OPT_CULL_FORM: ([1, 2, 3, 4, 5, 0], [-1, 6]),
        P.NV_OPT_CULL_RING: ([4, 8, 0], [-1, 1, 3, 5, 7, 9]),
        P.NV_OPT_TASK_EMIT: ([1, 2, 0], [-1, 3]),
        P.NV_OPT_DRAW_RECORDS: ([1, 2, 0], [-1, 3]),
        P.NV_OPT_RASTER_SMALL_LIMIT: ([0, 1, 2 ** 31 - 1, 16], [-1, -2 ** 31]),
        P.NV_OPT_RASTER_NEAR_CLIP: ([1, 0], [-1, 2]),
        P.NV_OPT_RASTER_VISIBILITY_ID: ([1, 0], [-1, 2]),
        P.NV_OPT_BLOOM_FUSED_TAIL: ([1, 0], [-1, 2]),
    }
    assert sorted(table) == list(range(1, 13))
    base = [env.h, 0, 0]
    rows = [("NULL context", "nv_set_option", [env.h, P.NV_OPT_CULL_FORM, 0], 0, None, EINVAL), ("option 0", "nv_set_option", base, 1, 0, EINVAL),
            ("option 13", "nv_set_option", base, 1, 13, EINVAL), ("option -1", "nv_set_option", base, 1, -1, EINVAL)]
    for option, (accepted, refused) in table.items():
        base = [env.h, option, accepted[-1]]
        rows += [("option %d value %d" % (option, v), "nv_set_option", base, 2, v, EINVAL) for v in refused]
        rows += [("option %d value %d" % (option, v), "nv_set_option", base, 2, v, OK) for v in accepted]  # (the default last)
    run(rows)


# ---------------------------------------------------------------------------------------------------------------- geometry passes

@pytest.mark.gpu
def test_cull_and_submit_passes(env):
    e = env
    cmds, count4, draws, meshes, dvb = e.dev(64 * L.TASKCMD.itemsize), e.dev(16), e.dev(DRAWS * L.MESHDRAW.itemsize), e.dev(MESHES * L.MESH.itemsize), e.dev(16)
    meshlets, mvb, cib, ccb, totals = e.dev(MESHLETS * L.MESHLET.itemsize), e.dev(16), e.dev(4 * 256), e.dev(16), e.dev(32)
    data, vertices, masks, records = e.dev(DATA_WORDS * 4), e.dev(VERTICES * L.VERTEX.itemsize), e.dev(256 * L.TRIMASK.itemsize), e.dev(256 * L.CLUSTERRECORD.itemsize)
    rows = []
    fn, base = "nv_drawcull", [e.h, e.stream, e.cull, 0, 1, p(draws), p(meshes), p(cmds), p(count4), p(dvb), None]
    rows += null(fn, base, dict(context=0, cull=2, draws=5, meshes=6, commands=7, count4=8, drawVisibility=9))
    for fn, last in (("nv_clustercull", dict(clusterIndices=10, clusterCount4=11)), ("nv_taskcull", dict(payloads=10, payloadCounts=11))):
        base = [e.h, e.stream, e.cull, 0, p(cmds), p(count4), p(draws), p(meshlets), p(mvb), None, p(cib), p(ccb)]
        rows += null(fn, base, dict(context=0, cull=2, commands=4, count4=5, draws=6, meshlets=7, **last))
    rows += null("nv_tasksubmit", [e.h, e.stream, p(count4), p(cmds)], dict(context=0, count4=2, commands=3))
    rows += null("nv_clustersubmit", [e.h, e.stream, p(ccb), p(cib)], dict(context=0, clusterCount4=2, clusterIndices=3))
    rows += null("nv_pack_counts", [e.h, e.stream, p(count4), p(ccb), None, p(totals)], dict(context=0, out3=5))
    fn, base = "nv_cluster_expand", [e.h, e.stream, p(cmds), p(meshlets), p(cib), p(ccb), p(records), 256, p(totals)]
    rows += null(fn, base, dict(context=0, commands=2, meshlets=3, clusterIndices=4, clusterCount4=5, records=6, totals3=8))
    fn, base = "nv_trianglecull", [e.h, e.stream, e.globals, p(cmds), p(draws), p(meshlets), p(data), p(vertices), p(cib), p(ccb), p(masks), 256, p(totals)]
    rows += null(fn, base, dict(context=0, globals=2, commands=3, draws=4, meshlets=5, meshletData=6, vertices=7, clusterIndices=8, clusterCount4=9,
                                masks=10, totals3=12))
    fn, base = "nv_meshlet_bounds", [e.h, e.stream, p(vertices), p(data), p(meshlets), MESHLETS, None]
    rows += null(fn, base, dict(context=0, vertices=2, meshletData=3, meshlets=4))
    run(rows)


@pytest.mark.gpu
def test_depth_passes(env):
    e = env
    cmds, draws, meshlets, data = e.dev(64 * L.TASKCMD.itemsize), e.dev(DRAWS * L.MESHDRAW.itemsize), e.dev(MESHLETS * L.MESHLET.itemsize), e.dev(DATA_WORDS * 4)
    vertices, cib, ccb, depth, vis, totals = e.dev(VERTICES * L.VERTEX.itemsize), e.dev(4 * 256), e.dev(16), e.dev(N * 4), e.dev(N * 8), e.dev(32)
    dcmds, count, indices = e.dev(DRAWS * L.DRAWCMD.itemsize), e.dev(16), e.dev(12 * 4)
    rows = []
    fn = "nv_rasterdepth"
    base = [e.h, e.stream, e.globals, p(cmds), p(draws), p(meshlets), p(data), p(vertices), p(cib), p(ccb), p(depth), W, H, p(vis), p(totals)]
    rows += null(fn, base, dict(context=0, globals=2, commands=3, draws=4, meshlets=5, meshletData=6, vertices=7, clusterIndices=8, clusterCount4=9, depth=10))
    rows += sizes(fn, base, 11, 12)
    rows += [("screenWidth != width", fn, base, 2, e.globals_w, EINVAL), ("screenHeight != height", fn, base, 2, e.globals_h, EINVAL)]

    # the alpha-tested pair: nv_rasterdepth's arguments, then the material table, the texture set and the alpha totals
    materials, alpha = e.dev(MATERIALS * L.MATERIAL.itemsize), e.dev(16)
    bdescs, bcount, blocks, units16 = e.block_set()
    sets = (("nv_rasterdepth_textured", "texels", 3, [p(e.dev(2 * L.TEXTUREDESC.itemsize)), 2, p(e.dev(16 * 4)), 16]),
            ("nv_rasterdepth_blocks", "blocks", 15, [p(bdescs), bcount, p(blocks), units16]))
    for fn, buffer, mask, tset in sets:
        base = [e.h, e.stream, e.globals, p(cmds), p(draws), p(meshlets), p(data), p(vertices), p(cib), p(ccb), p(depth), W, H, p(vis), p(totals),
                p(materials), MATERIALS] + tset + [p(alpha)]
        rows += null(fn, base, dict(context=0, globals=2, commands=3, draws=4, meshlets=5, meshletData=6, vertices=7, clusterIndices=8, clusterCount4=9,
                                    depth=10))
        rows += sizes(fn, base, 11, 12)
        rows += [("screenWidth != width", fn, base, 2, e.globals_w, EINVAL), ("screenHeight != height", fn, base, 2, e.globals_h, EINVAL)]
        masks = dict(commands=(3, 3), clusterIndices=(8, 3), clusterCount4=(9, 3), depth=(10, 3), meshlets=(5, 3), meshletData=(6, 3), visibility=(13, 7),
                     totals4=(14, 7), alphaTotals2=(21, 7), draws=(4, 15), vertices=(7, 15), materials=(15, 15), textures=(17, 15))
        masks[buffer] = (19, mask)
        for name, (index, m) in masks.items():
            rows += misaligned(fn, base, name, index, m)
        # the table and its buffer come together or not at all; a count needs the table; a material table has entries
        rows += [("textures NULL with %s" % buffer, fn, base, 17, None, EINVAL), ("%s NULL with textures" % buffer, fn, base, 19, None, EINVAL),
                 ("materials with materialCount 0", fn, base, 16, 0, EINVAL)]
        without = base[:17] + [None, 0, None, 0] + base[21:]
        rows += [("textureCount without a table", fn, without, 18, 2, EINVAL)]

    fn = "nv_rasterdepth_indexed"
    base = [e.h, e.stream, e.globals, p(dcmds), p(count), p(draws), DRAWS, p(indices), 12, p(vertices), VERTICES, p(depth), W, H, p(totals)]
    rows += null(fn, base, dict(context=0, globals=2, commands=3, count=4, draws=5, indices=7, vertices=9, depth=11))
    rows += sizes(fn, base, 12, 13)
    rows += [("screenWidth != width", fn, base, 2, e.globals_w, EINVAL), ("screenHeight != height", fn, base, 2, e.globals_h, EINVAL),
             ("drawCount above the reservation", fn, base, 6, RESERVED_DRAWS + 1, ENOMEM), ("drawCount 2^32 - 1", fn, base, 6, 2 ** 32 - 1, ENOMEM)]

    pyr = host.pyramid_desc(W, H)
    pyr.d_base = e.dev(pyr.totalTexels * 4)
    e.keep.append(pyr)
    fn, base = "nv_depthreduce", [e.h, e.stream, p(depth), W, H, C.byref(pyr)]
    rows += null(fn, base, dict(context=0, depth=2, pyramid=5)) + [("width 0", fn, base, 3, 0, EINVAL), ("height 0", fn, base, 4, 0, EINVAL)]
    for label, field, value in (("pyramid without a base", "d_base", None), ("pyramid of 0 levels", "levels", 0), ("pyramid of 17 levels", "levels", 17)):
        bad = PyramidDesc.from_buffer_copy(pyr)
        setattr(bad, field, value)
        e.keep.append(bad)
        rows.append((label, fn, base, 5, C.byref(bad), EINVAL))

    for fn, words, mask in (("nv_depth_merge", depth, 3), ("nv_visibility_merge", vis, 7)):
        src = e.dev(N * 8)

        def srcs(*addresses):
            a = (C.c_void_p * len(addresses))(*addresses)
            e.keep.append(a)
            return a
        base = [e.h, e.stream, p(words), srcs(src), 1, W, H]
        rows += null(fn, base, dict(context=0, dst=2, sources=3)) + sizes(fn, base, 5, 6) + misaligned(fn, base, "dst", 2, mask)
        rows += [("zero sources", fn, base, 4, 0, EINVAL), ("a NULL source", fn, base, 3, srcs(None), EINVAL),
                 ("a source that is the destination", fn, base, 3, srcs(words), EINVAL),
                 ("the second source is the destination", fn, [e.h, e.stream, p(words), srcs(src, src), 2, W, H], 3, srcs(src, words), EINVAL)]
        rows += [("source + %d" % o, fn, base, 3, srcs(src + o), EINVAL) for o in (1, (mask + 1) // 2)]
    run(rows)


# ---------------------------------------------------------------------------------------------------------------- visibility buffer

ATTR_NAMES = dict(globals=2, records=3)
ATTR_COUNTED = dict(draws=6, meshlets=8, meshletData=10, vertices=12)  # refused as NULL because their count is not 0
ATTR_MASKS = dict(records=(3, 15), attributes=(16, 15), draws=(6, 15), vertices=(12, 15), materials=(14, 15), totals4=(19, 7), meshlets=(8, 3),
                  meshletData=(10, 3), gbuffer0=(17, 3), gbuffer1=(18, 3))


@pytest.mark.gpu
def test_visibility_passes(env):
    e = env
    vis, draws, meshes, records, seen, pixels, totals = (e.dev(N * 8), e.dev(DRAWS * L.MESHDRAW.itemsize), e.dev(MESHES * L.MESH.itemsize),
                                                        e.dev(N * L.VISRECORD.itemsize), e.dev(16), e.dev(DRAWS * 4), e.dev(32))
    meshlets, data, vertices, materials = e.dev(MESHLETS * L.MESHLET.itemsize), e.dev(DATA_WORDS * 4), e.dev(VERTICES * L.VERTEX.itemsize), e.dev(MATERIALS * L.MATERIAL.itemsize)
    attributes, gb0, gb1 = e.dev(N * L.PIXELATTR.itemsize), e.dev(N * 4), e.dev(N * 4)
    descs, texels = e.dev(2 * L.TEXTUREDESC.itemsize), e.dev(16 * 4)
    rows = []
    fn = "nv_visibility_resolve"
    base = [e.h, e.stream, e.cull, p(vis), W, H, p(draws), DRAWS, p(meshes), MESHES, p(records), p(seen), p(pixels), p(totals)]
    rows += null(fn, base, dict(context=0, cull=2, visibility=3, draws=6, meshes=8)) + sizes(fn, base, 4, 5)
    rows += misaligned(fn, base, "visibility", 3, 7) + misaligned(fn, base, "records", 10, 15) + misaligned(fn, base, "totals4", 13, 7)

    def attribute_args(materials_, material_count, g0, g1):
        return [e.h, e.stream, e.globals, p(records), W, H, p(draws), DRAWS, p(meshlets), MESHLETS, p(data), DATA_WORDS, p(vertices), VERTICES,
                materials_, material_count, p(attributes), g0, g1, p(totals)]

    fn, base = "nv_visibility_attributes", attribute_args(p(materials), MATERIALS, p(gb0), p(gb1))
    tex = [p(descs), 2, p(texels), 16]
    bdescs, bcount, blocks, units16 = e.block_set()
    btex = [p(bdescs), bcount, p(blocks), units16]
    for fn, base in (("nv_visibility_attributes", base), ("nv_visibility_attributes_textured", base + tex), ("nv_visibility_attributes_blocks", base + btex)):
        rows += null(fn, base, dict(context=0, **ATTR_NAMES, **ATTR_COUNTED, materials=14)) + sizes(fn, base, 4, 5)
        rows += [("screenWidth != width", fn, base, 2, e.globals_w, EINVAL), ("screenHeight != height", fn, base, 2, e.globals_h, EINVAL)]
        for name, (index, mask) in ATTR_MASKS.items():
            rows += misaligned(fn, base, name, index, mask)
    # where the two differ.  The plain pass takes no material table (attributes only) and then refuses a G-buffer ...
    fn, base = "nv_visibility_attributes", attribute_args(None, 0, None, None)
    rows += [("gbuffer0 without materials", fn, base, 17, p(gb0), EINVAL), ("gbuffer1 without materials", fn, base, 18, p(gb1), EINVAL)]
    # ... the textured pass refuses a NULL table even where it has no entries, and a texture count without the table or the texels
    fn, base = "nv_visibility_attributes_textured", attribute_args(p(materials), 0, None, None) + tex
    rows += [("materials NULL with materialCount 0", fn, base, 14, None, EINVAL)]
    base = attribute_args(p(materials), MATERIALS, p(gb0), p(gb1)) + tex
    rows += null(fn, base, dict(textures=20, texels=22)) + misaligned(fn, base, "textures", 20, 15) + misaligned(fn, base, "texels", 22, 3)
    # ... and so does the block-resident pass, over its table and its blocks
    fn, base = "nv_visibility_attributes_blocks", attribute_args(p(materials), 0, None, None) + btex
    rows += [("materials NULL with materialCount 0", fn, base, 14, None, EINVAL)]
    base = attribute_args(p(materials), MATERIALS, p(gb0), p(gb1)) + btex
    rows += null(fn, base, dict(textures=20, blocks=22)) + misaligned(fn, base, "textures", 20, 15) + misaligned(fn, base, "blocks", 22, 15)
    run(rows)


@pytest.mark.gpu
def test_texture_decode(env):
    e = env
    blocks, texels = e.dev(8), e.dev(16 * 4)  # one BC1 block: 4 x 4 texels

    def desc(*fields):
        d = TextureDesc(*fields)
        e.keep.append(d)
        return C.byref(d)
    fn, base = "nv_texture_decode", [e.h, e.stream, p(blocks), 1, 4, 4, 1, p(texels), desc(0, 4, 4, 1)]
    rows = null(fn, base, dict(context=0, blocks=2, texels=7, desc=8)) + sizes(fn, base, 4, 5)
    rows += [("levels 0", fn, base, 6, 0, EINVAL), ("levels 16", fn, base, 6, 16, EINVAL), ("desc of another width", fn, base, 8, desc(0, 8, 4, 1), EINVAL),
             ("desc of another height", fn, base, 8, desc(0, 4, 8, 1), EINVAL), ("desc of other levels", fn, base, 8, desc(0, 4, 4, 2), EINVAL)]
    rows += misaligned(fn, base, "blocks", 2, 7) + misaligned(fn, base, "texels", 7, 3)
    rows += [("BC4", fn, base, 3, 4, ETEXFORMAT), ("BC5", fn, base, 3, 5, ETEXFORMAT), ("BC6H", fn, base, 3, 6, ETEXFORMAT),
             ("format 0", fn, base, 3, 0, EINVAL), ("format 8", fn, base, 3, 8, EINVAL), ("format 2^32 - 1", fn, base, 3, 2 ** 32 - 1, EINVAL)]
    run(rows)


# ---------------------------------------------------------------------------------------------------------------- shading end

@pytest.mark.gpu
def test_shade_passes(env):
    e = env
    shadow, out, depth, gb0, gb1, color = e.dev(N), e.dev(N), e.dev(N * 4), e.dev(N * 4), e.dev(N * 4), e.dev(N * 4)
    rows = []
    fn, base = "nv_shadow_fill", [e.h, e.stream, p(shadow), p(depth), W, H, 0]
    rows += null(fn, base, dict(context=0, shadow=2, depth=3)) + sizes(fn, base, 4, 5) + misaligned(fn, base, "depth", 3, 3)
    fn, base = "nv_shadow_blur", [e.h, e.stream, p(out), p(shadow), p(depth), W, H, 1, 0.1]
    rows += null(fn, base, dict(context=0, out=2, shadow=3, depth=4)) + sizes(fn, base, 5, 6) + misaligned(fn, base, "depth", 4, 3)
    rows += [("out is shadow", fn, base, 2, p(shadow), EINVAL), ("direction -1", fn, base, 7, -1, EINVAL), ("direction 2", fn, base, 7, 2, EINVAL)]

    desc = host.bloom_desc(W, H)
    assert (desc.width, desc.height, desc.levels) == (4, 2, 3)
    bloom = e.dev(desc.totalTexels * 4)

    def other(**fields):
        d = BloomDesc.from_buffer_copy(desc)
        for k, v in fields.items():
            setattr(d, k, v)
        e.keep.append(d)
        return C.byref(d)
    larger = host.bloom_desc(W * 2, H * 2)
    e.keep += [desc, larger]
    bad_descs = [("desc NULL", None), ("desc of another image", C.byref(larger)), ("desc with another total", other(totalTexels=desc.totalTexels + 1)),
                 ("desc with another level count", other(levels=2)), ("desc of width 0", other(width=0))]

    for fn, tail in (("nv_shade_final", []), ("nv_shade_final_bloom", [p(bloom), C.byref(desc)])):
        base = [e.h, e.stream, e.shade, p(gb0), p(gb1), p(depth), p(shadow), p(color), W, H] + tail
        rows += null(fn, base, dict(context=0, shade=2, gbuffer0=3, gbuffer1=4, depth=5, color=7)) + sizes(fn, base, 8, 9)
        rows += [("imageSize[0] != width", fn, base, 2, e.shade_w, EINVAL), ("imageSize[1] != height", fn, base, 2, e.shade_h, EINVAL),
                 ("shadowsEnabled without a shadow image", fn, base, 6, None, EINVAL)]
        for name, index in dict(gbuffer0=3, gbuffer1=4, depth=5, color=7).items():
            rows += misaligned(fn, base, name, index, 3)
        if tail:
            rows += null(fn, base, dict(bloom=10)) + misaligned(fn, base, "bloom", 10, 3) + [(label, fn, base, 11, d, EINVAL) for label, d in bad_descs]

    for fn in ("nv_bloom_extract", "nv_bloom"):
        base = [e.h, e.stream, p(gb0), W, H, p(bloom), C.byref(desc)]
        rows += null(fn, base, dict(context=0, gbuffer0=2, bloom=5)) + sizes(fn, base, 3, 4) + misaligned(fn, base, "gbuffer0", 2, 3)
        rows += misaligned(fn, base, "bloom", 5, 3) + [(label, fn, base, 6, d, EINVAL) for label, d in bad_descs]
    # the per-level passes take no image size: the descriptor has to be nv_bloom_desc_init's for its own level 0
    per_level = bad_descs[:1] + bad_descs[2:] + [("desc of width 8193", other(width=8193))]
    fn, base = "nv_bloom_downsample", [e.h, e.stream, p(bloom), C.byref(desc), 1]
    rows += null(fn, base, dict(context=0, bloom=2)) + misaligned(fn, base, "bloom", 2, 3) + [(label, fn, base, 3, d, EINVAL) for label, d in per_level]
    rows += [("level 0", fn, base, 4, 0, EINVAL), ("level == levels", fn, base, 4, desc.levels, EINVAL), ("level 2^32 - 1", fn, base, 4, 2 ** 32 - 1, EINVAL)]
    fn, base = "nv_bloom_upsample", [e.h, e.stream, p(bloom), C.byref(desc), 0, 2.0]
    rows += null(fn, base, dict(context=0, bloom=2)) + misaligned(fn, base, "bloom", 2, 3) + [(label, fn, base, 3, d, EINVAL) for label, d in per_level]
    rows += [("level == levels - 1", fn, base, 4, desc.levels - 1, EINVAL), ("level 2^32 - 2", fn, base, 4, 2 ** 32 - 2, EINVAL),
             ("level 2^32 - 1", fn, base, 4, 2 ** 32 - 1, EINVAL), ("radius -1", fn, base, 5, -1.0, EINVAL),
             ("radius below zero by one ulp", fn, base, 5, -1.401298464324817e-45, EINVAL), ("radius NaN", fn, base, 5, float("nan"), EINVAL),
             ("radius +inf", fn, base, 5, float("inf"), EINVAL), ("radius -inf", fn, base, 5, float("-inf"), EINVAL)]
    run(rows)


# ---------------------------------------------------------------------------------------------------------------- shadow trace

@pytest.mark.gpu
def test_shadow_trace(env):
    e = env
    scene, tset = SA.layered_scene()
    depth, shadow = e.dev(N * 4), e.dev(N)
    draws, materials = e.upload(scene["draws"]), e.upload(scene["materials"])
    descs, texels = e.upload(np.ascontiguousarray(tset["descs"], L.TEXTUREDESC)), e.upload(np.ascontiguousarray(tset["texels"], np.uint32))
    trace = [e.h, e.stream, e.shadow_data, p(depth), p(shadow), W, H, 1]
    textured = trace + [p(draws), len(scene["draws"]), p(materials), len(scene["materials"]), p(descs), len(tset["descs"]), p(texels), len(tset["texels"])]
    bdescs, bcount, bblocks, units16 = e.block_set()
    blocks = trace + [p(draws), len(scene["draws"]), p(materials), len(scene["materials"]), p(bdescs), bcount, p(bblocks), units16]
    build = [e.h, e.stream, p(draws), len(scene["draws"])]

    # nothing uploaded: every argument is valid and the context has no scene (the context's first argument is repeated as the "change")
    run([("no scene uploaded", "nv_shadow_trace", trace, 0, e.h, EINVAL), ("no scene uploaded", "nv_shadow_trace_textured", textured, 0, e.h, EINVAL),
         ("no scene uploaded, quality 0", "nv_shadow_trace_textured", textured, 7, 0, EINVAL), ("no scene uploaded", "nv_rt_tlas_build", build, 0, e.h, EINVAL),
         ("no scene uploaded", "nv_shadow_trace_blocks", blocks, 0, e.h, EINVAL), ("no scene uploaded, quality 0", "nv_shadow_trace_blocks", blocks, 7, 0, EINVAL)])

    # a scene without texcoords
    e.ctx.rt_scene_upload(e.ctx.rt_scene_build(scene["meshes"], scene["indices"], scene["vertices"], scene["draws"]))
    fn = "nv_shadow_trace"
    rows = [("a scene built without texcoords", "nv_shadow_trace_textured", textured, 0, e.h, EINVAL),
            ("a scene built without texcoords, quality 0", "nv_shadow_trace_textured", textured, 7, 0, EINVAL),
            ("before nv_rt_scene_reserve_dynamic", "nv_rt_tlas_build", build, 0, e.h, EINVAL),
            ("a scene built without texcoords", "nv_shadow_trace_blocks", blocks, 0, e.h, EINVAL),
            ("a scene built without texcoords, quality 0", "nv_shadow_trace_blocks", blocks, 7, 0, EINVAL)]
    rows += null(fn, trace, dict(context=0, shadow_data=2, depth=3, shadow=4)) + sizes(fn, trace, 5, 6) + misaligned(fn, trace, "depth", 3, 3)
    rows += [("imageSize[0] != width", fn, trace, 2, e.shadow_data_w, EINVAL), ("imageSize[1] != height", fn, trace, 2, e.shadow_data_h, EINVAL),
             ("quality -1", fn, trace, 7, -1, EINVAL), ("quality 2", fn, trace, 7, 2, EINVAL)]
    run(rows)

    e.ctx.rt_scene_reserve_dynamic(4)
    fn = "nv_rt_tlas_build"
    run(null(fn, build, dict(context=0, draws=2)) + misaligned(fn, build, "draws", 2, 3) + [("drawCount above the reservation", fn, build, 3, 5, EINVAL)])

    # the textured scene
    e.ctx.rt_scene_upload(e.ctx.rt_scene_build(scene["meshes"], scene["indices"], scene["vertices"], scene["draws"], texcoords=True))
    fn = "nv_shadow_trace_textured"
    rows = null(fn, textured, dict(context=0, shadow_data=2, depth=3, shadow=4, draws=8, materials=10, textures=12, texels=14)) + sizes(fn, textured, 5, 6)
    rows += [("imageSize[0] != width", fn, textured, 2, e.shadow_data_w, EINVAL), ("imageSize[1] != height", fn, textured, 2, e.shadow_data_h, EINVAL),
             ("quality -1", fn, textured, 7, -1, EINVAL), ("quality 2", fn, textured, 7, 2, EINVAL)]
    for name, (index, mask) in dict(depth=(3, 3), draws=(8, 15), materials=(10, 15), textures=(12, 15), texels=(14, 3)).items():
        rows += misaligned(fn, textured, name, index, mask)
    fn = "nv_shadow_trace_blocks"  # (a count or units16 without its table or buffer: the NULL rows)
    rows += null(fn, blocks, dict(context=0, shadow_data=2, depth=3, shadow=4, draws=8, materials=10, textures=12, blocks=14)) + sizes(fn, blocks, 5, 6)
    rows += [("imageSize[0] != width", fn, blocks, 2, e.shadow_data_w, EINVAL), ("imageSize[1] != height", fn, blocks, 2, e.shadow_data_h, EINVAL),
             ("quality -1", fn, blocks, 7, -1, EINVAL), ("quality 2", fn, blocks, 7, 2, EINVAL)]
    for name, (index, mask) in dict(depth=(3, 3), draws=(8, 15), materials=(10, 15), textures=(12, 15), blocks=(14, 15)).items():
        rows += misaligned(fn, blocks, name, index, mask)
    run(rows)
