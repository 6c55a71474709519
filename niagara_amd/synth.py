"""Synthetic scenes of the BASELINE.json configs (numpy, host side).

The reference generates its stress scene in main() (src/niagara.cpp:969-998); meshlet bounds come from meshoptimizer
there (src/scene.cpp:69-85), which is not vendored, so meshlet pools are drawn from a seeded generator with the
distributions SURVEY.md §8(d) fixes.
"""
import numpy as np

from . import host
from . import layouts as L


def make_meshlets(count, seed=2):
    """centre ~U[-1,1]^3 and radius ~U[0.02,0.1] as fp16; cone axis = random unit vector -> round(127 x) s8;
    cutoff ~U{0..127}"""
    rng = np.random.default_rng(seed)
    m = np.zeros(count, dtype=L.MESHLET)
    m["center"] = rng.uniform(-1, 1, (count, 3)).astype(np.float16).view(np.uint16)
    m["radius"] = rng.uniform(0.02, 0.1, count).astype(np.float16).view(np.uint16)
    axis = rng.normal(size=(count, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    m["cone_axis"] = np.rint(axis * 127).astype(np.int8)
    m["cone_cutoff"] = rng.integers(0, 128, count).astype(np.int8)
    m["vertexCount"] = 64
    m["triangleCount"] = 96
    return m


def make_meshes(mesh_count, lod_count, meshlets_lod0, center=(0.0, 0.0, 0.0), radius=1.8, seed=3):
    """meshes with `lod_count` LODs; LOD i has ceil(meshlets_lod0 / 2^i) meshlets, error 0.002*2^i (error 0 for LOD 0),
    indexCount 86832>>i.  Returns (meshes, total_meshlets); meshlet ranges are packed back to back."""
    rng = np.random.default_rng(seed)
    meshes = np.zeros(mesh_count, dtype=L.MESH)
    offset = 0
    index_offset = 0
    for i in range(mesh_count):
        meshes[i]["center"] = np.asarray(center, np.float32) + rng.uniform(-0.05, 0.05, 3).astype(np.float32) * (mesh_count > 1)
        meshes[i]["radius"] = radius
        meshes[i]["vertexOffset"] = i * 1000
        meshes[i]["vertexCount"] = 1000
        meshes[i]["lodCount"] = lod_count
        for l in range(lod_count):
            mc = max(1, -(-meshlets_lod0 // (1 << l))) if meshlets_lod0 else 0
            lod = meshes[i]["lods"][l]
            lod["indexOffset"] = index_offset
            lod["indexCount"] = 86832 >> l
            lod["meshletOffset"] = offset
            lod["meshletCount"] = mc
            lod["error"] = 0.0 if l == 0 else 0.002 * (1 << l)
            offset += mc
            index_offset += 86832 >> l
    return meshes, offset


def make_task_commands(draw_count, commands_per_draw, late_draw_visibility=None, meshlet_base=0):
    """config 3A: full commands (taskCount 64), command k covers meshlets [64k, 64k+64) and visibility slots alike.
    The array is padded with zeroed dummy commands to a multiple of 64, exactly what tasksubmit leaves behind
    (tasksubmit.comp.glsl:40-46); use count4_for() for the matching {count, X, 64, 1} words."""
    n = draw_count * commands_per_draw
    c = np.zeros((n + 63) // 64 * 64, dtype=L.TASKCMD)
    k = np.arange(n, dtype=np.uint32)
    c["drawId"][:n] = k // commands_per_draw
    c["taskOffset"][:n] = k * 64 + meshlet_base
    c["taskCount"][:n] = 64
    c["meshletVisibilityOffset"][:n] = k * 64
    if late_draw_visibility is not None:
        c["lateDrawVisibility"][:n] = late_draw_visibility[c["drawId"][:n]]
    return c


def count4_for(command_count):
    """the dccb words tasksubmit writes for `command_count` commands (tasksubmit.comp.glsl:30-38)"""
    count = min(command_count, L.TASK_WGLIMIT)
    return np.array([command_count, min((count + 63) // 64, 65535), 64, 1], np.uint32)


def make_depth(width, height, znear=0.1, rects=64, seed=4):
    """reverse-Z depth target: background 0 (far), `rects` axis-aligned rectangles with depth = znear / z, z~U[5,100]"""
    rng = np.random.default_rng(seed)
    depth = np.zeros((height, width), dtype=np.float32)
    for _ in range(rects):
        w = int(rng.integers(max(2, width // 64), max(3, width // 4)))
        h = int(rng.integers(max(2, height // 64), max(3, height // 4)))
        x = int(rng.integers(0, max(1, width - w)))
        y = int(rng.integers(0, max(1, height - h)))
        z = np.float32(rng.uniform(5, 100))
        depth[y:y + h, x:x + w] = np.maximum(depth[y:y + h, x:x + w], np.float32(znear) / z)
    return depth


def cluster_scene(draw_count, commands_per_draw=10, seed=2, scene_radius=300.0):
    """config 3A / 5 inputs: draws (niagara generator), meshlet pool, padded task commands, real command count"""
    draws = host.synth_draws(draw_count, 1, scene_radius)
    n_cmd = draw_count * commands_per_draw
    meshlets = make_meshlets(n_cmd * 64, seed)
    draws["meshletVisibilityOffset"] = np.arange(draw_count, dtype=np.uint32) * (commands_per_draw * 64)
    commands = make_task_commands(draw_count, commands_per_draw)
    return draws, meshlets, commands, n_cmd


def make_globals(cd, viewport):
    """the mesh pipeline's push constants (src/shaders/mesh.h:46-51): niagara's reverse-Z infinite projection
    (perspectiveProjection, src/niagara.cpp:424-431) rebuilt from the P00 / P11 / znear the CullData already carries"""
    g = np.zeros(1, dtype=L.GLOBALS)
    p = np.zeros(16, np.float32)
    p[0], p[5], p[11], p[14] = cd["P00"][0], cd["P11"][0], 1.0, cd["znear"][0]
    g["projection"][0] = p
    g["cullData"][0] = cd[0]
    g["screenWidth"], g["screenHeight"] = viewport
    return g


def make_geometry(meshlets, seed=5, vertices_per_mesh=4096):
    """Synthetic meshlet payloads in niagara's packed form (src/scene.cpp:24-115, src/shaders/meshlet.mesh.glsl:107-127):
    per meshlet `dataOffset` words = vertex references (u16 pairs when shortRefs, else u32) followed by 3 index bytes per
    triangle; vertices = fp16 positions scattered around the meshlet's centre with about its radius.  Fills vertexCount
    (<= 64), triangleCount (<= 96), dataOffset, baseVertex, shortRefs of `meshlets` in place; returns (meshlet_data u32[],
    vertices).  meshoptimizer builds the real thing and is not vendored: distributions only, like the bounds."""
    rng = np.random.default_rng(seed)
    n = len(meshlets)
    vc = rng.integers(3, 65, n).astype(np.uint32)
    tc = np.minimum(rng.integers(1, 97, n), 96).astype(np.uint32)
    short = rng.integers(0, 2, n).astype(np.uint32)
    ref_words = np.where(short == 1, (vc + 1) // 2, vc)
    idx_words = (tc * 3 + 3) // 4
    words = ref_words + idx_words
    offsets = np.concatenate([[0], np.cumsum(words)[:-1]]).astype(np.uint32)
    data = np.zeros(int(words.sum()) + 4, np.uint32)
    d16, d8 = data.view(np.uint16), data.view(np.uint8)
    base = (np.arange(n, dtype=np.uint32) * 61) % max(1, vertices_per_mesh - 64 * 4)  # overlapping windows of a shared pool per "mesh"
    pool = (np.arange(n, dtype=np.uint32) // 4096) * vertices_per_mesh
    base = base + pool
    total_vertices = int(pool.max()) + vertices_per_mesh if n else vertices_per_mesh
    vertices = np.zeros(total_vertices, dtype=L.VERTEX)
    centers = meshlets["center"].view(np.float16).astype(np.float32).reshape(n, 3)
    radii = meshlets["radius"].view(np.float16).astype(np.float32)
    # positions: every vertex of the pool gets a position near the centre of the first meshlet whose window covers it
    vpos = rng.normal(size=(total_vertices, 3)).astype(np.float32)
    owner = np.minimum(np.searchsorted(base, np.arange(total_vertices, dtype=np.uint32), side="right").clip(1) - 1, n - 1) if n else np.zeros(total_vertices, int)
    vpos = centers[owner] + vpos * (radii[owner][:, None] * 0.6)
    vertices["vx"], vertices["vy"], vertices["vz"] = (vpos[:, k].astype(np.float16).view(np.uint16) for k in range(3))
    vertices["np"] = rng.integers(0, 2 ** 32, total_vertices, dtype=np.uint64).astype(np.uint32)
    vertices["tp"] = rng.integers(0, 2 ** 16, total_vertices).astype(np.uint16)
    for i in range(n):
        o, v, t = int(offsets[i]), int(vc[i]), int(tc[i])
        refs = rng.integers(0, 192, v).astype(np.uint32)  # window of 192 pool vertices behind baseVertex
        if short[i]:
            d16[o * 2:o * 2 + v] = refs
        else:
            data[o:o + v] = refs
        io = (o + int(ref_words[i])) * 4
        d8[io:io + t * 3] = rng.integers(0, v, t * 3).astype(np.uint8)
    meshlets["vertexCount"] = vc
    meshlets["triangleCount"] = tc
    meshlets["dataOffset"] = offsets
    meshlets["baseVertex"] = base
    meshlets["shortRefs"] = short
    return data, vertices


def _grid_meshlets(nx, ny, block):
    """a plane of nx x ny quads over [-1, 1]^2 at z = 0, facing +z (counter-clockwise seen from +z), cut into meshlets of block x block
    quads: ((block + 1)^2 <= 64 vertices, 2 block^2 <= 96 triangles).  Returns (positions (n, 3), [(vertex ids, triangles (t, 3) local)])"""
    xs, ys = np.linspace(-1, 1, nx + 1, dtype=np.float32), np.linspace(-1, 1, ny + 1, dtype=np.float32)
    vid = lambda i, j: j * (nx + 1) + i
    pos = np.array([(xs[i], ys[j], 0.0) for j in range(ny + 1) for i in range(nx + 1)], np.float32)
    out = []
    for bj in range(0, ny, block):
        for bi in range(0, nx, block):
            tris = []
            for j in range(bj, min(bj + block, ny)):
                for i in range(bi, min(bi + block, nx)):
                    a, b, c, d = vid(i, j), vid(i + 1, j), vid(i + 1, j + 1), vid(i, j + 1)
                    tris += [(a, b, c), (a, c, d)]
            out.append(tris)
    return pos, out


def _box_faces(n):
    """a closed cube [-1, 1]^3, every face n x n quads, outward faces counter-clockwise: (positions, [triangles]) as one meshlet"""
    pos, (tris,) = _grid_meshlets(n, n, n)
    faces = [np.eye(3, dtype=np.float32)[[0, 1, 2]],  # +z: x, y, normal
             np.array([[-1, 0, 0], [0, 1, 0], [0, 0, -1]], np.float32),  # -z
             np.array([[0, 0, -1], [0, 1, 0], [1, 0, 0]], np.float32),   # +x
             np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], np.float32),   # -x
             np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32),   # +y
             np.array([[1, 0, 0], [0, 0, 1], [0, -1, 0]], np.float32)]   # -y
    allpos, alltris = [], []
    for k, m in enumerate(faces):
        p = pos[:, :1] * m[0] + pos[:, 1:2] * m[1] + m[2]  # u, v in the face plane, pushed out along its normal
        alltris += [(a + k * len(pos), b + k * len(pos), c + k * len(pos)) for a, b, c in tris]
        allpos.append(p)
    return np.concatenate(allpos).astype(np.float32), [alltris]


def occluder_scene(viewport=(320, 192), wall_distance=20.0, wall_half=12.0, hidden=8, beside=4, box_scale=1.0, hidden_spread=4.0,
                   seed=6, meshlet_bounds=None):
    """A controlled scene with real surfaces for the closed occlusion loop: a wall (a tessellated grid, 24 x 24 quads in meshlets of
    6 x 6) facing the camera at `wall_distance`, `hidden` closed boxes behind it within +-`hidden_spread` of its centre line (their
    HiZ footprints lie well inside the wall) and `beside` boxes to its left and right that it does not cover.  The camera is
    niagara's default (origin, looking down -z).  Meshlet bounds are the library's algorithm: `meshlet_bounds(vertices, data, meshlets)`
    fills them in place (oracle.meshlet_bounds), or, when None, Context.meshlet_bounds on the current device.
    Returns a dict of meshes, meshlets, draws, meshlet data, vertices, cull data, viewport and the draw ids of each group."""
    rng = np.random.default_rng(seed)
    wall_pos, wall_tris = _grid_meshlets(24, 24, 6)
    box_pos, box_tris = _box_faces(2)
    meshes = np.zeros(2, dtype=L.MESH)
    meshlet_list, words, vertices = [], [], []
    vbase = 0
    for mi, (pos, groups, short) in enumerate(((wall_pos, wall_tris, 0), (box_pos, box_tris, 1))):
        h = pos.astype(np.float16)
        v = np.zeros(len(pos), dtype=L.VERTEX)
        v["vx"], v["vy"], v["vz"] = (h[:, k].view(np.uint16) for k in range(3))
        vertices.append(v)
        center, radius = host.mesh_bounds(h.astype(np.float32))
        meshes[mi]["center"], meshes[mi]["radius"] = center, radius
        meshes[mi]["vertexOffset"], meshes[mi]["vertexCount"] = vbase, len(pos)
        meshes[mi]["lodCount"] = 1
        lod = meshes[mi]["lods"][0]
        lod["meshletOffset"], lod["meshletCount"], lod["indexCount"] = len(meshlet_list), len(groups), 3 * sum(len(g) for g in groups)
        for tris in groups:
            t = np.asarray(tris, np.uint32)
            used = np.unique(t)
            local = np.searchsorted(used, t).astype(np.uint8)
            assert len(used) <= 64 and len(t) <= 96
            m = np.zeros(1, dtype=L.MESHLET)
            m["dataOffset"] = sum(len(w) for w in words)
            m["baseVertex"] = vbase
            m["vertexCount"], m["triangleCount"], m["shortRefs"] = len(used), len(t), short
            refs = used.astype(np.uint16 if short else np.uint32)
            if short and len(refs) % 2:
                refs = np.append(refs, np.uint16(0))
            idx = local.reshape(-1)
            idx = np.append(idx, np.zeros((-len(idx)) % 4, np.uint8))
            words.append(np.concatenate([refs.view(np.uint32), idx.view(np.uint32)]))
            meshlet_list.append(m)
        vbase += len(pos)
    meshlets = np.concatenate(meshlet_list)
    data = np.concatenate(words + [np.zeros(4, np.uint32)]).astype(np.uint32)
    vertices = np.concatenate(vertices)
    if meshlet_bounds is None:
        from . import pipeline as P
        import torch
        ctx = P.Context()
        try:
            mlb = P.to_device(meshlets, ctx.device)
            ctx.meshlet_bounds(P.to_device(vertices, ctx.device), P.to_device(data, ctx.device), mlb, len(meshlets))
            ctx.status()
            meshlets = P.from_device(mlb, L.MESHLET).copy()
        finally:
            ctx.close()
        del torch
    else:
        meshlet_bounds(vertices, data, meshlets)

    n = 1 + hidden + beside
    draws = np.zeros(n, dtype=L.MESHDRAW)
    draws["orientation"] = (0.0, 0.0, 0.0, 1.0)
    draws[0]["position"], draws[0]["scale"], draws[0]["meshIndex"] = (0.0, 0.0, -wall_distance), wall_half, 0
    for i in range(1, n):
        draws[i]["meshIndex"], draws[i]["scale"] = 1, box_scale
        d = rng.uniform(1.5, 2.0) * wall_distance
        if i <= hidden:
            x, y = rng.uniform(-hidden_spread, hidden_spread, 2)
        else:
            side = 1.0 if (i - hidden) % 2 else -1.0
            x, y = side * rng.uniform(1.3, 1.6) * wall_half * d / wall_distance, rng.uniform(-hidden_spread, hidden_spread)
        draws[i]["position"] = (x, y, -d)
    slots, _ = host.assign_visibility_offsets(draws, meshes)
    pw, ph = host.previous_pow2(viewport[0]), host.previous_pow2(viewport[1])
    cd = host.build_cull_data(viewport=viewport, pyramid=(pw, ph), draw_count=n, cullingEnabled=1, lodEnabled=1, occlusionEnabled=1,
                              clusterOcclusionEnabled=1, clusterBackfaceEnabled=1)
    return dict(meshes=meshes, meshlets=meshlets, draws=draws, data=data, vertices=vertices, cull=cd, viewport=viewport, slots=slots,
                wall=[0], hidden=list(range(1, 1 + hidden)), beside=list(range(1 + hidden, n)))


def indexed_geometry(meshes, meshlets, data):
    """The index buffer of niagara's classic path recovered from the meshlet payloads: every LOD's meshlets decoded in order into mesh-local
    vertex ids (reference + baseVertex - the mesh's vertexOffset, as drawcull's MeshDrawCommand adds vertexOffset back) and laid back to back.
    Triangles whose index byte is past min(vertexCount, 64) are left out (the cluster path skips them).  Returns (indices u32[], a copy of
    `meshes` with each LOD's indexOffset / indexCount set)."""
    meshes = meshes.copy()
    d16, d8 = data.view(np.uint16), data.view(np.uint8)
    out, at = [], 0
    for mi in range(len(meshes)):
        base = int(meshes[mi]["vertexOffset"])
        for l in range(int(meshes[mi]["lodCount"])):
            first, count = int(meshes["lods"]["meshletOffset"][mi, l]), int(meshes["lods"]["meshletCount"][mi, l])
            for k in range(first, first + count):
                m = meshlets[k]
                vc, tc, off, short = int(m["vertexCount"]), min(int(m["triangleCount"]), 96), int(m["dataOffset"]), m["shortRefs"] == 1
                refs = (d16[off * 2:off * 2 + vc] if short else data[off:off + vc]).astype(np.int64) + int(m["baseVertex"]) - base
                io = (off + ((vc + 1) // 2 if short else vc)) * 4
                idx = d8[io:io + 3 * tc].reshape(-1, 3).astype(np.int64)
                out.append(refs[idx[(idx < min(vc, 64)).all(axis=1)]].reshape(-1))
            n = sum(len(t) for t in out) - at
            meshes["lods"]["indexOffset"][mi, l], meshes["lods"]["indexCount"][mi, l] = at, n
            at += n
    indices = np.concatenate(out).astype(np.uint32) if out else np.zeros(0, np.uint32)
    return indices, meshes


def occluder_scene_indexed(**kw):
    """occluder_scene(**kw) for the classic path: the same scene plus its index buffer ("indices") and the meshes with their LODs' index
    ranges set (indexed_geometry)"""
    s = occluder_scene(**kw)
    indices, meshes = indexed_geometry(s["meshes"], s["meshlets"], s["data"])
    return dict(s, meshes=meshes, indices=indices)


def _pack_meshes(parts, meshlet_bounds):
    """(positions, [triangles per meshlet], shortRefs) per mesh -> (meshes, meshlets, meshlet data, vertices) with one LOD each, as
    occluder_scene lays them out; meshlet bounds by `meshlet_bounds(vertices, data, meshlets)` (in place)"""
    meshes = np.zeros(len(parts), dtype=L.MESH)
    meshlet_list, words, vertices = [], [], []
    vbase = 0
    for mi, (pos, groups, short) in enumerate(parts):
        h = pos.astype(np.float16)
        v = np.zeros(len(pos), dtype=L.VERTEX)
        v["vx"], v["vy"], v["vz"] = (h[:, k].view(np.uint16) for k in range(3))
        vertices.append(v)
        center, radius = host.mesh_bounds(h.astype(np.float32))
        meshes[mi]["center"], meshes[mi]["radius"] = center, radius
        meshes[mi]["vertexOffset"], meshes[mi]["vertexCount"] = vbase, len(pos)
        meshes[mi]["lodCount"] = 1
        lod = meshes[mi]["lods"][0]
        lod["meshletOffset"], lod["meshletCount"], lod["indexCount"] = len(meshlet_list), len(groups), 3 * sum(len(g) for g in groups)
        for tris in groups:
            t = np.asarray(tris, np.uint32)
            used = np.unique(t)
            local = np.searchsorted(used, t).astype(np.uint8)
            assert len(used) <= 64 and len(t) <= 96
            m = np.zeros(1, dtype=L.MESHLET)
            m["dataOffset"] = sum(len(w) for w in words)
            m["baseVertex"] = vbase
            m["vertexCount"], m["triangleCount"], m["shortRefs"] = len(used), len(t), short
            refs = used.astype(np.uint16 if short else np.uint32)
            if short and len(refs) % 2:
                refs = np.append(refs, np.uint16(0))
            idx = local.reshape(-1)
            idx = np.append(idx, np.zeros((-len(idx)) % 4, np.uint8))
            words.append(np.concatenate([refs.view(np.uint32), idx.view(np.uint32)]))
            meshlet_list.append(m)
        vbase += len(pos)
    meshlets = np.concatenate(meshlet_list)
    data = np.concatenate(words + [np.zeros(4, np.uint32)]).astype(np.uint32)
    vertices = np.concatenate(vertices)
    meshlet_bounds(vertices, data, meshlets)
    return meshes, meshlets, data, vertices


def interior_scene(viewport=(320, 192), half=30.0, eye_height=1.5, wall_x=1.5, below=4, behind=4, open_=4, box_scale=0.5, seed=7,
                   meshlet_bounds=None):
    """The camera inside the geometry, for the closed loop with near-plane clipping (NV_OPT_RASTER_NEAR_CLIP): niagara's default camera
    (origin, looking down -z) stands `eye_height` above a floor and `wall_x` to the left of a wall.  Both are one coarse grid (4 x 4 quads in
    meshlets of 2 x 2) of half-extent `half` centred under / beside the camera, so every triangle between the camera and 15 units ahead
    crosses the near plane: without clipping only the far half of either surface is drawn.  `below` closed boxes lie 3.5 units under the
    floor and `behind` as far behind the wall, 9 to 13 units ahead: inside the frustum, close enough that the undrawn part is what hides
    them, and deep enough that the 2 x 2 pyramid texels of their test (up to twice the size of the sphere's box) still see only the surface
    in front of them.  `open_` boxes stand on the open side.  `meshlet_bounds(vertices, data, meshlets)` fills the bounds in place (oracle.meshlet_bounds; required here: no device is
    opened).  Returns occluder_scene's dict with the draw ids of "surfaces", "hidden" (below + behind) and "open"."""
    if meshlet_bounds is None:
        raise ValueError("interior_scene needs meshlet_bounds= (oracle.meshlet_bounds)")
    rng = np.random.default_rng(seed)
    grid_pos, grid_tris = _grid_meshlets(4, 4, 2)
    box_pos, box_tris = _box_faces(2)
    meshes, meshlets, data, vertices = _pack_meshes(((grid_pos, grid_tris, 0), (box_pos, box_tris, 1)), meshlet_bounds)
    n = 2 + below + behind + open_
    draws = np.zeros(n, dtype=L.MESHDRAW)
    draws["orientation"] = (0.0, 0.0, 0.0, 1.0)
    r = np.float32(np.sqrt(0.5))
    # the grid faces +z: about x by -90 degrees it faces +y (the floor), about y by -90 degrees it faces -x (the wall, seen from the camera)
    draws[0]["position"], draws[0]["scale"], draws[0]["orientation"] = (0.0, -eye_height, 0.0), half, (-r, 0.0, 0.0, r)
    draws[1]["position"], draws[1]["scale"], draws[1]["orientation"] = (wall_x, 0.0, 0.0), half, (0.0, -r, 0.0, r)
    for i in range(2, n):
        draws[i]["meshIndex"], draws[i]["scale"] = 1, box_scale
        z = -rng.uniform(9.0, 13.0)
        if i < 2 + below:
            pos = (rng.uniform(-3.0, 0.5), -eye_height - 3.5, z)
        elif i < 2 + below + behind:
            pos = (wall_x + 3.5, rng.uniform(0.5, 2.0), z)
        else:
            pos = (rng.uniform(-7.0, -1.0), rng.uniform(0.5, 2.0), z)
        draws[i]["position"] = pos
    slots, _ = host.assign_visibility_offsets(draws, meshes)
    pw, ph = host.previous_pow2(viewport[0]), host.previous_pow2(viewport[1])
    cd = host.build_cull_data(viewport=viewport, pyramid=(pw, ph), draw_count=n, cullingEnabled=1, lodEnabled=1, occlusionEnabled=1,
                              clusterOcclusionEnabled=1, clusterBackfaceEnabled=1)
    return dict(meshes=meshes, meshlets=meshlets, draws=draws, data=data, vertices=vertices, cull=cd, viewport=viewport, slots=slots,
                surfaces=[0, 1], hidden=list(range(2, 2 + below + behind)), open=list(range(2 + below + behind, n)))


def interior_scene_indexed(**kw):
    """interior_scene(**kw) for the classic path: the same scene plus its index buffer ("indices") and the meshes with their LODs' index
    ranges set (indexed_geometry)"""
    s = interior_scene(**kw)
    indices, meshes = indexed_geometry(s["meshes"], s["meshlets"], s["data"])
    return dict(s, meshes=meshes, indices=indices)


# ---- material textures: content for tools and tests

def _rgb565(c):
    """(..., 3) uint8 -> the 565 code (truncating: the encoder's endpoints need not be the nearest codes)"""
    c = c.astype(np.uint32)
    return (c[..., 0] >> 3) << 11 | (c[..., 1] >> 2) << 5 | c[..., 2] >> 3


def _expand565(code):
    r, g, b = code >> 11 & 31, code >> 5 & 63, code & 31
    return np.stack([(r * 255 + 15) // 31, (g * 255 + 31) // 63, (b * 255 + 15) // 31], -1).astype(np.int64)


def bc1_encode(image, cutout=False):
    """a minimal BC1 encoder: image (h, w, 3 or 4) uint8 -> the blocks' bytes, row-major.  Per block the endpoints are the per-channel maximum
    and minimum (c0 > c1: the four-colour mode; a flat block stores c0 = c1 and index 0), every texel takes the nearest of the four colours.
    Partial blocks repeat the edge texels.  Alpha is ignored (BC1 here is opaque) unless `cutout`: then a block with a texel of alpha < 128
    is stored in the punch-through mode (c0 <= c1: two endpoints and their half, index 3 = transparent black), its transparent texels take
    index 3 and the others the nearest of the three colours; blocks without such a texel are encoded as before"""
    full = np.asarray(image, np.uint8)
    if cutout and full.shape[-1] == 4:
        return _bc1_encode_cutout(full)
    img = full[..., :3]
    h, w = img.shape[:2]
    img = np.pad(img, ((0, -h % 4), (0, -w % 4), (0, 0)), mode="edge")
    bh, bw = img.shape[0] // 4, img.shape[1] // 4
    blocks = img.reshape(bh, 4, bw, 4, 3).transpose(0, 2, 1, 3, 4).reshape(bh * bw, 16, 3)
    c0, c1 = _rgb565(blocks.max(axis=1)), _rgb565(blocks.min(axis=1))
    swap = c0 < c1  # per-channel extremes are ordered channel by channel; the packed codes almost always are too
    c0, c1 = np.where(swap, c1, c0), np.where(swap, c0, c1)
    e0, e1 = _expand565(c0), _expand565(c1)
    palette = np.stack([e0, e1, (2 * e0 + e1) // 3, (e0 + 2 * e1) // 3], axis=1)  # (n, 4, 3)
    dist = ((blocks[:, :, None, :].astype(np.int64) - palette[:, None, :, :]) ** 2).sum(-1)  # (n, 16, 4)
    idx = np.where((c0 == c1)[:, None], 0, dist.argmin(-1)).astype(np.uint32)
    bits = (idx << (2 * np.arange(16, dtype=np.uint32))[None, :]).sum(axis=1).astype(np.uint32)
    out = np.zeros((bh * bw, 2), np.uint32)
    out[:, 0] = c0.astype(np.uint32) | c1.astype(np.uint32) << 16
    out[:, 1] = bits
    return out.tobytes()


def _bc1_encode_cutout(image):
    """bc1_encode(image, cutout=True): the opaque encoding with the blocks that hold a transparent texel replaced by punch-through blocks"""
    h, w = image.shape[:2]
    out = np.frombuffer(bc1_encode(image[..., :3]), np.uint32).reshape(-1, 2).copy()
    img = np.pad(image, ((0, -h % 4), (0, -w % 4), (0, 0)), mode="edge")
    bh, bw = img.shape[0] // 4, img.shape[1] // 4
    blocks = img.reshape(bh, 4, bw, 4, 4).transpose(0, 2, 1, 3, 4).reshape(bh * bw, 16, 4)
    clear = blocks[:, :, 3] < 128
    punch = clear.any(axis=1)
    if not punch.any():
        return out.tobytes()
    b, t = blocks[punch][:, :, :3], clear[punch]
    solid = np.where(t[:, :, None], 0, b)  # the endpoints come from the opaque texels alone (a block without one stores black)
    low = np.where(t[:, :, None], 255, b)
    hi, lo = _rgb565(solid.max(axis=1)), _rgb565(np.where(t.all(axis=1)[:, None], 0, low.min(axis=1)))
    c0, c1 = np.minimum(hi, lo), np.maximum(hi, lo)  # c0 <= c1: the three-colour mode
    e0, e1 = _expand565(c0), _expand565(c1)
    palette = np.stack([e0, e1, (e0 + e1) // 2], axis=1)
    dist = ((b[:, :, None, :].astype(np.int64) - palette[:, None, :, :]) ** 2).sum(-1)
    idx = np.where(t, 3, dist.argmin(-1)).astype(np.uint32)
    out[punch, 0] = c0.astype(np.uint32) | c1.astype(np.uint32) << 16
    out[punch, 1] = (idx << (2 * np.arange(16, dtype=np.uint32))[None, :]).sum(axis=1).astype(np.uint32)
    return out.tobytes()


def _half_image(img):
    """the next mip level: max(1, side // 2) per axis, the mean of the 2 x 2 (or 2 x 1, 1 x 2) source texels"""
    h, w = img.shape[:2]
    nh, nw = max(1, h // 2), max(1, w // 2)
    ys, xs = np.minimum(np.arange(nh) * 2, h - 1), np.minimum(np.arange(nw) * 2, w - 1)
    ys1, xs1 = np.minimum(ys + 1, h - 1), np.minimum(xs + 1, w - 1)
    s = img.astype(np.uint32)
    return ((s[ys][:, xs] + s[ys][:, xs1] + s[ys1][:, xs] + s[ys1][:, xs1] + 2) // 4).astype(np.uint8)


def dds_bytes(image, mips=True, cutout=False):
    """a DDS file image as niagara's loadImage accepts it (src/textures.cpp:159-210): FourCC DXT1, the BC1 blocks of `image` and, with mips,
    of its whole chain down to 1 x 1; cutout: bc1_encode's punch-through alpha"""
    img = np.asarray(image, np.uint8)
    h, w = img.shape[:2]
    levels, payload = 0, b""
    while True:
        payload += bc1_encode(img, cutout)
        levels += 1
        if not mips or (img.shape[0] == 1 and img.shape[1] == 1):
            break
        img = _half_image(img)
    head = np.zeros(32, np.uint32)
    head[0] = 0x20534444                      # "DDS "
    head[1], head[2] = 124, 0x1 | 0x2 | 0x4 | 0x1000 | 0x20000 | 0x80000  # dwSize; CAPS | HEIGHT | WIDTH | PIXELFORMAT | MIPMAPCOUNT | LINEARSIZE
    head[3], head[4] = h, w
    head[5] = ((w + 3) // 4) * ((h + 3) // 4) * 8
    head[7] = levels
    head[19], head[20], head[21] = 32, 0x4, 0x31545844  # ddspf: dwSize, DDPF_FOURCC, "DXT1"
    head[27] = 0x1000 | (0x400008 if levels > 1 else 0)  # DDSCAPS_TEXTURE (| COMPLEX | MIPMAP)
    return head.tobytes() + payload


def texture_images(size=64):
    """the four images of with_textures: a checker albedo, a bump normal map, a specular map, an emissive map; (size, size, 4) uint8 each"""
    y, x = np.mgrid[0:size, 0:size]
    cell = size // 8 or 1
    check = ((x // cell + y // cell) % 2).astype(np.float64)
    albedo = np.stack([0.9 - 0.6 * check, 0.35 + 0.5 * check, 0.25 + 0.1 * check, np.ones_like(check)], -1)
    fx, fy = 2 * np.pi * x / size, 2 * np.pi * y / size
    nx, ny = 0.45 * np.cos(2 * fx), 0.45 * np.cos(2 * fy)
    nz = np.sqrt(np.maximum(0.0, 1 - nx * nx - ny * ny))
    normal = np.stack([nx * 0.5 + 0.5, ny * 0.5 + 0.5, nz * 0.5 + 0.5, np.ones_like(nx)], -1)
    spec = np.stack([0.5 + 0.5 * np.sin(fx), 0.5 + 0.5 * np.sin(fy), check, np.ones_like(check)], -1)
    glow = np.exp(-(((x - size / 2) ** 2 + (y - size / 2) ** 2) / (size / 4) ** 2))
    emissive = np.stack([glow, 0.6 * glow, 0.2 * glow, np.ones_like(glow)], -1)
    return [np.rint(np.clip(i, 0, 1) * 255).astype(np.uint8) for i in (albedo, normal, spec, emissive)]


def with_textures(scene, size=64, mips=True, cutout=False):
    """cutout: the albedo's darker checker cells are transparent (alpha 0, BC1 punch-through): a cut-out caster for the alpha-tested shadow
    trace.  A copy of a scene dict with "textures" — four DDS file images (BC1): a checker albedo, a bump normal map, a specular map and an emissive
    map, textures[1..4] of the set — and a material table ("materials"; created with five entries spread over the draws when the scene has
    none) whose every entry names all four.  Vertices without texcoords (all zero, as make_geometry leaves them) get a planar map of their
    positions"""
    s = dict(scene)
    images = texture_images(size)
    if cutout:
        cell = size // 8 or 1
        y, x = np.mgrid[0:size, 0:size]
        images[0] = images[0].copy()
        images[0][..., 3] = np.where((x // cell + y // cell) % 2 == 1, 0, 255)
    s["textures"] = [dds_bytes(img, mips, cutout and k == 0) for k, img in enumerate(images)]
    if "materials" in s:
        m = s["materials"].copy()
    else:
        m = np.zeros(5, L.MATERIAL)
        m["diffuseFactor"], m["specularFactor"] = (0.9, 0.9, 0.9, 1.0), (0.5, 0.5, 0.5, 0.6)
        m["emissiveFactor"] = (1.0, 1.0, 1.0)
        s["draws"] = s["draws"].copy()
        s["draws"]["materialIndex"] = np.arange(len(s["draws"])) % len(m)
    m["albedoTexture"], m["normalTexture"], m["specularTexture"], m["emissiveTexture"] = 1, 2, 3, 4
    s["materials"] = m
    v = s["vertices"]
    if not (v["tu"].any() or v["tv"].any()):
        v = v.copy()
        pos = np.stack([v["vx"], v["vy"], v["vz"]], -1).view(np.float16).astype(np.float32)
        uv = (np.stack([pos[:, 0] + 0.25 * pos[:, 2], pos[:, 1] - 0.25 * pos[:, 2]], -1) * 0.5 + 0.5).astype(np.float16)
        v["tu"], v["tv"] = uv[:, 0].view(np.uint16), uv[:, 1].view(np.uint16)
        s["vertices"] = v
    return s


def orbit_animations(draws, which, keyframes_per=8, seed=11, orbit=2.0, period=(0.25, 2.0), start=(0.0, 1.0)):
    """(animations, keyframes), layouts.ANIMATION / KEYFRAME: one animation per draw index in `which` (no duplicates), `keyframes_per`
    keyframes each (an int, or one count per animation).  Keyframe j of an animation places the draw on a circle of radius `orbit` x its scale
    around its position in `draws`, in a random plane, with the draw's scale x U[0.75, 1.25] and a unit quaternion that turns by j / count
    of a full turn about a random axis from the draw's own orientation; every fourth animation repeats a rotation in two neighbouring
    keyframes (slerp's linear branch) and every third flips the sign of every other keyframe's quaternion (its negated-y path).  period and
    startTime ~U[period], U[start].  For tests and tools: the reference reads its animations from glTF (src/scene.cpp)"""
    rng = np.random.default_rng(seed)
    which = np.asarray(which, np.int64).reshape(-1)
    if len(np.unique(which)) != len(which):
        raise ValueError("orbit_animations: a draw index appears twice (nv_upload_animations refuses duplicate targets)")
    n = len(which)
    counts = np.broadcast_to(np.asarray(keyframes_per, np.int64), (n,)).copy()
    if n and counts.min() < 1:
        raise ValueError("orbit_animations: every animation needs at least one keyframe")
    anims = np.zeros(n, L.ANIMATION)
    anims["drawIndex"] = which
    anims["lightIndex"] = -1
    anims["startTime"] = rng.uniform(start[0], start[1], n).astype(np.float32)
    anims["period"] = rng.uniform(period[0], period[1], n).astype(np.float32)
    anims["keyframeCount"] = counts
    anims["keyframeOffset"] = np.concatenate([[0], np.cumsum(counts)[:-1]]) if n else 0
    total = int(counts.sum())
    keys = np.zeros(total, L.KEYFRAME)
    if not total:
        return anims, keys
    owner = np.repeat(np.arange(n), counts)
    j = np.arange(total) - np.repeat(anims["keyframeOffset"].astype(np.int64), counts)
    phase = 2.0 * np.pi * j / counts[owner]

    def unit(v):
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    u = unit(rng.normal(size=(n, 3)))
    w = unit(np.cross(u, rng.normal(size=(n, 3))))
    d = draws[which]
    radius = orbit * d["scale"].astype(np.float64)
    centre = d["position"].astype(np.float64)
    keys["translation"] = (centre[owner] + radius[owner, None] * (np.cos(phase)[:, None] * u[owner] + np.sin(phase)[:, None] * w[owner])).astype(np.float32)
    keys["scale"] = (d["scale"].astype(np.float64)[owner] * rng.uniform(0.75, 1.25, total)).astype(np.float32)
    # rotation: q_draw * (axis sin(phase / 2), cos(phase / 2)), components (x, y, z, w)
    axis = unit(rng.normal(size=(n, 3)))[owner]
    held = (owner % 4 == 0) & (j % 2 == 1)  # repeats keyframe j - 1's rotation
    half = 0.5 * np.where(held, 2.0 * np.pi * (j - 1) / counts[owner], phase)
    b = axis * np.sin(half)[:, None]
    bx, by, bz, bw = b[:, 0], b[:, 1], b[:, 2], np.cos(half)
    q = d["orientation"].astype(np.float64)[owner]
    norm = np.linalg.norm(q, axis=1)
    q = np.where(norm[:, None] > 0, q / np.where(norm > 0, norm, 1.0)[:, None], np.array([0.0, 0.0, 0.0, 1.0]))
    ax, ay, az, aw = q.T
    r = np.stack([aw * bx + ax * bw + ay * bz - az * by,
                  aw * by - ax * bz + ay * bw + az * bx,
                  aw * bz + ax * by - ay * bx + az * bw,
                  aw * bw - ax * bx - ay * by - az * bz], axis=1)
    r = unit(r)
    flip = (owner % 3 == 0) & (j % 2 == 1)
    r[flip] = -r[flip]
    keys["rotation"] = r.astype(np.float32)
    return anims, keys
