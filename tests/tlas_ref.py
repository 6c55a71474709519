"""An independent numpy restatement of the rebuilt TLAS's key, order and tree (test infrastructure).  It takes the leaf boxes
and draw ids of the casters in ANY order, recomputes the middles, the cells and the Morton keys in fp32, orders by (key, drawId) and splits
the sorted strings key << 32 | k recursively at their highest differing bit: the `skip` and `leaf` words of the preorder layout and the
instance order a correct build must reproduce.  Also the blob's sections and the draw sets the TLAS tests share."""
import numpy as np

from niagara_amd import layouts as L

HEADER = np.dtype([(n, "<u4") for n in ("magic", "version", "bytes", "meshCount", "tlasNodes", "instances", "blasNodes", "triangles", "tableOff", "tlasOff",
                                         "instOff", "blasOff", "triOff")] + [("padOrigin", "<f4"), ("drawCount", "<u4"), ("reserved", "<u4")])
NODE = np.dtype([("lo", "<f4", 3), ("skip", "<u4"), ("hi", "<f4", 3), ("leaf", "<u4")])
INSTANCE = np.dtype([("position", "<f4", 3), ("scale", "<f4"), ("orientation", "<f4", 4), ("drawId", "<u4"), ("postPass", "<u4"), ("blas", "<u4"), ("reserved", "<u4", 5)])
LEAF_SHIFT = 29
F = np.float32


def sections(blob):
    """header, TLAS nodes, instances, and the bytes of the static side (BLAS table, BLAS nodes, triangles)"""
    h = blob[:64].view(HEADER)[0]
    part = lambda off, count, size: blob[int(off):int(off) + int(count) * size]
    static = (part(h["tableOff"], h["meshCount"], 32).tobytes(), part(h["blasOff"], h["blasNodes"], 32).tobytes(), part(h["triOff"], h["triangles"], 48).tobytes())
    return h, part(h["tlasOff"], h["tlasNodes"], 32).view(NODE), part(h["instOff"], h["instances"], 64).view(INSTANCE), static


def _spread3(v):
    v = v.astype(np.uint32)
    out = np.zeros_like(v)
    for bit in range(10):
        out |= ((v >> np.uint32(bit)) & np.uint32(1)) << np.uint32(3 * bit)
    return out


def keys(lo, hi):
    """the 30-bit Morton keys of boxes (n, 3) fp32: every operation one fp32 operation"""
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    with np.errstate(all="ignore"):
        mid = lo * F(0.5) + hi * F(0.5)
        mid = np.where(np.isfinite(mid), mid, F(0.0)).astype(F)
        q = np.zeros(mid.shape, np.uint32)
        if len(mid):
            mlo, mhi = mid.min(0), mid.max(0)
            for k in range(3):
                if not mhi[k] > mlo[k]:
                    continue
                ext = F(mhi[k] * F(0.5)) - F(mlo[k] * F(0.5))
                if not ext > 0:
                    continue
                t = (mid[:, k] * F(0.5) - mlo[k] * F(0.5)) / ext
                c = np.minimum(np.maximum(t * F(1024.0), F(0.0)), F(1023.0))
                assert c.dtype == F
                q[:, k] = c.astype(np.uint32)
    return (_spread3(q[:, 0]) << np.uint32(2)) | (_spread3(q[:, 1]) << np.uint32(1)) | _spread3(q[:, 2])


def tree(sorted_keys):
    """(skip, leaf, depth) of the radix tree of key << 32 | k over the sorted keys, in the preorder layout"""
    n = len(sorted_keys)
    if n == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32), 0
    strings = (np.asarray(sorted_keys).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    skip, leaf = np.zeros(2 * n - 1, np.uint32), np.zeros(2 * n - 1, np.uint32)
    stack, deepest = [(0, 0, n - 1, 0)], 0
    while stack:
        pos, l, r, depth = stack.pop()
        deepest = max(deepest, depth)
        skip[pos] = pos + 2 * (r - l + 1) - 1
        if l == r:
            leaf[pos] = 1 << LEAF_SHIFT | l
            continue
        bit = (int(strings[l]) ^ int(strings[r])).bit_length() - 1
        split = l + int(np.searchsorted((strings[l:r + 1] >> np.uint64(bit)) & np.uint64(1), 1))  # the first string with the bit set
        stack.append((pos + 1, l, split - 1, depth + 1))
        stack.append((pos + 2 * (split - l), split, r, depth + 1))
    return skip, leaf, deepest


def restate(lo, hi, draw_ids):
    """dict(order = the draw ids in instance order, skip, leaf, depth) from the casters' boxes and draw ids in any order"""
    k = keys(lo, hi)
    ids = np.asarray(draw_ids, np.uint32)
    order = np.lexsort((ids, k))
    skip, leaf, depth = tree(k[order])
    return dict(order=ids[order], perm=order, skip=skip, leaf=leaf, depth=depth, keys=k[order])


def check_blob(blob, shuffle_seed=0):
    """the rebuilt blob against the restatement (fed the leaves in a shuffled order) and the box rules; returns the restatement"""
    h, nodes, inst, _ = sections(blob)
    n = int(h["instances"])
    assert len(nodes) == (2 * n - 1 if n else 0)
    leaves = np.flatnonzero(nodes["leaf"] != 0)
    assert len(leaves) == n
    first = nodes["leaf"][leaves] & np.uint32((1 << LEAF_SHIFT) - 1)
    assert (first == np.arange(n)).all() and (nodes["leaf"][leaves] >> LEAF_SHIFT == 1).all()  # leaf k holds instance k, in preorder
    perm = np.random.default_rng(shuffle_seed).permutation(n)
    r = restate(nodes["lo"][leaves][perm], nodes["hi"][leaves][perm], inst["drawId"][perm])
    assert r["order"].tolist() == inst["drawId"].tolist()
    assert r["skip"].tolist() == nodes["skip"].tolist() and r["leaf"].tolist() == nodes["leaf"].tolist()
    inner = np.flatnonzero(nodes["leaf"] == 0)
    if len(inner):
        a, b = inner + 1, nodes["skip"][inner + 1]
        assert (nodes["lo"][inner] == np.minimum(nodes["lo"][a], nodes["lo"][b])).all() and (nodes["hi"][inner] == np.maximum(nodes["hi"][a], nodes["hi"][b])).all()
    return r


def moved(draws, seed, radius):
    """every transform of `draws` redrawn (shadow_ref.fuzz_scene's distributions); meshIndex and postPass stay"""
    rng = np.random.default_rng(seed)
    d = draws.copy()
    n = len(d)
    q = rng.normal(size=(n, 4))
    d["orientation"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    d["scale"] = np.exp(rng.uniform(np.log(0.25), np.log(8.0), n)).astype(np.float32)
    d["position"] = rng.uniform(-radius, radius, (n, 3)).astype(np.float32)
    return d


def mixed_draws(n, seed, mesh_count=2, radius=40.0, empty_mesh=None):
    """n random draws mixed with everything that can go wrong: duplicate transforms (equal keys), two far clusters, the singular quaternion
    (the infinite box), the zero quaternion, and draws that do not cast — NaN position, scale 0, postPass 2, meshIndex >= meshCount, a mesh without triangles"""
    rng = np.random.default_rng(seed)
    d = np.zeros(n, L.MESHDRAW)
    d = moved(d, seed + 1, radius)
    d["meshIndex"] = rng.integers(0, mesh_count, n)
    d["postPass"] = rng.integers(0, 2, n)
    if n >= 8:
        far = rng.random(n) < 0.3
        d["position"][far, 0] += np.float32(5.0e4)
        dup = rng.random(n) < 0.2
        for f in ("position", "scale", "orientation", "meshIndex"):
            d[f][dup] = d[f][np.flatnonzero(dup)[0]] if dup.any() else d[f][dup]
        kinds = rng.integers(0, 12, n)
        d["position"][kinds == 0, 1] = np.nan
        d["scale"][kinds == 1] = 0.0
        d["postPass"][kinds == 2] = 2
        d["meshIndex"][kinds == 3] = mesh_count + 3
        if empty_mesh is not None:
            d["meshIndex"][kinds == 4] = empty_mesh
        d["orientation"][np.flatnonzero(kinds == 5)[:2]] = (np.sqrt(0.5), 0.0, 0.0, 0.0)  # w = 0, |xyz|^2 = 1/2: the singular map
        d["orientation"][np.flatnonzero(kinds == 6)[:2]] = 0.0                           # the zero quaternion: the identity map
    return d


def with_empty_mesh(scene):
    """the scene with one more mesh that has no triangles (its index is len(meshes) - 1)"""
    meshes = np.concatenate([scene["meshes"], scene["meshes"][:1]])
    meshes["lods"]["indexCount"][-1] = 0
    return dict(scene, meshes=meshes)
