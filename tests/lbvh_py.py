"""Test-side restatement of the device BVH build (csrc/device/lbvh.h, build_bvh_device in render.hip),
in numpy, so that the tree a context builds under NART_BVH_BUILD=device can be compared bit for bit:
the build is deterministic (correctly rounded float32 division, nothing contracted, stable radix
sorts, boxes from min / max only).

The hierarchy is where this differs from the kernels on purpose.  k_lbvh_karras finds every inner
node's range and split with per-node binary searches over common-prefix lengths; here the leaf keys
are made the distinct 64-bit values key << 32 | leaf index, and each range is split top-down at its
highest differing bit, level by level.  Inner nodes are numbered by Karras's convention (root 0; a
node covering [first, last] split after g has the left child g and the right child g + 1, a child
being a leaf when its range is one leaf), so both must produce the same children.  Boxes are range
minima / maxima (the kernels merge bottom-up through a flag per node); the breadth-first order is a
stable sort of the inner nodes by depth.

Word 14 of the triangle records (the reference octree's leaf and inside bit) cannot be restated
without restating the reference octree: build() takes it per scene triangle as an input, and the
tests take it from the host build's records (nart_amd.bvh_dump), which carry it per triangle id.

Vectorised: no Python loop over triangles or nodes, one over the tree's levels.
"""
import numpy as np

import bvh_check

f32 = np.float32
LEAF = 4  # LBVH_LEAF


def spread10(q):
    """10 bits -> every third bit, bit by bit."""
    q = q.astype(np.uint32)
    out = np.zeros_like(q)
    for b in range(10):
        out |= ((q >> np.uint32(b)) & np.uint32(1)) << np.uint32(3 * b)
    return out


def morton_codes(c):
    """30-bit Morton codes of the centroids c (m, 3) over their own bounds (k_lbvh_bounds,
    k_lbvh_morton): (c - lo) / ext * 1024 in float32, clamped to [0, 1023] and truncated; 0.5 on an
    axis whose extent is not > 0 (cell 512).  x takes the highest bit of each triple."""
    lo, hi = c.min(axis=0), c.max(axis=0)
    ext = (hi - lo).astype(f32)
    with np.errstate(all="ignore"):
        u = ((c - lo).astype(f32) / ext).astype(f32)
    u = np.where(ext > 0, u, f32(0.5)).astype(f32)
    s = (u * f32(1024)).astype(f32)
    q = np.minimum(np.maximum(s, f32(0)), f32(1023)).astype(np.uint32)
    return (spread10(q[:, 0]) << np.uint32(2)) | (spread10(q[:, 1]) << np.uint32(1)) | spread10(q[:, 2])


def hierarchy(lkey):
    """The radix tree over the n >= 2 leaf keys, top-down.  Returns (child, depth, first, last): child
    (n - 1, 2) int64 in Karras numbering with leaves as ~leaf index, the depth of every inner node
    (root 0) and the leaf range [first, last] (n - 1, 2) each child covers."""
    n = len(lkey)
    K = (lkey.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    assert np.all(K[1:] > K[:-1])
    child = np.zeros((n - 1, 2), np.int64)
    depth = np.zeros(n - 1, np.int64)
    cfirst, clast = np.zeros((n - 1, 2), np.int64), np.zeros((n - 1, 2), np.int64)
    node, first, last = np.array([0]), np.array([0]), np.array([n - 1])
    level = 0
    while len(node):
        x = K[first] ^ K[last]
        for s in (1, 2, 4, 8, 16, 32):  # every bit at and below the highest differing one
            x |= x >> np.uint64(s)
        # the first key of the range with that bit set: the keys below it in the range have it clear
        split = K[last] & ~(x >> np.uint64(1))
        g = np.searchsorted(K, split, side="left").astype(np.int64) - 1
        assert np.all((g >= first) & (g < last))
        lleaf, rleaf = g == first, g + 1 == last
        child[node, 0] = np.where(lleaf, ~g, g)
        child[node, 1] = np.where(rleaf, ~(g + 1), g + 1)
        depth[node] = level
        cfirst[node, 0], clast[node, 0], cfirst[node, 1], clast[node, 1] = first, g, g + 1, last
        node = np.concatenate([g[~lleaf], (g + 1)[~rleaf]])
        first, last = np.concatenate([first[~lleaf], (g + 1)[~rleaf]]), np.concatenate([g[~lleaf], last[~rleaf]])
        level += 1
    return child, depth, cfirst, clast


def build(tris, vis, pad, info):
    """The tree build_bvh_device makes of the scene triangles `tris` (Scene.triangles()) with the
    visible ids `vis` (ascending), boxes grown by `pad`, word 14 of triangle g = info[g].  A dict as
    nart_amd.bvh_dump returns it, plus "order" (the triangle id of every record) and "codes" (the
    sorted Morton codes)."""
    tris = np.ascontiguousarray(tris, f32)
    vis = np.asarray(vis, np.int64)
    assert np.all(np.diff(vis) > 0)
    pad = f32(pad)
    m = len(vis)
    out = {"on_device": True, "pad": pad, "num_leaf_tris": m}
    if m == 0:
        out.update(nodes=np.zeros(0, bvh_check.NODE_DTYPE), tri_isect=np.zeros((0, 16), f32), tri_perm=np.zeros((3, 0, 16), f32),
                   root_code=-1, stack_depth=2, num_nodes=0, order=vis, codes=np.zeros(0, np.uint32))
        return out
    lo, hi = bvh_check.tri_bounds(tris, vis)
    c = (f32(0.5) * (lo + hi).astype(f32)).astype(f32)
    codes = morton_codes(c)
    o = np.argsort(codes, kind="stable")
    codes, lo, hi, order = codes[o], lo[o], hi[o], vis[o]
    n = (m + LEAF - 1) // LEAF
    rec = bvh_check.tri_records(tris, order, np.asarray(info, np.uint32)[order])
    out.update(tri_isect=rec, tri_perm=bvh_check.permute_records(rec), order=order, codes=codes, num_nodes=n - 1)
    if n == 1:
        out.update(nodes=np.zeros(0, bvh_check.NODE_DTYPE), root_code=int(~(m - 1)), stack_depth=2)
        return out
    child, depth, first, last = hierarchy(codes[::LEAF])
    # breadth-first order: stable by depth; node r of the output is inner node bfs[r]
    bfs = np.argsort(depth, kind="stable")
    remap = np.empty(n - 1, np.int64)
    remap[bfs] = np.arange(n - 1)
    # subtree bounds of every child = bounds of its leaf range = of the records [4 first, min(m, 4 last + 4))
    a, b = first * LEAF, np.minimum(m, last * LEAF + LEAF)
    idx = np.stack([a, b], -1).reshape(-1)
    inf = np.full((1, 3), np.inf, f32)
    blo = np.minimum.reduceat(np.concatenate([lo, inf]), idx, axis=0)[0::2].reshape(n - 1, 2, 3)
    bhi = np.maximum.reduceat(np.concatenate([hi, -inf]), idx, axis=0)[0::2].reshape(n - 1, 2, 3)
    leaf_first = ~child * LEAF
    leaf_code = ~((leaf_first << 5) | (np.minimum(m, leaf_first + LEAF) - leaf_first - 1))
    code = np.where(child < 0, leaf_code, remap[np.maximum(child, 0)])
    nodes = np.zeros(n - 1, bvh_check.NODE_DTYPE)
    nodes["lo0"], nodes["hi0"] = (blo[bfs, 0] - pad).astype(f32), (bhi[bfs, 0] + pad).astype(f32)
    nodes["lo1"], nodes["hi1"] = (blo[bfs, 1] - pad).astype(f32), (bhi[bfs, 1] + pad).astype(f32)
    nodes["child"] = code[bfs].astype(np.int32)
    out.update(nodes=nodes, root_code=0, stack_depth=max(int(depth.max()) + 2, 2))
    return out
