"""Validator for a BVH in the render path's node format (csrc/device/dscene.h BVHNode, the triangle
test records of host/bvh_build.cpp build_bvh and their per-axis permutation), whichever builder made
it: the host's binned SAH or the device's linear BVH (csrc/device/lbvh.h).  Plain numpy on a dump
(nart_amd.bvh_dump / HipRenderer.bvh_dump, or tests/lbvh_py.py's restatement); nothing here calls
into the library.

check(dump, tris, expected_ids) raises BvhInvalid, whose message starts with the name of the
invariant that failed:

    reachability         every node index in [0, num_nodes) is reached from the root exactly once
    leaf ranges          counts in [1, LEAF_MAX]; the ranges [first, first + count) tile [0, num_leaf_tris)
    triangle ids         word 13 of the records is exactly the expected id set, each id once
    child box            every child box contains the float32 bounds of its subtree's triangles grown
                         by pad (exact=True: equals them bit for bit)
    breadth-first order  an inner child's index exceeds its parent's; depth never decreases along the array
    stack depth          stack_depth >= inner levels on the deepest root-to-leaf path + 1
    record               words 0-12 and 15 are build_bvh's formulas for the triangle named in word 13
    permuted record      every per-axis record is nart_hip_create's permutation of its record

Leaf codes are decoded as the traversal decodes them: ~code = first << 5 | (count - 1).
"""
import numpy as np

f32 = np.float32
LEAF_MAX = 32  # NART_LEAF_MAX (csrc/device/dscene.h)
# BVHNode (csrc/device/dscene.h), as the dumps hold it (nart_amd.api.BVH_NODE_DTYPE)
NODE_DTYPE = np.dtype([("lo0", f32, 3), ("hi0", f32, 3), ("lo1", f32, 3), ("hi1", f32, 3), ("child", np.int32, 2),
                       ("pad", np.int32, 2)])


class BvhInvalid(AssertionError):
    def __init__(self, invariant, detail):
        super().__init__("%s: %s" % (invariant, detail))
        self.invariant = invariant


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def tri_records(tris, ids, word14):
    """build_bvh's test records (host/bvh_build.cpp) for the scene triangles `ids`, in that order:
    n = cross(v1 - v0, v2 - v0), dot(v0, n), the vertices, the id, word 14 as given (uint32 per
    record) and |n| / 8 -- every product, sum and root one float32 operation in the source's order."""
    ids = np.asarray(ids, np.int64)
    t = np.ascontiguousarray(tris, f32)[ids]
    v0, v1, v2 = t[:, 0:3], t[:, 3:6], t[:, 6:9]
    e1, e2 = (v1 - v0).astype(f32), (v2 - v0).astype(f32)
    n = np.empty((len(ids), 3), f32)
    n[:, 0] = e1[:, 1] * e2[:, 2] - e2[:, 1] * e1[:, 2]
    n[:, 1] = e1[:, 2] * e2[:, 0] - e2[:, 2] * e1[:, 0]
    n[:, 2] = e1[:, 0] * e2[:, 1] - e2[:, 0] * e1[:, 1]
    rec = np.zeros((len(ids), 16), f32)
    rec[:, 0:3] = n
    rec[:, 3] = (v0[:, 0] * n[:, 0] + v0[:, 1] * n[:, 1]) + v0[:, 2] * n[:, 2]
    rec[:, 4:13] = t[:, 0:9]
    rec[:, 15] = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]) * f32(0.125)
    u = rec.view(np.uint32)
    u[:, 13] = ids.astype(np.uint32)
    u[:, 14] = np.asarray(word14, np.uint32)
    return rec


def permute_records(rec):
    """nart_hip_create's permuted records: for ray major axis m the vertices as (kx, ky, kz) =
    (m + 1, m + 2, m) mod 3, then words 13, 14, 15, then the plane (words 0-3).  (3, nt, 16)."""
    rec = np.ascontiguousarray(rec, f32)
    out = np.zeros((3,) + rec.shape, f32)
    for m in range(3):
        ax = [(m + 1) % 3, (m + 2) % 3, m]
        for k in range(3):
            out[m][:, 3 * k:3 * k + 3] = rec[:, 4 + 3 * k:7 + 3 * k][:, ax]
        out[m][:, 9:12] = rec[:, 13:16]
        out[m][:, 12:16] = rec[:, 0:4]
    return out


def tri_bounds(tris, ids):
    """float32 (lo, hi) of the scene triangles `ids`, (len, 3) each."""
    t = np.ascontiguousarray(tris, f32)[np.asarray(ids, np.int64)][:, :9].reshape(-1, 3, 3)
    return t.min(axis=1), t.max(axis=1)


def walk(dump):
    """Breadth-first walk from the root.  Returns (depth per node, leaves) with leaves a dict of arrays
    over every leaf child: first, count, parent (-1: the root is the leaf), side, level (inner nodes
    above it); checks `reachability` on the way (so that the walk ends on any input)."""
    nodes, nn, root = dump["nodes"], int(dump["num_nodes"]), int(dump["root_code"])
    if len(nodes) != nn:
        raise BvhInvalid("reachability", "%d node records for num_nodes = %d" % (len(nodes), nn))
    leaf = {"code": [], "parent": [], "side": [], "level": []}
    depth = np.full(nn, -1, np.int64)
    if root < 0:
        if nn:
            raise BvhInvalid("reachability", "the root is a leaf but there are %d nodes nothing points to" % nn)
        leaf = {"code": [np.array([root])], "parent": [np.array([-1])], "side": [np.array([0])],
                "level": [np.array([0])]}
    else:
        if root >= nn:
            raise BvhInvalid("reachability", "root %d outside [0, %d)" % (root, nn))
        visits = np.zeros(nn, np.int64)
        frontier = np.array([root], np.int64)
        visits[root] = 1
        level = 0
        while len(frontier):
            depth[frontier] = level
            c = nodes["child"][frontier].astype(np.int64)  # (k, 2)
            par = np.repeat(frontier, 2)
            side = np.tile(np.array([0, 1]), len(frontier))
            c = c.reshape(-1)
            inner = c >= 0
            if np.any(c[inner] >= nn):
                bad = par[inner][c[inner] >= nn][0]
                raise BvhInvalid("reachability", "node %d has a child index outside [0, %d)" % (bad, nn))
            np.add.at(visits, c[inner], 1)
            if np.any(visits > 1):
                raise BvhInvalid("reachability", "node %d is reached more than once (shared child or cycle)"
                                 % int(np.nonzero(visits > 1)[0][0]))
            leaf["code"].append(c[~inner])
            leaf["parent"].append(par[~inner])
            leaf["side"].append(side[~inner])
            leaf["level"].append(np.full(int((~inner).sum()), level + 1))
            frontier = c[inner]
            level += 1
        if np.any(visits == 0):
            raise BvhInvalid("reachability", "node %d is never reached from the root (orphan)"
                             % int(np.nonzero(visits == 0)[0][0]))
    leaf = {k: np.concatenate(v).astype(np.int64) for k, v in leaf.items()}
    code = ~leaf["code"]
    leaf["first"], leaf["count"] = code >> 5, (code & 31) + 1
    return depth, leaf


def check(dump, tris, expected_ids, exact=False):
    """Assert every invariant of the module docstring on `dump` (a dict as nart_amd.bvh_dump returns
    it) for the scene triangle array `tris` (Scene.triangles()) and the ids expected in leaves.
    exact=True additionally demands that every child box equals its subtree's padded bounds."""
    nodes, rec, perm = dump["nodes"], np.ascontiguousarray(dump["tri_isect"], f32), dump["tri_perm"]
    nt, nn = int(dump["num_leaf_tris"]), int(dump["num_nodes"])
    pad = f32(dump["pad"])
    expected = np.sort(np.asarray(expected_ids, np.int64))
    if rec.shape != (nt, 16) or tuple(np.shape(perm)) != (3, nt, 16):
        raise BvhInvalid("leaf ranges", "record arrays of shape %s / %s for num_leaf_tris = %d"
                         % (rec.shape, np.shape(perm), nt))
    if nt == 0:  # the empty tree: never traversed
        if nn or int(dump["root_code"]) >= 0:
            raise BvhInvalid("reachability", "an empty tree with %d nodes and root %d" % (nn, dump["root_code"]))
        if len(expected):
            raise BvhInvalid("triangle ids", "%d triangles expected, none in the tree" % len(expected))
        return

    # 1. reachability
    depth, leaf = walk(dump)

    # 2. leaf ranges
    if np.any(leaf["count"] < 1) or np.any(leaf["count"] > LEAF_MAX):
        raise BvhInvalid("leaf ranges", "a leaf count outside [1, %d]" % LEAF_MAX)
    o = np.argsort(leaf["first"], kind="stable")
    first, count = leaf["first"][o], leaf["count"][o]
    ends = first + count
    if first[0] != 0 or ends[-1] != nt or np.any(first[1:] != ends[:-1]):
        i = 0 if first[0] != 0 else (int(np.nonzero(first[1:] != ends[:-1])[0][0]) + 1 if np.any(first[1:] != ends[:-1])
                                     else len(first) - 1)
        raise BvhInvalid("leaf ranges", "the leaf ranges do not tile [0, %d): gap or overlap at the leaf starting at "
                         "record %d (the ranges before it end at %d)" % (nt, first[i], ends[i - 1] if i else 0))

    # 3. triangle ids
    ids = rec.view(np.uint32)[:, 13].astype(np.int64)
    if len(ids) != len(expected) or not np.array_equal(np.sort(ids), expected):
        u, c = np.unique(ids, return_counts=True)
        raise BvhInvalid("triangle ids", "the records name %d ids (%d distinct, %d more than once), expected %d; "
                         "missing %s, unexpected %s" % (len(ids), len(u), int((c > 1).sum()), len(expected),
                                                         np.setdiff1d(expected, u)[:4], np.setdiff1d(u, expected)[:4]))

    # 4. child boxes: bounds of the leaves' record ranges, then bottom-up over the levels
    tlo, thi = tri_bounds(tris, ids)
    starts = leaf["first"]
    # reduceat over [first, first + count): pairs of indices, the odd results are discarded
    idx = np.stack([starts, starts + leaf["count"]], 1).reshape(-1)
    sentinel = np.zeros((1, 3), f32)
    llo = np.minimum.reduceat(np.concatenate([tlo, sentinel + np.inf]), idx, axis=0)[0::2]
    lhi = np.maximum.reduceat(np.concatenate([thi, sentinel - np.inf]), idx, axis=0)[0::2]
    if nn:
        clo = np.full((nn, 2, 3), np.inf, f32)   # subtree bounds of each child of each node
        chi = np.full((nn, 2, 3), -np.inf, f32)
        clo[leaf["parent"], leaf["side"]] = llo
        chi[leaf["parent"], leaf["side"]] = lhi
        child = nodes["child"].astype(np.int64)
        for lv in range(int(depth.max()), -1, -1):  # children are one level deeper: already complete
            at = np.nonzero(depth == lv)[0]
            for s in range(2):
                sel = at[child[at, s] >= 0]
                k = child[sel, s]
                clo[sel, s] = np.minimum(clo[k, 0], clo[k, 1])
                chi[sel, s] = np.maximum(chi[k, 0], chi[k, 1])
        want_lo, want_hi = (clo - pad).astype(f32), (chi + pad).astype(f32)
        box_lo = np.stack([nodes["lo0"], nodes["lo1"]], 1)
        box_hi = np.stack([nodes["hi0"], nodes["hi1"]], 1)
        bad = ~((box_lo <= want_lo) & (box_hi >= want_hi))
        if np.any(bad):
            i, s, a = (int(x[0]) for x in np.nonzero(bad))
            raise BvhInvalid("child box", "child %d of node %d does not contain its triangles on axis %d: box "
                             "[%.9g, %.9g], padded bounds [%.9g, %.9g]"
                             % (s, i, a, box_lo[i, s, a], box_hi[i, s, a], want_lo[i, s, a], want_hi[i, s, a]))
        if exact:
            bad = (_bits(box_lo) != _bits(want_lo)) | (_bits(box_hi) != _bits(want_hi))
            if np.any(bad):
                i, s, a = (int(x[0]) for x in np.nonzero(bad))
                raise BvhInvalid("child box", "child %d of node %d is not exactly its padded bounds on axis %d: box "
                                 "[%.9g, %.9g], padded bounds [%.9g, %.9g]"
                                 % (s, i, a, box_lo[i, s, a], box_hi[i, s, a], want_lo[i, s, a], want_hi[i, s, a]))

        # 5. breadth-first order
        up = (child >= 0) & (child <= np.arange(nn)[:, None])
        if np.any(up):
            raise BvhInvalid("breadth-first order", "node %d has an inner child with an index not above its own"
                             % int(np.nonzero(up.any(axis=1))[0][0]))
        if np.any(np.diff(depth) < 0):
            i = int(np.nonzero(np.diff(depth) < 0)[0][0])
            raise BvhInvalid("breadth-first order", "depth decreases along the array: node %d at depth %d, node %d at "
                             "depth %d" % (i, depth[i], i + 1, depth[i + 1]))

    # 6. stack depth
    levels = int(leaf["level"].max())
    if int(dump["stack_depth"]) < levels + 1:
        raise BvhInvalid("stack depth", "stack_depth %d for %d inner levels on the deepest path (needs %d)"
                         % (dump["stack_depth"], levels, levels + 1))

    # 7. records
    want = tri_records(tris, ids, rec.view(np.uint32)[:, 14])
    bad = _bits(rec) != _bits(want)
    if np.any(bad):
        i, w = (int(x[0]) for x in np.nonzero(bad))
        raise BvhInvalid("record", "record %d (triangle %d) word %d is %.9g (0x%08x), the host formula gives %.9g "
                         "(0x%08x)" % (i, ids[i], w, rec[i, w], _bits(rec)[i, w], want[i, w], _bits(want)[i, w]))
    bad = _bits(perm) != _bits(permute_records(rec))
    if np.any(bad):
        m, i, w = (int(x[0]) for x in np.nonzero(bad))
        raise BvhInvalid("permuted record", "axis %d record %d word %d is not the permutation of its record" % (m, i, w))
