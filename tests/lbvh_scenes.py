"""Seeded "triangle soup" scenes that drive the device BVH build (csrc/device/lbvh.h) to the sizes and
key distributions no shipped scene reaches (tests/test_lbvh_restatement.py, tests/test_gpu_lbvh.py).

A soup is N small tilted Lambert triangles with centres drawn in the box [-1, 1]^3, one disk light
above it and a camera looking at it, written through nart_amd.scenes.write_geo (the largest scene
through a vectorised writer of the same token stream, see write_soup_geo).

Which triangles the tree holds is decided by the replayed reference octree (host/bvh_build.cpp
reference_visibility): it drops the chunks a splitting leaf leaves behind, and a root that stays a
leaf makes nothing visible, so the visible count m is not N.  CASES below was found by searching N
and the seed with the host-only nart_amd.bvh_info (find() is that search); every test asserts the
property of m its case was chosen for (check_case), so a change of the octree replay or of the
generator that moves m is noticed instead of silently testing something else.

    m = visible triangles, n = ceil(m / 4) leaves, n - 1 inner nodes
"""
import json
import os

import numpy as np

import nart_amd
from nart_amd import scenes

f32 = np.float32

# Where the cluster option puts its ball.  The Morton cells of the [-8, 8] extent the outliers set are
# about 1/64 wide, so a ball of radius 1e-4 rarely straddles a cell face; the tests assert that it
# does not (the restatement's sorted codes must hold CLUSTER_MIN_EQUAL equal ones).
CLUSTER_CENTRE = (0.3 + 1.0 / 128, -0.2 + 1.0 / 128, 0.1 + 1.0 / 128)


def soup_triangles(n, seed, size=0.03, cluster=None, flat_axis=None):
    """(n, 3, 3) float32 vertices.  cluster=(K, r): the first K triangles lie within a ball of radius r
    around CLUSTER_CENTRE, and eight far outliers (the last eight triangles, near the corners of
    [-8, 8]^3) set the scene extent, so that all K centroids get one Morton code.  flat_axis=a: every
    triangle spans [-h, h] on axis a with its third vertex in between, so that every centroid (the
    middle of the bounds) is exactly 0 there while the triangles stay tilted and the scene keeps volume."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-1.0, 1.0, (n, 3))
    off = rng.uniform(-1.0, 1.0, (n, 3, 3)) * size
    if cluster is not None:
        k, r = cluster
        assert k + 8 <= n
        d = rng.normal(size=(k, 3))
        d *= (r * 0.5 * rng.uniform(0, 1, (k, 1)) ** (1 / 3)) / np.linalg.norm(d, axis=1, keepdims=True)
        centre[:k] = np.asarray(CLUSTER_CENTRE) + d
        off[:k] *= (r * 0.5) / (size * np.sqrt(3.0))
        corners = np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], np.float64)
        centre[n - 8:] = corners * 7.9
    v = centre[:, None, :] + off
    if flat_axis is not None:
        h = rng.uniform(0.2, 1.0, n) * size * 4
        t = rng.uniform(-0.9, 0.9, n)
        v[:, 0, flat_axis], v[:, 1, flat_axis], v[:, 2, flat_axis] = -h, h, t * h
    return v.astype(f32)


def write_soup_geo(path, v):
    """The token stream scenes.write_geo writes for triangles v (n, 3, 3) with one shared normal, built
    from whole arrays: n faces of 3 vertices, indices 0..3n-1, the vertices, normal index 0 for every
    corner, one normal."""
    n = len(v)
    idx = " ".join(map(str, range(3 * n)))
    flat = v.astype(f32).reshape(-1).astype(np.float64).tolist()
    floats = (" ".join(["%.9g"] * len(flat))) % tuple(flat)
    with open(path, "w") as f:
        f.write(" ".join([str(n), " ".join(["3"] * n), idx, floats, " ".join(["0"] * (3 * n)), "0 0 1"]) + "\n")


def soup(directory, n, seed, fast=False, **options):
    """Write the soup scene (soup.json + soup.geo) into `directory`; returns the JSON path."""
    os.makedirs(directory, exist_ok=True)
    v = soup_triangles(n, seed, **options)
    geo = os.path.join(directory, "soup.geo")
    if fast:
        write_soup_geo(geo, v)
    else:
        faces = [[3 * i, 3 * i + 1, 3 * i + 2] for i in range(n)]
        scenes.write_geo(geo, faces, [tuple(p) for p in v.reshape(-1, 3)], [(0.0, 0.0, 1.0)], [[0, 0, 0]] * n)
    scene = {
        "renderSessions": [{"imageWidth": 64, "imageHeight": 48, "bucketSize": 16, "spp": 2, "bounces": 4,
                            "filterWidth": 2, "rougheningFactor": 0}],
        "camera": {"fov": 22.0, "transform": [1, 0, 0, 0, 0, 0, -1, -6.5, 0, 1, 0, 0, 0, 0, 0, 1]},
        "meshes": [{"filePath": geo, "material": {"type": "lambert", "rho_d": [0.7, 0.6, 0.5]}}],
        "lights": [{"type": "disk", "radius": 0.8, "Le": [1, 1, 1], "intensity": 40.0,
                    "transform": [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 2.5, 0, 0, 0, 1]}],
    }
    path = os.path.join(directory, "soup.json")
    with open(path, "w") as f:
        json.dump(scene, f, indent=1)
    return path


def find(accept, n_values, seeds, directory, **options):
    """The search behind CASES: the first (N, seed) whose visible count m (host only, bvh_info)
    satisfies accept(m); None if there is none."""
    for n in n_values:
        for seed in seeds:
            sc = nart_amd.Scene(soup(directory, n, seed, fast=True, **options))
            m = nart_amd.bvh_info(sc)["num_leaf_tris"]
            sc.close()
            if accept(m):
                return n, seed, m
    return None


def _leaves(m):
    return (m + 3) // 4


def _equal_codes(k):
    return {"cluster": (k, 1e-4)}


# case -> (N, seed, options, the property of m the case exists for).  Random soups this sparse lose
# few chunks to the octree, so every exact target was reachable.
CASES = {
    "empty": (1, 1, {}, lambda m: m == 0),                                    # one chunk: the root stays a leaf
    "one_leaf": (3, 1, {}, lambda m: 1 <= m <= 4),
    "two_leaves_short": (5, 1, {}, lambda m: m == 5),                         # last leaf of one triangle
    "two_leaves": (8, 1, {}, lambda m: _leaves(m) == 2 and m % 4 == 0),
    "three_leaves": (12, 1, {}, lambda m: _leaves(m) == 3 and m % 4 == 0),
    "three_leaves_short": (10, 1, {}, lambda m: _leaves(m) == 3 and m % 4 != 0),
    "inner_255": (1024, 1, {}, lambda m: _leaves(m) - 1 == 255),
    "inner_256": (1025, 1, {}, lambda m: _leaves(m) - 1 == 256),
    "inner_257": (1030, 1, {}, lambda m: _leaves(m) - 1 == 257),
    "tris_256k": (768, 1, {}, lambda m: m > 256 and m % 256 == 0),
    "tris_256k_1": (769, 1, {}, lambda m: m > 256 and m % 256 == 1),
    "medium": (20000, 1, {}, lambda m: 16000 <= m <= 32000),
    "cluster": (22000, 1, _equal_codes(2100), lambda m: 16000 <= m <= 32000),  # + check_equal_codes
    "flat_axis": (20000, 1, {"flat_axis": 1}, lambda m: 16000 <= m <= 32000),  # + check_flat_axis
    "large": (262145, 0, {}, lambda m: 262144 < m <= 262144 + 64),             # k_lbvh_bounds' second trip
}
SMALL = [c for c in CASES if c != "large"]
CLUSTER_MIN_EQUAL = 2048


def check_case(name, m):
    """Assert that case `name` still has the property it was chosen for."""
    n_tris, seed, options, prop = CASES[name]
    assert prop(m), "lbvh scene %r (N=%d, seed=%d, %r) no longer has its property: m = %d, leaves = %d" % (
        name, n_tris, seed, options, m, _leaves(m))


def case_scene(name, directory):
    n_tris, seed, options, _ = CASES[name]
    return nart_amd.Scene(soup(directory, n_tris, seed, fast=n_tris > 4096, **options))


_PREPARED = {}


def prepared(name, directory):
    """Everything the tests of one case share, computed once per process: the scene, its triangle
    array, the host SAH dump (nart_amd.bvh_dump), the visible ids (ascending) and word 14 per scene
    triangle taken from that dump, and the restatement of the device build (tests/lbvh_py.py) for
    them.  Nobody changes these arrays."""
    if name not in _PREPARED:
        import lbvh_py
        sc = case_scene(name, os.path.join(directory, name))
        tris = sc.triangles()
        host = nart_amd.bvh_dump(sc)
        check_case(name, host["num_leaf_tris"])
        words = host["tri_isect"].view(np.uint32)
        ids = words[:, 13].astype(np.int64)
        info = np.zeros(len(tris), np.uint32)
        info[ids] = words[:, 14]
        vis = np.unique(ids)
        restated = lbvh_py.build(tris, vis, host["pad"], info)
        _PREPARED[name] = {"scene": sc, "tris": tris, "host": host, "vis": vis, "info": info, "restated": restated}
    return _PREPARED[name]


def expected_ids(name, prep):
    """The ids the tree must hold, from outside the dump where that is possible: when the octree drops
    nothing (m = N) they are all of the scene's triangles; otherwise the dump's own distinct ids (the
    validator then still demands each exactly once)."""
    n_tris = len(prep["tris"])
    return np.arange(n_tris) if prep["host"]["num_leaf_tris"] == n_tris else prep["vis"]


def check_equal_codes(prep):
    """The cluster case's second property: at least CLUSTER_MIN_EQUAL triangles share one Morton code."""
    _, counts = np.unique(prep["restated"]["codes"], return_counts=True)
    assert counts.max() >= CLUSTER_MIN_EQUAL, counts.max()


def check_flat_axis(prep, axis=1):
    """The flat-axis case's second property: every visible centroid has the same coordinate there."""
    t = prep["tris"][prep["vis"]][:, :9].reshape(-1, 3, 3)[:, :, axis]
    c = f32(0.5) * (t.min(axis=1) + t.max(axis=1))
    assert np.all(c == c[0]) and t.max() > t.min()
