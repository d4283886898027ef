"""Scenes and ray sets of the device trace probe (HipRenderer.trace / oracle.trace_n): deterministic, no GPU.

The traversal (path.h trav_step, traverse_packet) followed by octree.h oc_resolve must return exactly
the hit the reference's Octree::Intersect returns.  Renders hand it only camera rays from one origin and
secondary rays with directions from continuous distributions; the sets here are the rays a render never
casts.  Each set is designed for one class of trouble and then filled from a seed; tests/test_trace_cases.py
shows on the CPU, with the oracle alone, that every class is populated in every scene that can produce it.

Scenes (small: the oracle's brute force over all triangles per ray stays in seconds):
    lattice      layers of axis-aligned unit quads at integer and power-of-two coordinates (exact
                 arithmetic: coplanar neighbours tie bit for bit, chunk boxes are flat, origins sit exactly on
                 box faces) plus a tilted sheet z = x + 8 with integer vertices.  In-plane rays give NaN
                 plane distances here, but the exact arithmetic also makes their edge functions exactly
                 zero, so Triangle::Intersect rejects them: NaNs that pass come from the other scenes
    inner_256    lbvh_scenes' soup around the 256-inner-node boundary
    cluster      a soup with 2100 triangles in one Morton cell: a deep tree, so short stacks spill
    glassSphere  the shipped scene (shared edges and vertices on a curved mesh)
    empty        the root stays a leaf: nothing is visible
    one_leaf     one BVH leaf
"""
import json
import os

import numpy as np

import nart_amd
from nart_amd import scenes

import lbvh_scenes

f32 = np.float32
SEED = 20240611
SCENES = ("lattice", "inner_256", "cluster", "glassSphere", "empty", "one_leaf")
CLUSTER = (4096, 1, {"cluster": (2100, 1e-4)})  # N, seed, options of lbvh_scenes.soup
BUILDERS = ("host", "device")  # the host SAH tree and the device LBVH (NART_BVH_BUILD=device): every scene on both
SCALES = (1e-3, 1.0, 1e3)  # the reference does not normalise the directions it traces (cast_ray normalises its own)
# direction components around zero: signed zeros, denormals, and either side of the reciprocal clamp at 1e20
SPECIALS = (0.0, -0.0, 1e-45, -1e-40, 1e-30, -1e-30, 1e-25, -1e-25)
FLT_MIN = float(np.finfo(f32).tiny)
TMAX_EDGES = ("zero", "min_normal", "below", "at", "above", "inf")


# ------------------------------------------------------------------------------------------------ scenes
def lattice_triangles():
    """(n, 3, 3) float32 vertices and the mesh (0 flat layers, 1 tilted sheet) of every triangle."""
    tris, mesh = [], []

    def quad(p, u, v, m):
        p, u, v = (np.asarray(a, np.float64) for a in (p, u, v))
        tris.append([p, p + u, p + u + v])
        tris.append([p, p + u + v, p + v])
        mesh.extend([m, m])

    for z in (-2.0, -0.5, 0.25, 1.0):  # horizontal layers, unit cells over [-4, 4]^2
        for i in range(-4, 4):
            for j in range(-4, 4):
                quad((i, j, z), (1, 0, 0), (0, 1, 0), 0)
    for i in range(-4, 4):  # a wall y = 4 over z in [-2, 2]
        for k in range(-2, 2):
            quad((i, 4, k), (1, 0, 0), (0, 0, 1), 0)
    for i in range(-4, 4):  # the tilted sheet z = x + 8
        for j in range(-4, 4):
            quad((i, j, 8 + i), (1, 0, 1), (0, 1, 0), 1)
    return np.asarray(tris, f32), np.asarray(mesh)


def lattice(directory):
    os.makedirs(directory, exist_ok=True)
    v, mesh = lattice_triangles()
    meshes = []
    for m, rho in ((0, [0.7, 0.6, 0.5]), (1, [0.2, 0.5, 0.8])):
        t = v[mesh == m]
        n = len(t)
        verts = [tuple(p) for p in t.reshape(-1, 3)]
        faces = [[3 * i, 3 * i + 1, 3 * i + 2] for i in range(n)]
        uvs = [((p[0] + 0.25 * p[2] + 8) / 16.0, (p[1] + 0.5 * p[2] + 8) / 16.0) for p in verts]
        geo = os.path.join(directory, "lattice%d.geo" % m)
        scenes.write_geo(geo, faces, verts, [(0.0, 0.0, 1.0)], [[0, 0, 0]] * n, uvs, faces)
        meshes.append({"filePath": geo, "material": {"type": "lambert", "rho_d": rho}})
    scene = {
        "renderSessions": [{"imageWidth": 64, "imageHeight": 48, "bucketSize": 16, "spp": 2, "bounces": 4,
                            "filterWidth": 2, "rougheningFactor": 0}],
        "camera": {"fov": 40.0, "transform": [1, 0, 0, 0, 0, 0, -1, -30, 0, 1, 0, 0, 0, 0, 0, 1]},
        "meshes": meshes,
        "lights": [{"type": "disk", "radius": 0.8, "Le": [1, 1, 1], "intensity": 40.0,
                    "transform": [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 20, 0, 0, 0, 1]}],
    }
    path = os.path.join(directory, "lattice.json")
    with open(path, "w") as f:
        json.dump(scene, f, indent=1)
    return path


def scene(name, directory):
    d = os.path.join(directory, name)
    if name == "lattice":
        return nart_amd.Scene(lattice(d))
    if name == "glassSphere":
        return nart_amd.Scene(scenes.glass_sphere(d))
    if name == "cluster":
        n, seed, options = CLUSTER
        return nart_amd.Scene(lbvh_scenes.soup(d, n, seed, fast=True, **options))
    return lbvh_scenes.case_scene(name, d)


# ------------------------------------------------------------------------------------------------ float32 pieces
def _dot(a, b):  # GLM's dot(vec3) order, float32
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2],
                     a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0],
                     a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], axis=-1)


def plane_terms(T, o, d):
    """Numerator and denominator of Triangle::Intersect's plane distance (geometry.cpp:34-36), float32."""
    v0 = T[:, 0]
    n = _cross(T[:, 1] - v0, T[:, 2] - v0)
    return _dot(v0, n) - _dot(o, n), _dot(d, n)


def ulp_step(t, k):
    """t moved k float32 steps (positive finite t)."""
    return (np.asarray(t, f32).view(np.uint32).astype(np.int64) + k).astype(np.uint32).view(f32)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


# ------------------------------------------------------------------------------------------------ ray sets
FAR = 32.0      # far origins, in units of the scene's largest coordinate (below)
BEYOND = 1e4    # ... and far beyond what the device's boxes are padded for: measured, not asserted


def scene_maxabs(sc, T):
    """The scene's largest coordinate magnitude, camera position included, at least 1 (render.hip
    scene_maxabs): the scale of the BVH2's box padding."""
    _, m = sc.camera()
    return max(1.0, float(np.abs(T).max()), abs(float(m[3])), abs(float(m[7])), abs(float(m[11])))


def designed(name, T, maxabs):
    """The ray sets that need no oracle: {class: (n, 8) float32 records}.  T: (m, 3, 3) float32 scene
    triangles (m >= 1).

    Far origins.  The BVH2 slab test computes a box's distances as fma(bound, 1 / d, -o / d): about four
    float32 roundings between an entry and an exit distance, each of the size of an ulp of |o / d|, i.e.
    4 * 2^-23 |o| in space.  The boxes are padded by 2^-14 of the scene's largest coordinate, camera
    included (render.hip), so the test is exact up to |o| = 2^7 times that; every ray of a render starts
    within 1 times it.  The far set starts at FAR = 32 of these units (a quarter of the limit).  The
    "beyond" set, at BEYOND scene radii, is outside what the padding covers: the tests run it and print
    how many rays differ, and assert nothing about the oracle there."""
    rng = np.random.default_rng([SEED, SCENES.index(name)])
    # the part of the scene the rays aim at (the cluster soup's eight outliers set its extent, not its bulk)
    lo, hi = np.percentile(T.reshape(-1, 3), 1, axis=0), np.percentile(T.reshape(-1, 3), 99, axis=0)
    centre, radius = 0.5 * (lo + hi), max(0.5 * float(np.linalg.norm(hi - lo)), 1e-3)
    grid = name == "lattice"  # origins on integer coordinates: o, d and the target are exact

    def interior(n):
        k = rng.integers(0, len(T), n)
        b = rng.dirichlet((1.0, 1.0, 1.0), n)
        if grid:  # quarter-point barycentrics: exact
            b = np.asarray([(0.5, 0.25, 0.25), (0.25, 0.5, 0.25), (0.25, 0.25, 0.5)])[rng.integers(0, 3, n)]
        return k, np.einsum("nj,njc->nc", b, T[k].astype(np.float64))

    def outside(n, r=3.0):
        o = centre + _unit(rng, n) * radius * r
        return np.round(o) if grid else o

    def rec(o, d, tmax=np.inf, kind=nart_amd.TRACE_CLOSEST):
        return nart_amd.trace_rays(np.asarray(o, np.float64).astype(f32), np.asarray(d, np.float64).astype(f32), tmax, kind)

    def through(p, o, scale=None):
        o32 = np.asarray(o, np.float64).astype(f32)
        d = (np.asarray(p, np.float64).astype(f32) - o32).astype(np.float64)  # one float32 subtraction: o + d = p
        return rec(o32, d if scale is None else d * scale)

    sets = {}
    n = 1536
    _, p = interior(n)
    sets["interior"] = through(p, outside(n), np.asarray(SCALES)[np.arange(n) % 3][:, None])
    k = rng.integers(0, len(T), n)
    sets["vertex"] = through(T[k, rng.integers(0, 3, n)], outside(n))
    k, j = rng.integers(0, len(T), n), rng.integers(0, 3, n)
    mid = 0.5 * (T[k, j].astype(np.float64) + T[k, (j + 1) % 3].astype(np.float64))
    sets["edge"] = through(mid, outside(n))
    if grid:  # straight down the shared edges of coplanar neighbours: exact ties, hits on flat box faces
        o = mid.copy()
        axis = rng.integers(0, 3, n)
        o[np.arange(n), axis] += np.where(rng.integers(0, 2, n) == 1, 16.0, -16.0)
        sets["edge_axis"] = through(mid, o)

    # directions with one or two components at or around zero, through interior points
    pat = [(a,) for a in range(3)] + [(0, 1), (0, 2), (1, 2)]
    rows = [(pp, s) for pp in pat for s in SPECIALS]
    reps = 16
    _, p = interior(len(rows) * reps)
    d = _unit(rng, len(p))
    for i, (pp, s) in enumerate(rows * reps):
        d[i, list(pp)] = s
    d32 = d.astype(f32)
    o = p - np.where(np.abs(d32) < 1e-20, 0.0, d32.astype(np.float64)) * (3.0 * radius)
    sets["direction"] = rec(o, d32)

    n = 512
    k, p = interior(n)
    sets["origin_on_triangle"] = rec(p, _unit(rng, n))
    k = rng.integers(0, len(T), n)
    sets["origin_on_vertex"] = rec(T[k, rng.integers(0, 3, n)], _unit(rng, n))
    _, p = interior(n)
    sets["origin_inside"] = rec(p + _unit(rng, n) * radius * 1e-3 * (0 if grid else 1) +
                                (np.asarray([0.0, 0.0, 0.125]) if grid else 0.0), _unit(rng, n))
    _, p = interior(n)
    sets["far"] = through(p, centre + _unit(rng, n) * FAR * maxabs)
    _, p = interior(n)
    sets["beyond"] = through(p, centre + _unit(rng, n) * radius * BEYOND)
    o = outside(n)
    sets["miss"] = rec(o, (o - centre) + _unit(rng, n) * 0.3 * radius)
    if grid:  # origins exactly on layer planes and cell boundaries (faces of the flat chunk boxes)
        o = np.stack([rng.integers(-4, 5, n), rng.integers(-4, 5, n), rng.choice([-2.0, -0.5, 0.25, 1.0], n)], axis=1)
        d = _unit(rng, n)
        d[: n // 2] = np.round(d[: n // 2] * 2.0) / 2.0  # half of them on the coarse directions
        d[np.all(d == 0, axis=1)] = (0.0, 0.0, 1.0)
        sets["origin_on_face"] = rec(o, d)

    # NaN plane distances: the origin on the triangle's plane and inside its bounds, the direction in the
    # plane, both exactly so in the reference's float arithmetic (0 / 0).  Candidates: origins at a corner or
    # at v0 + e1 / 4 + e2 / 4, directions a e1 + b e2 with small integer and power-of-two weights (a rounded
    # shear Sx, Sy then leaves rounding noise in the edge functions, which can pass the edge test); kept
    # where both terms are exactly zero.
    m = 24000 if len(T) > 8 else 60000
    k = rng.integers(0, len(T), m)
    Tk = T[k]
    e1, e2 = Tk[:, 1] - Tk[:, 0], Tk[:, 2] - Tk[:, 0]
    w = rng.choice([0.0, 0.25, 0.5, 1.0], (m, 2)).astype(f32)
    w[rng.integers(0, 2, m) == 0] = 0.0
    o = (Tk[:, 0] + w[:, :1] * f32(0.25) * e1) + w[:, 1:] * f32(0.25) * e2
    ab = rng.choice([-3.0, -2.0, -1.0, -0.5, 0.5, 1.0, 2.0, 3.0, 5.0, 7.0], (m, 2)).astype(f32)
    ab[rng.integers(0, 4, m) == 0, 1] = 0.0
    d = ab[:, :1] * e1 + ab[:, 1:] * e2
    num, den = plane_terms(Tk, o, d)
    keep = np.nonzero((num == 0) & (den == 0) & np.any(d != 0, axis=1))[0]
    if not grid:
        # ... and the ray lies in no other triangle's plane: not along an edge it shares with a neighbour, not in
        # the coplanar other half of a planar quad.  Decided here, from the geometry alone (float64): another
        # triangle counts as in-plane when the direction is within 2^-14 of its plane and the origin within
        # 2^-14 scene radii of it.  (The lattice is all coplanar neighbours, in exact arithmetic.)
        keep = keep[:4096]
        Td = T.astype(np.float64)
        na = np.cross(Td[:, 1] - Td[:, 0], Td[:, 2] - Td[:, 0])
        na /= np.maximum(np.linalg.norm(na, axis=1, keepdims=True), 1e-300)
        alone = np.zeros(len(keep), bool)
        for c in range(0, len(keep), 256):
            oc, dc = o[keep[c:c + 256]].astype(np.float64), d[keep[c:c + 256]].astype(np.float64)
            dc = dc / np.linalg.norm(dc, axis=1, keepdims=True)
            tilt = np.abs(dc @ na.T)
            dist = np.abs(np.einsum("rtc,tc->rt", Td[None, :, 0] - oc[:, None], na))
            alone[c:c + 256] = ((tilt < 2.0 ** -14) & (dist < 2.0 ** -14 * radius)).sum(axis=1) == 1
        keep = keep[alone]
    keep = keep[:1024]
    sets["nan_plane"] = rec(o[keep], d[keep])
    nrm = _cross(e1, e2)[keep].astype(np.float64)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    off = (o[keep] + (nrm * 0.25 * (radius if not grid else 1.0)).astype(f32)).astype(f32)
    num, den = plane_terms(Tk[keep], off, d[keep])
    ok = (num != 0) & (den == 0)
    sets["inf_plane"] = rec(off[ok], d[keep][ok])
    return sets


def tmax_edges(base, want):
    """The tmax set: for every ray of `base` the oracle's closest hit t* (want: its trace_n records, hits
    only) gives tmax in TMAX_EDGES, as a closest and as an any-hit query."""
    hit = want[:, 0] != nart_amd.TRACE_NO_HIT
    r, t = base[hit][:192], want[hit][:192, 1].view(f32)
    out = []
    for kind in (nart_amd.TRACE_CLOSEST, nart_amd.TRACE_ANY):
        for tm in (np.zeros_like(t), np.full_like(t, FLT_MIN), ulp_step(t, -1), t, ulp_step(t, 1), np.full_like(t, np.inf)):
            q = r.copy()
            q[:, 3] = tm
            q[:, 7] = np.full(len(q), kind, np.uint32).view(f32)
            out.append(q)
    return np.concatenate(out) if out else np.zeros((0, 8), f32)


def host_leaves(sc):
    """Of the host SAH tree (nart_amd.bvh_dump): {"sizes": triangles per leaf, "last": the scene triangles of the
    leaf that ends the record array}.  A leaf's records are read in groups of NART_TRI_PF, so a leaf of odd
    size reads one record past itself, and the last leaf reads into the NART_TRI_PAD padding records."""
    d = nart_amd.bvh_dump(sc)
    if not d["num_leaf_tris"]:
        return {"sizes": np.zeros(0, np.int64), "last": np.zeros(0, np.int64)}
    ch = d["nodes"]["child"].reshape(-1) if d["num_nodes"] else np.asarray([d["root_code"]])
    lc = (~ch[ch < 0].astype(np.int64)) & 0xFFFFFFFF
    first, count = lc >> 5, (lc & 31) + 1
    i = int(np.argmax(first))
    assert first[i] + count[i] == d["num_leaf_tris"]
    ids = d["tri_isect"].view(np.uint32)[first[i]:first[i] + count[i], 13].astype(np.int64)
    return {"sizes": count, "last": ids}


_PREPARED = {}


def prepared(name, directory):
    """Everything the tests of one scene share, computed once per process and changed by nobody: the scene,
    its ray sets {class: records} (tmax included), all rays in one array with the class of each, and the
    oracle's records for them."""
    if name not in _PREPARED:
        import time

        import oracle
        sc = scene(name, directory)
        T = sc.triangles()[:, :9].reshape(-1, 3, 3)
        orc = oracle.Oracle(sc)
        sets = designed(name, T, scene_maxabs(sc, T))
        beyond = sets.pop("beyond")
        leaves = host_leaves(sc)
        if len(leaves["last"]):  # rays at the triangles of the last leaf of the record array (its groups read the padding)
            rng = np.random.default_rng([SEED, SCENES.index(name), 1])
            k = leaves["last"][rng.integers(0, len(leaves["last"]), 256)]
            b = rng.dirichlet((4.0, 4.0, 4.0), 256)
            pts = np.einsum("nj,njc->nc", b, T[k].astype(np.float64)).astype(f32)
            nrm = np.cross(T[k, 1] - T[k, 0], T[k, 2] - T[k, 0]).astype(np.float64)
            nrm *= np.where(rng.integers(0, 2, 256) == 1, 1.0, -1.0)[:, None] / np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
            size = np.linalg.norm(T[k, 1] - T[k, 0], axis=1)[:, None]
            o32 = (pts + nrm * size + _unit(rng, 256) * size * 0.2).astype(f32)  # from close by, along the normal
            sets["last_leaf"] = nart_amd.trace_rays(o32, pts - o32)
        t0 = time.process_time()
        base = np.concatenate([sets["interior"][:256], sets["edge"][:128]] + ([sets["edge_axis"][:128]] if "edge_axis" in sets else []))
        sets["tmax"] = tmax_edges(base, oracle.trace_n(orc, base))
        sets["any"] = np.concatenate([sets[c][:n] for c, n in (("interior", 384), ("edge", 384), ("miss", 128), ("nan_plane", 256))])
        sets["any"][:, 7] = np.full(len(sets["any"]), nart_amd.TRACE_ANY, np.uint32).view(f32)
        names = sorted(sets)
        rays = np.concatenate([sets[c] for c in names])
        cls = np.concatenate([np.full(len(sets[c]), i) for i, c in enumerate(names)])
        want = oracle.trace_n(orc, rays)
        _PREPARED[name] = {"beyond": beyond, "beyond_want": oracle.trace_n(orc, beyond),
                           "leaves": leaves, "scene": sc, "tris": T, "sets": sets, "classes": names, "rays": rays, "cls": cls, "want": want,
                           "oracle_seconds": time.process_time() - t0}
    return _PREPARED[name]


def of_class(prep, c):
    return prep["cls"] == prep["classes"].index(c)


def set_aside(prep):
    """The rays of the one case the device is documented not to emulate (tests/test_octree_nan_case.py): the ray
    lies in a triangle's plane, Triangle::Intersect's plane distance is 0 / 0, the reference's answer rests on
    that triangle, and the BVH2 traversal need not test it, so nothing tells the device to replay the octree
    search.  Each part is shown by the oracle alone, per ray:
      * closest hit: a NaN plane distance passes Triangle::Intersect (TRACE_NAN_ACCEPTED), the reference's
        search answers differently once NaN distances are rejected, i.e. the NaN triangle shares the winner's
        chunk and emptied it (TRACE_NAN_DECIDES), and the origin lies outside that triangle's bounds
        (TRACE_NAN_OUTSIDE).  With the origin inside the bounds the ray starts inside the leaf's padded box and
        every box above it, so the leaf is reached whatever the tree: those rays are compared.
      * any hit: the NaN hides every hit of the reference's search (TRACE_NAN_HIDES: no hit, but a hit with
        NaN distances rejected).  The any-hit traversal ends at the first accepted hit, which may come before
        the NaN triangle's leaf.  Any-hit rays with a passing NaN that hides nothing are compared.
      * the answer itself, with or without the NaN triangles, is a ghost hit (TRACE_GHOST_WINS): 0 / 0 came out
        as a quotient of two roundings, a finite t before the ray enters the winner's bounds or on a ray that
        misses them (grown by 2^-12 of the coordinates involved), so the ray never enters the winner's leaf box
        at that distance."""
    import oracle
    flags = prep["want"][:, 2]
    any_hit = prep["rays"][:, 7].view(np.uint32) == nart_amd.TRACE_ANY
    both = oracle.TRACE_NAN_DECIDES | oracle.TRACE_NAN_OUTSIDE
    return np.where(any_hit, (flags & oracle.TRACE_NAN_HIDES) != 0, (flags & both) == both) | ((flags & oracle.TRACE_GHOST_WINS) != 0)


def compare(got, want):
    """Indices of the rays whose device record differs from the oracle's: triangle, t bits and the Isect
    words bit for bit where the oracle's float is not NaN, NaN where it is."""
    bad = (got[:, 0] != want[:, 0]) | (got[:, 1] != want[:, 1])
    wf, gf = want[:, 6:23].view(f32), got[:, 6:23].view(f32)
    nan = np.isnan(wf)
    bad |= np.any(np.where(nan, ~np.isnan(gf), got[:, 6:23] != want[:, 6:23]), axis=1)
    bad |= np.any(got[:, 23:26] != want[:, 23:26], axis=1)
    return np.nonzero(bad)[0]


def describe(prep, got, want, idx, limit=6):
    lines = ["%d of %d rays differ" % (len(idx), len(want))]
    for i in idx[:limit]:
        r = prep["rays"][i]
        lines.append("  ray %d (%s) o %r d %r tmax %r kind %d: device tri %d t %08x, oracle tri %d t %08x flags %x" % (
            i, prep["classes"][prep["cls"][i]], r[0:3].tolist(), r[4:7].tolist(), float(r[3]), int(r[7:8].view(np.uint32)[0]),
            got[i, 0], got[i, 1], want[i, 0], want[i, 1], want[i, 2]))
    return "\n".join(lines)
