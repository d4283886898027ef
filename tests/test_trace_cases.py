"""The ray sets of the device trace probe (trace_cases.py) on the CPU, with the oracle alone: every class of
trouble holds at least 32 rays in every scene that can produce it, the cases behave as designed for the
reference, and the rays set aside for the one documented non-emulated case are few ("Probing the
traversal").  tests/test_gpu_trace.py then runs the same rays on the device.
"""
import numpy as np
import pytest

import nart_amd
import oracle
import trace_cases as tc

MIN = 32
NO_HIT = nart_amd.TRACE_NO_HIT
# what a scene cannot produce: a soup's triangles share no edge (no tie), nothing is visible in `empty`, one
# leaf under the octree's root is all the octree sees too, and the lattice's exact arithmetic zeroes the edge
# functions of every in-plane ray (module docstring of trace_cases)
NO_TIES = ("inner_256", "empty", "one_leaf")
NO_OCTREE_DIFFERENCE = ("inner_256", "one_leaf")
NO_ACCEPTED_NAN = ("lattice",)


@pytest.fixture(scope="module")
def scene_dir(built, tmp_path_factory):
    from nart_amd import build as nb
    nb.build_hip_lib()  # nart_amd.bvh_info / bvh_dump (host-only entry points of libnart_hip.so)
    return str(tmp_path_factory.mktemp("trace"))


@pytest.fixture(params=tc.SCENES)
def prep(request, scene_dir):
    return request.param, tc.prepared(request.param, scene_dir)


def _hit(prep, mask):
    w, closest = prep["want"][mask], prep["rays"][mask][:, 7].view(np.uint32) == nart_amd.TRACE_CLOSEST
    return np.where(closest, w[:, 0] != NO_HIT, w[:, 0] == 1)


def test_scene_sizes(prep):
    name, p = prep
    assert 1 <= len(p["tris"]) <= 4096 and len(p["rays"]) <= 65536
    info = nart_amd.bvh_info(p["scene"])
    if name == "empty":
        assert info["num_leaf_tris"] == 0  # the root stays a leaf: geometry_visible is false
    if name == "one_leaf":
        assert 1 <= info["num_leaf_tris"] <= 4 and info["num_nodes"] == 0
    if name == "inner_256":
        assert (info["num_leaf_tris"] + 3) // 4 - 1 == 256
    if name == "cluster":
        assert info["stack_depth"] >= 4  # sk = 1 and 2 leave levels for the global column


def test_leaf_sizes_and_the_last_leaf(scene_dir):
    """The leaf loop's grouped loads (NART_TRI_PF = 2 records at a time, padding after the array): the host
    trees of these scenes hold leaves of 1, 2, 3, 4, 5 and 7 triangles (the builders make none larger on
    scenes this small), and in every scene with a tree at least 32 rays are answered from the last leaf."""
    sizes = set()
    for name in tc.SCENES:
        p = tc.prepared(name, scene_dir)
        sizes |= set(p["leaves"]["sizes"].tolist())
        if name == "empty":
            assert "last_leaf" not in p["classes"]
            continue
        w = p["want"][tc.of_class(p, "last_leaf")]
        assert np.isin(w[:, 0], p["leaves"]["last"]).sum() >= MIN, name
    assert {1, 2, 3, 4, 5, 7} <= sizes, sizes


def test_every_class_is_populated(prep):
    name, p = prep
    flags = p["want"][:, 2]
    pop = {c: int(tc.of_class(p, c).sum()) for c in p["classes"]}
    for c in ("interior", "vertex", "edge", "direction", "origin_on_triangle", "origin_on_vertex", "origin_inside", "far",
              "miss", "nan_plane", "any"):
        assert pop[c] >= MIN, (c, pop)
    if name == "lattice":
        assert pop["edge_axis"] >= MIN and pop["origin_on_face"] >= MIN
    if name != "empty":
        for c in ("interior", "vertex", "edge", "direction", "far", "origin_inside", "any"):
            assert _hit(p, tc.of_class(p, c)).sum() >= MIN, c
        assert pop["tmax"] == 2 * len(tc.TMAX_EDGES) * 192 and pop["inf_plane"] >= MIN
    assert (flags[tc.of_class(p, "nan_plane")] & oracle.TRACE_NAN).astype(bool).sum() >= MIN
    if name not in NO_ACCEPTED_NAN:
        assert (flags[tc.of_class(p, "nan_plane")] & oracle.TRACE_NAN_ACCEPTED).astype(bool).sum() >= MIN
    if name not in NO_TIES:
        assert (flags & oracle.TRACE_TIE_CLOSEST).astype(bool).sum() >= MIN
    if name not in NO_OCTREE_DIFFERENCE:
        assert (flags & oracle.TRACE_NOT_BRUTE).astype(bool).sum() >= MIN
    assert (~_hit(p, np.ones(len(flags), bool))).sum() >= MIN


def test_direction_set_holds_every_special_component(prep):
    _, p = prep
    d = p["rays"][tc.of_class(p, "direction")][:, 4:7]
    bits = d.view(np.uint32)
    for s in tc.SPECIALS:
        b = np.float32(s).view(np.uint32)
        one = ((bits == b).sum(axis=1) == 1).sum()
        two = ((bits == b).sum(axis=1) == 2).sum()
        assert one >= 16 and two >= 16, (s, one, two)
    scale = np.abs(p["rays"][tc.of_class(p, "interior")][:, 4:7]).max(axis=1)
    # ray i carries SCALES[i % 3]: directions of about 1e-3, 1 and 1e3 times the distance to the target
    assert len(scale) // 3 >= MIN and np.median(scale[2::3]) > 1e5 * np.median(scale[0::3])


def test_cases_behave_as_designed(prep):
    name, p = prep
    w, r, flags = p["want"], p["rays"], p["want"][:, 2]
    assert not _hit(p, tc.of_class(p, "miss")).any()
    assert np.all(flags[tc.of_class(p, "nan_plane")] & oracle.TRACE_NAN)
    # a hit's t lies in (0, tmax), whatever the class
    closest = (r[:, 7].view(np.uint32) == nart_amd.TRACE_CLOSEST) & (w[:, 0] != NO_HIT)
    t = w[closest, 1].view(np.float32)
    assert np.all(t > 0) and np.all(t < r[closest, 3])
    assert np.array_equal(w[~closest & (r[:, 7].view(np.uint32) == nart_amd.TRACE_CLOSEST), 1].view(np.float32),
                          r[~closest & (r[:, 7].view(np.uint32) == nart_amd.TRACE_CLOSEST), 3])  # a miss returns tmax
    if name == "lattice":
        m = tc.of_class(p, "edge_axis")
        assert (flags[m] & oracle.TRACE_TIE_CLOSEST).astype(bool).sum() >= MIN
    if name == "empty":
        assert not _hit(p, np.ones(len(w), bool)).any()
        return
    # tmax edges: [kind][edge][ray]
    m = tc.of_class(p, "tmax")
    n = 192
    tw, tr = w[m].reshape(2, len(tc.TMAX_EDGES), n, -1), r[m].reshape(2, len(tc.TMAX_EDGES), n, -1)
    e = {k: i for i, k in enumerate(tc.TMAX_EDGES)}
    tstar = tr[0, e["at"], :, 3]
    assert np.array_equal(tw[0, e["inf"], :, 1].view(np.float32), tstar)  # t* is the oracle's own hit
    assert np.all(tw[0, e["zero"], :, 0] == NO_HIT) and np.all(tw[1, e["zero"], :, 0] == 0)
    assert np.all(tw[0, e["min_normal"], :, 0] == NO_HIT) and np.all(tw[1, e["min_normal"], :, 0] == 0)
    # tmax = t*: Triangle::Intersect's t >= tMax rejects the hit at t* itself
    at = tw[0, e["at"]]
    assert np.all((at[:, 0] == NO_HIT) | (at[:, 1].view(np.float32) < tstar))
    # closest and any-hit are one search: a hit exists for one iff it does for the other
    assert np.array_equal(tw[0, :, :, 0] != NO_HIT, tw[1, :, :, 0] == 1)
    assert (tw[0, e["above"], :, 0] != NO_HIT).sum() >= MIN and (tw[0, e["below"], :, 0] == NO_HIT).sum() >= MIN


def test_few_rays_are_set_aside(prep):
    """The carve-out (trace_cases.set_aside): at most 1 % of a scene's rays, and none of the designed NaN set,
    which is fixed before the oracle runs (trace_cases.designed) and holds every ray designed() returned."""
    _, p = prep
    aside = tc.set_aside(p)
    assert aside.mean() <= 0.01, aside.sum()
    assert tc.of_class(p, "nan_plane").sum() == len(p["sets"]["nan_plane"]) and "nan_neighbour" not in p["classes"]
    assert not aside[tc.of_class(p, "nan_plane")].any()
    # any-hit copies of NaN rays are compared wherever the NaN hides no hit
    any_nan = tc.of_class(p, "any") & ((p["want"][:, 2] & oracle.TRACE_NAN_ACCEPTED) != 0)
    assert (any_nan & ~aside).sum() >= MIN or p["want"][tc.of_class(p, "nan_plane"), 2].max() & oracle.TRACE_NAN_ACCEPTED == 0


def test_batched_trace_is_the_single_ray_trace(prep):
    """oracle_trace_n against oracle_trace (which keeps its behaviour) on rays without a tie or NaN, where the
    single-ray function's triangle lookup by t is unambiguous."""
    _, p = prep
    orc = oracle.Oracle(p["scene"])
    plain = np.nonzero((p["want"][:, 2] & (oracle.TRACE_TIE | oracle.TRACE_NAN)) == 0)[0]
    closest = plain[p["rays"][plain, 7].view(np.uint32) == nart_amd.TRACE_CLOSEST]
    for i in closest[:: max(1, len(closest) // 200)]:
        r, w = p["rays"][i], p["want"][i]
        g, t, bg, bt = oracle.trace(orc, r[0:3], r[4:7], float(r[3]))
        assert (g & 0xFFFFFFFF, np.float32(t).view(np.uint32)) == (w[0], w[1]), i
        assert (bg & 0xFFFFFFFF, np.float32(bt).view(np.uint32)) == (w[3], w[4]), i
