"""The device BVH build's restatement (tests/lbvh_py.py) and the tree validator (tests/bvh_check.py)
on the CPU: the restatement's trees and the host's binned-SAH trees (nart_amd.bvh_dump, no device)
pass the validator on every edge-size scene of tests/lbvh_scenes.py and on the shipped scenes, and
the validator rejects each of eight corruptions by the name of the invariant it breaks.  The device
tree itself is compared with the restatement in tests/test_gpu_lbvh.py."""
import copy
import ctypes

import numpy as np
import pytest

import bvh_check
import lbvh_scenes
import nart_amd


@pytest.fixture(scope="module")
def scene_dir(built, tmp_path_factory):
    from nart_amd import build as nb
    nb.build_hip_lib()
    return str(tmp_path_factory.mktemp("lbvh"))


def _check_case(name, scene_dir):
    prep = lbvh_scenes.prepared(name, scene_dir)
    r, h = prep["restated"], prep["host"]
    lbvh_scenes.check_case(name, r["num_leaf_tris"])
    if name == "cluster":
        lbvh_scenes.check_equal_codes(prep)
        medium = lbvh_scenes.prepared("medium", scene_dir)["restated"]
        assert r["stack_depth"] > medium["stack_depth"], (r["stack_depth"], medium["stack_depth"])
    if name == "flat_axis":
        lbvh_scenes.check_flat_axis(prep)
    want = lbvh_scenes.expected_ids(name, prep)
    bvh_check.check(r, prep["tris"], want, exact=True)
    bvh_check.check(h, prep["tris"], want)
    # the host dump and the restatement hold the same visible set, and (m + 3) / 4 leaves make the tree
    assert np.array_equal(np.sort(r["order"]), np.sort(h["tri_isect"].view(np.uint32)[:, 13].astype(np.int64)))
    assert r["num_nodes"] == max((r["num_leaf_tris"] + 3) // 4 - 1, 0)
    assert h["num_leaf_tris"] == nart_amd.bvh_info(prep["scene"])["num_leaf_tris"]


@pytest.mark.parametrize("name", lbvh_scenes.SMALL)
def test_restatement_and_host_tree_pass_validator(scene_dir, name):
    _check_case(name, scene_dir)


def test_restatement_and_host_tree_pass_validator_large(scene_dir):
    _check_case("large", scene_dir)


@pytest.mark.parametrize("which", ["glass", "cornell", "materials"])
def test_host_tree_of_shipped_scenes_passes_validator(scene_dir, glass_scene, cornell_scene, materials_scene, which):
    sc = {"glass": glass_scene, "cornell": cornell_scene, "materials": materials_scene}[which]
    h = nart_amd.bvh_dump(sc)
    info = nart_amd.bvh_info(sc)
    assert (h["num_leaf_tris"], h["num_nodes"], h["stack_depth"]) == (
        info["num_leaf_tris"], info["num_nodes"], info["stack_depth"])
    ids = np.unique(h["tri_isect"].view(np.uint32)[:, 13].astype(np.int64))
    if which == "glass":  # the octree drops nothing of glassSphere (test_abi.test_bvh_depth_cap)
        assert np.array_equal(ids, np.arange(2560))
    bvh_check.check(h, sc.triangles(), ids)


def test_vectorised_geo_writer_writes_write_geo_file(scene_dir):
    """The large scenes' writer produces, byte for byte, the file scenes.write_geo writes."""
    import os
    a = lbvh_scenes.soup(os.path.join(scene_dir, "geo_a"), 37, 3, fast=False, flat_axis=2)
    b = lbvh_scenes.soup(os.path.join(scene_dir, "geo_b"), 37, 3, fast=True, flat_axis=2)
    geo = lambda p: open(os.path.join(os.path.dirname(p), "soup.geo"), "rb").read()  # noqa: E731
    assert geo(a) == geo(b) and len(geo(a)) > 37 * 9


def test_dump_hook_capacities(scene_dir):
    """nart_hip_bvh_dump: a size query fills info and copies nothing; a buffer that is too small, or
    only some buffers, is NART_E_INVALID."""
    prep = lbvh_scenes.prepared("three_leaves_short", scene_dir)
    lib, blob = nart_amd.hip_lib(), ctypes.c_void_p(prep["scene"].blob)
    info = nart_amd.api.BvhDumpInfo()
    assert lib.nart_hip_bvh_dump(blob, ctypes.byref(info), None, 0, None, 0, None, 0) == 0
    nn, nt = info.num_nodes, info.num_leaf_tris
    assert (nn, nt) == (prep["host"]["num_nodes"], prep["host"]["num_leaf_tris"]) and nt == 10 and nn >= 1
    nodes, rec, perm = np.zeros(nn * 16, np.float32), np.zeros(nt * 16, np.float32), np.zeros(nt * 48, np.float32)
    full = (nodes.ctypes.data, nn, rec.ctypes.data, nt * 16, perm.ctypes.data, nt * 48)
    for k in (1, 3, 5):
        short = list(full)
        short[k] -= 1
        assert lib.nart_hip_bvh_dump(blob, ctypes.byref(info), *short) == -1
        assert not nodes.any() and not rec.any() and not perm.any()
    assert lib.nart_hip_bvh_dump(blob, ctypes.byref(info), nodes.ctypes.data, nn, None, 0, perm.ctypes.data, nt * 48) == -1
    assert lib.nart_hip_bvh_dump(blob, None, *full) == -1
    assert lib.nart_hip_bvh_dump(blob, ctypes.byref(info), *full) == 0
    assert np.array_equal(rec.view(np.uint32), prep["host"]["tri_isect"].view(np.uint32).reshape(-1))


# ---------------------------------------------------------------- validator self-test
def _leaf_child(d, min_count):
    """(node, side) of a leaf child with at least min_count triangles."""
    code = ~d["nodes"]["child"].astype(np.int64)
    i, s = np.nonzero((d["nodes"]["child"] < 0) & ((code & 31) + 1 >= min_count))
    return int(i[len(i) // 2]), int(s[len(i) // 2])


def _shrink_box(d):
    i = d["num_nodes"] // 2
    d["nodes"]["hi0"][i, 1] = np.nextafter(d["nodes"]["hi0"][i, 1], np.float32(-np.inf))


def _drop_last_triangle(d):
    i, s = _leaf_child(d, 2)
    code = ~int(d["nodes"]["child"][i, s])
    d["nodes"]["child"][i, s] = ~(code - 1)  # count - 1 in the low five bits


def _duplicate_id(d):
    w = d["tri_isect"].view(np.uint32)
    w[5, 13] = w[6, 13]


def _share_child(d):
    inner = np.nonzero(d["nodes"]["child"][:, 0] >= 0)[0]
    a, b = int(inner[0]), int(inner[-1])
    assert a != b
    d["nodes"]["child"][b, 0] = d["nodes"]["child"][a, 0]


def _swap_nodes(d):
    depth, _ = bvh_check.walk(d)
    i = 1
    j = int(np.nonzero(depth > depth[i])[0][-1])
    p = np.arange(d["num_nodes"])
    p[i], p[j] = j, i
    nodes = d["nodes"][p]
    c = nodes["child"]
    nodes["child"] = np.where(c >= 0, p[np.maximum(c, 0)], c)  # the same tree, two nodes renumbered
    d["nodes"] = nodes


def _lower_stack(d):
    d["stack_depth"] -= 1


def _flip_plane_bit(d):
    d["tri_isect"].view(np.uint32)[7, 2] ^= 1


def _swap_perm_axes(d):
    r = d["tri_perm"][1, 9]
    assert r[0] != r[1]
    r[0], r[1] = r[1], r[0]


CORRUPTIONS = [("child box", _shrink_box), ("leaf ranges", _drop_last_triangle), ("triangle ids", _duplicate_id),
               ("reachability", _share_child), ("breadth-first order", _swap_nodes), ("stack depth", _lower_stack),
               ("record", _flip_plane_bit), ("permuted record", _swap_perm_axes)]


@pytest.mark.parametrize("source", ["restated", "host"])
@pytest.mark.parametrize("invariant,corrupt", CORRUPTIONS, ids=[c[1].__name__.lstrip("_") for c in CORRUPTIONS])
def test_validator_rejects_corruption(scene_dir, source, invariant, corrupt):
    prep = lbvh_scenes.prepared("inner_257", scene_dir)
    d = copy.deepcopy(prep[source])
    want = lbvh_scenes.expected_ids("inner_257", prep)
    bvh_check.check(d, prep["tris"], want, exact=source == "restated")  # valid before
    corrupt(d)
    with pytest.raises(bvh_check.BvhInvalid, match="^" + invariant + ":") as e:
        bvh_check.check(d, prep["tris"], want)
    assert e.value.invariant == invariant
