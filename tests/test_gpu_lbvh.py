"""Device-side BVH build (NART_BVH_BUILD=device, device/lbvh.h): a linear BVH
built by HIP kernels (Morton codes, radix sort, Karras hierarchy, bottom-up refit, breadth-first
emit) in the host build's node format.  Only the closest hit has to match the reference and the
traversal is exact for any tree, so every image must still equal the oracle's bit for bit."""
import numpy as np
import pytest

import bvh_check
import lbvh_scenes
import nart_amd
import oracle

pytestmark = pytest.mark.gpu


def _params(scene, w, h, spp, **kw):
    p = nart_amd.load_sessions(scene.path)[0]
    p.image_width, p.image_height, p.spp = w, h, spp
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.fixture
def device_bvh(monkeypatch):
    monkeypatch.setenv("NART_BVH_BUILD", "device")


@pytest.mark.parametrize("variant", [0, 3], ids=["rayqueue", "megakernel"])
def test_device_bvh_glass_sphere(gpu, glass_scene, device_bvh, variant):
    r = nart_amd.HipRenderer(glass_scene, variant=variant)
    b = r.bvh()
    assert b["on_device"] and b["num_leaf_tris"] > 0 and b["num_nodes"] > 0, b
    p = _params(glass_scene, 128, 96, 4)
    assert _bits_equal(r.render(p), oracle.Oracle(glass_scene).render(p))


def test_device_bvh_cornell_octree_buckets(gpu, cornell_scene, device_bvh):
    """The C2 buckets whose octree answers need the exact emulation (test_gpu_parity)."""
    import torch
    from test_gpu_parity import C2_OCTREE_BUCKETS
    p = _params(cornell_scene, 1920, 1080, 16)
    g = nart_amd.session_geometry(p)
    ids = np.array(C2_OCTREE_BUCKETS[:6], np.uint32)
    tiles = torch.zeros((len(ids), g.tile_size * g.tile_size, 5), dtype=torch.float32, device="cuda")
    r = nart_amd.HipRenderer(cornell_scene)
    assert r.bvh()["on_device"]
    r.render_buckets_async(p, ids, tiles.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert _bits_equal(tiles.cpu().numpy(), oracle.Oracle(cornell_scene).render_buckets(p, ids))


def test_device_bvh_materials_and_teapot(gpu, materials_scene, tmp_path, device_bvh):
    from nart_amd import scenes
    for sc, (w, h, spp) in ((materials_scene, (160, 120, 4)),
                            (nart_amd.Scene(scenes.c4_teapot(str(tmp_path))), (160, 90, 4))):
        r = nart_amd.HipRenderer(sc)
        b = r.bvh()
        assert b["on_device"], b
        p = _params(sc, w, h, spp)
        assert _bits_equal(r.render(p), oracle.Oracle(sc).render(p)), sc.path


def test_device_bvh_matches_host_image_and_reports(gpu, glass_scene, monkeypatch):
    p = _params(glass_scene, 96, 64, 8)
    host = nart_amd.HipRenderer(glass_scene)
    hb = host.bvh()
    assert not hb["on_device"]
    monkeypatch.setenv("NART_BVH_BUILD", "device")
    dev = nart_amd.HipRenderer(glass_scene)
    db = dev.bvh()
    assert db["on_device"] and db["num_leaf_tris"] == hb["num_leaf_tris"]
    assert _bits_equal(dev.render(p), host.render(p))


# ---------------------------------------------------------------- the tree itself
# The tests above see the tree through a few thousand rays.  The ones below read it back
# (HipRenderer.bvh_dump), run the validator over every node, box, leaf and record (tests/bvh_check.py),
# and compare it bit for bit with the numpy restatement of the build (tests/lbvh_py.py), on scenes
# that reach the sizes and key distributions where the build kernels change path (tests/lbvh_scenes.py).
IMAGE_CASES = ["empty", "one_leaf", "two_leaves_short", "cluster", "medium"]


@pytest.fixture(scope="module")
def scene_dir(gpu, tmp_path_factory):
    return str(tmp_path_factory.mktemp("lbvh"))


def _words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype != nart_amd.api.BVH_NODE_DTYPE else a.view(np.uint32).reshape(len(a), 16)


def _assert_is_restatement(d, prep, name):
    """The dumped device tree passes the validator and is the restatement's, word for word."""
    r, tris = prep["restated"], prep["tris"]
    lbvh_scenes.check_case(name, d["num_leaf_tris"])
    assert d["on_device"]
    bvh_check.check(d, tris, lbvh_scenes.expected_ids(name, prep), exact=True)
    assert (d["num_nodes"], d["num_leaf_tris"], d["root_code"], d["stack_depth"]) == (
        r["num_nodes"], r["num_leaf_tris"], r["root_code"], r["stack_depth"])
    assert np.float32(d["pad"]).view(np.uint32) == np.float32(prep["host"]["pad"]).view(np.uint32)
    w = _words(d["tri_isect"])
    assert np.array_equal(w[:, 13].astype(np.int64), r["order"]), "record order"
    assert np.array_equal(w[:, 14], prep["info"][r["order"]]), "word 14 per triangle id differs from the host build's"
    assert np.array_equal(_words(d["nodes"]), _words(r["nodes"])), "nodes"
    assert np.array_equal(w, _words(r["tri_isect"])), "records"
    assert np.array_equal(_words(d["tri_perm"]), _words(r["tri_perm"])), "permuted records"


@pytest.mark.parametrize("name", lbvh_scenes.SMALL)
def test_device_tree_is_valid_and_equals_restatement(scene_dir, device_bvh, name):
    prep = lbvh_scenes.prepared(name, scene_dir)
    if name == "cluster":
        lbvh_scenes.check_equal_codes(prep)
        assert prep["restated"]["stack_depth"] > lbvh_scenes.prepared("medium", scene_dir)["restated"]["stack_depth"]
    if name == "flat_axis":
        lbvh_scenes.check_flat_axis(prep)
    r = nart_amd.HipRenderer(prep["scene"])
    _assert_is_restatement(r.bvh_dump(), prep, name)


def test_device_tree_large_is_valid_and_equals_restatement(scene_dir, device_bvh):
    """m just over 262,144: k_lbvh_bounds goes round its grid-stride loop a second time, and the
    refit runs over a thousand contending workgroups' worth of leaves; invariant 4 (every child box
    is exactly its subtree's padded bounds) on all of its boxes is the check on that refit."""
    prep = lbvh_scenes.prepared("large", scene_dir)
    r = nart_amd.HipRenderer(prep["scene"])
    _assert_is_restatement(r.bvh_dump(), prep, "large")


def _images(scene, monkeypatch, build):
    if build == "device":
        monkeypatch.setenv("NART_BVH_BUILD", "device")
    else:
        monkeypatch.delenv("NART_BVH_BUILD", raising=False)
    p = _params(scene, 64, 48, 2)
    out = []
    for variant in (0, 3):
        r = nart_amd.HipRenderer(scene, variant=variant)
        assert r.bvh()["on_device"] == (build == "device")
        out.append(r.render(p))
        r.close()
    return p, out


@pytest.mark.parametrize("name", IMAGE_CASES)
def test_device_tree_renders_host_image(scene_dir, monkeypatch, name):
    prep = lbvh_scenes.prepared(name, scene_dir)
    p, dev = _images(prep["scene"], monkeypatch, "device")
    _, host = _images(prep["scene"], monkeypatch, "host")
    for variant, d, h in zip((0, 3), dev, host):
        assert _bits_equal(d, h), (name, variant)
    if name == "cluster":
        ref = oracle.Oracle(prep["scene"]).render(p)
        assert _bits_equal(dev[0], ref) and _bits_equal(dev[1], ref)
    if name in ("cluster", "medium"):
        assert (dev[0][..., :3].sum(-1) > 0).mean() > 0.1  # the camera does see the soup, not only the light


def test_device_tree_large_renders_host_image(scene_dir, monkeypatch):
    prep = lbvh_scenes.prepared("large", scene_dir)
    _, dev = _images(prep["scene"], monkeypatch, "device")
    _, host = _images(prep["scene"], monkeypatch, "host")
    assert _bits_equal(dev[0], host[0]) and _bits_equal(dev[1], host[1])


def test_device_tree_second_build_is_identical(scene_dir, device_bvh):
    """Two contexts, two builds, one tree.  This cannot prove the refit race-free -- a race may well
    lose the same way twice, or never on this day; the real check on the refit is invariant 4 on
    every box of the contended medium and large trees (the tests above)."""
    prep = lbvh_scenes.prepared("medium", scene_dir)
    a = nart_amd.HipRenderer(prep["scene"]).bvh_dump()
    b = nart_amd.HipRenderer(prep["scene"]).bvh_dump()
    for k in ("nodes", "tri_isect", "tri_perm"):
        assert np.array_equal(_words(a[k]), _words(b[k])), k
    assert (a["root_code"], a["stack_depth"], a["num_nodes"]) == (b["root_code"], b["stack_depth"], b["num_nodes"])


def test_device_tree_multi_device_rehearsal(scene_dir, device_bvh):
    """devices=[0, 0] with the device build: every sub-context builds its own tree; the image is the
    single-device image and the dump (the first device's tree) is the restatement's."""
    prep = lbvh_scenes.prepared("medium", scene_dir)
    p = _params(prep["scene"], 64, 48, 2)
    single = nart_amd.HipRenderer(prep["scene"]).render(p)
    multi = nart_amd.HipRenderer(prep["scene"], devices=[0, 0])
    assert multi.devices()[0] == 2 and multi.bvh()["on_device"]
    assert _bits_equal(multi.render(p), single)
    _assert_is_restatement(multi.bvh_dump(), prep, "medium")


def test_host_context_dump_equals_host_only_dump(scene_dir, monkeypatch):
    """The context hook on the default host build returns what the host-only hook returns."""
    monkeypatch.delenv("NART_BVH_BUILD", raising=False)
    prep = lbvh_scenes.prepared("inner_257", scene_dir)
    d, h = nart_amd.HipRenderer(prep["scene"]).bvh_dump(), prep["host"]
    assert not d["on_device"]
    for k in ("nodes", "tri_isect", "tri_perm"):
        assert np.array_equal(_words(d[k]), _words(h[k])), k
    assert (d["root_code"], d["stack_depth"], d["num_nodes"], d["pad"]) == (
        h["root_code"], h["stack_depth"], h["num_nodes"], h["pad"])
