"""CPU tests of the oracle (the checker) and of reference behaviours it must reproduce.

The RNG, LatinSquare and Fresnel checks use a second, independent restatement in numpy /
Python of rng.h:8-59, sampling.cpp:64-86 and bxdf.cpp:3-22 so the C oracle is cross-checked
rather than trusted.  Everything here runs without a GPU.
"""
import json
import os

import numpy as np
import pytest

import nart_amd
import oracle

M32 = 0xFFFFFFFF


def np_rng_float_stream(seed, n):
    """rng.h: y = seed + 2463534242; xorshift 13/17/5; f = min(1-eps, float(u32(y*0x9E3779BB)) * 2^-32)."""
    y = (seed + 2463534242) & M32
    out = np.empty(n, np.float32)
    for i in range(n):
        y ^= (y << 13) & M32
        y ^= y >> 17
        y ^= (y << 5) & M32
        f = np.float32((y * 0x9E3779BB) & M32) * np.float32(2.3283064365386963e-10)
        out[i] = min(np.float32(1) - np.finfo(np.float32).eps, f)
    return out


def py_latin_square(seed, n):
    y = (seed + 2463534242) & M32

    def nxt():
        nonlocal y
        y ^= (y << 13) & M32
        y ^= y >> 17
        y ^= (y << 5) & M32
        return y

    def uf():
        f = np.float32((nxt() * 0x9E3779BB) & M32) * np.float32(2.3283064365386963e-10)
        return min(np.float32(1) - np.finfo(np.float32).eps, f)

    def ui(mx):
        return (((nxt() * 0x9E3779B9) & M32) * (mx + 1)) >> 32

    inv = np.float32(1) / np.float32(n)
    s = []
    for i in range(n):
        a = (np.float32(i) + uf()) * inv  # x drawn first (Clang left-to-right, Q2)
        b = (np.float32(i) + uf()) * inv
        s.append([a, b])
    for i in range(n):
        c = ui(n - 1 - i)
        s[i][0], s[c][0] = s[c][0], s[i][0]
        c = ui(n - 1 - i)
        s[i][1], s[c][1] = s[c][1], s[i][1]
    return np.array(s, np.float32), y


@pytest.mark.parametrize("seed", [0, 1, 260 * 7 + 3, 1924 * 1083 + 1919])
def test_rng_stream_independent_restatement(built, seed):
    assert np.array_equal(oracle.rng_stream(seed, 64), np_rng_float_stream(seed, 64))


@pytest.mark.parametrize("seed,spp", [(0, 1), (5, 4), (1234, 16), (999999, 33), (77, 256)])
def test_latin_square_independent_restatement(built, seed, spp):
    got, st = oracle.latin_square(seed, spp)
    want, wst = py_latin_square(seed, spp)
    assert np.array_equal(got, want)
    assert st == wst


@pytest.mark.parametrize("spp", [1, 2, 7, 16, 256])
def test_latin_square_strata(built, spp):
    s, _ = oracle.latin_square(4242, spp)
    for d in range(2):
        strata = np.floor(s[:, d].astype(np.float64) * spp).astype(int)
        assert sorted(strata) == list(range(spp))


def test_fresnel_known_answers(built):
    # normal incidence air -> glass: ((1.5-1)/(1.5+1))^2 = 0.04
    assert abs(oracle.fresnel(1.0, 1.5, 1.0) - 0.04) < 1e-6
    assert oracle.fresnel(1.5, 1.5, 0.3) == 0.0            # equal etas
    assert oracle.fresnel(1.5, 1.0, 0.1) == 1.0            # total internal reflection
    f = oracle.fresnel(1.0, 1.5, 0.5)
    ci = np.sqrt(1 - (1 / 1.5 * np.sqrt(1 - 0.25)) ** 2)
    rs = ((0.5 - 1.5 * ci) / (0.5 + 1.5 * ci)) ** 2
    rp = ((1.5 * 0.5 - ci) / (1.5 * 0.5 + ci)) ** 2
    assert abs(f - 0.5 * (rs + rp)) < 1e-6


def test_glass_sphere_octree_matches_survey(glass_scene):
    """Reference octree facts for glassSphere: Cleary grid 30x27x9,
    202 non-empty chunks (chunk-index bug included), one chunk of 1,761 triangles."""
    s = oracle.Oracle(glass_scene).bvh_stats()
    assert s["grid"] == (30, 27, 9)
    assert s["chunks"] == 202
    assert s["max_chunk_tris"] == 1761
    assert not s["root_is_leaf"]
    assert s["reachable_tris"] == 2560


def _one_chunk_scene(tmp_path):
    from nart_amd import scenes
    d = str(tmp_path)
    scenes.write_geo(os.path.join(d, "tri.geo"), [[0, 1, 2]], [(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(0, 0, 1)],
                     [[0, 0, 0]])
    scene = {"renderSessions": [{"imageWidth": 16, "imageHeight": 16, "spp": 2}],
             "camera": {"fov": 20, "transform": [1, 0, 0, 0.3, 0, 1, 0, 0.3, 0, 0, 1, 3, 0, 0, 0, 1]},
             "meshes": [{"filePath": os.path.join(d, "tri.geo"), "material": {"type": "lambert", "rho_d": [1, 1, 1]}}],
             "lights": [{"type": "disk", "radius": 0.5, "Le": [1, 1, 1], "intensity": 5,
                         "transform": [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 2, 0, 0, 0, 1]}]}
    path = os.path.join(d, "one.json")
    json.dump(scene, open(path, "w"))
    return path


def test_root_leaf_scene_renders_no_geometry(built, tmp_path):
    """Q14: one chunk -> the octree root stays a leaf and Octree::Intersect never hits
    (bvh.cpp:131-151): the triangle is invisible, alpha stays 0."""
    sc = nart_amd.Scene(_one_chunk_scene(tmp_path))
    o = oracle.Oracle(sc)
    assert o.bvh_stats()["root_is_leaf"]
    p = nart_amd.load_sessions(sc.path)[0]
    out = o.render_samples(p, 0, 0, 16, 16)
    assert np.all(out[..., 3] == 0.0)


def test_oracle_render_properties(glass_scene):
    p = nart_amd.load_sessions(glass_scene.path)[0]
    p.image_width, p.image_height, p.spp = 24, 16, 3
    o = oracle.Oracle(glass_scene)
    a = o.render(p, threads=4)
    b = o.render(p, threads=1)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))  # thread-count independent
    g = nart_amd.session_geometry(p)
    fb = g.filter_bounds
    inner = a[fb:fb + p.image_height, fb:fb + p.image_width]
    assert np.all(inner[..., 4] > 0)
    # rows/cols beyond W+fb / H+fb are never written by the combine (render.cpp:193-195)
    assert np.all(a[p.image_height + fb:, :, :] == 0) and np.all(a[:, p.image_width + fb:, :] == 0)
    s = o.render_samples(p, 0, 0, p.image_width, p.image_height)
    assert set(np.unique(s[..., 3])) <= {0.0, 1.0}
    assert np.isfinite(s).all()


def test_oracle_path_counts(glass_scene, materials_scene):
    """Oracle.render(counts=...): per-render path counts (nart_oracle.h ORACLE_N_*), the reference the
    counter pass's rays_extend / bounces / rays_shadow are checked against.  Counting changes no
    bit of the image, the sums do not depend on the number of workers, two renders running at the
    same time do not mix, and the counts obey the integrator's structure (pathintegrator.cpp:165-246)."""
    import threading
    frames = []
    for sc, w, h, spp in ((glass_scene, 40, 24, 3), (materials_scene, 33, 21, 2)):
        p = nart_amd.load_sessions(sc.path)[0]
        p.image_width, p.image_height, p.spp = w, h, spp
        o = oracle.Oracle(sc)
        c1, c4 = {}, {}
        a = o.render(p, threads=1, counts=c1)
        b = o.render(p, threads=4, counts=c4)
        plain = o.render(p, threads=4)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(a.view(np.uint32), plain.view(np.uint32))
        assert c1 == c4 and set(c1) == set(oracle.PATH_COUNTS)
        g = nart_amd.session_geometry(p)
        n = g.total_width * g.total_height * spp
        assert c1["traced_samples"] == n
        # one camera query per sample, then at most one more per shaded hit; a shaded hit makes at most
        # the two occlusion queries of EstimateDirect
        assert n <= c1["extension_queries"] <= n + c1["shaded_hits"]
        assert 0 < c1["shaded_hits"] < c1["extension_queries"]
        assert 0 < c1["visibility_queries"] <= 2 * c1["shaded_hits"]
        frames.append((o, p, c1))
        for bounces, ext in ((0, 0), (1, n)):
            q = p.copy()
            q.bounces = bounces
            c = {}
            o.render(q, counts=c)
            assert c["extension_queries"] == ext and c["traced_samples"] == n
            assert c["shaded_hits"] <= ext and (bounces or c["visibility_queries"] == 0)
    got = [{}, {}]
    th = [threading.Thread(target=lambda i=i: frames[i][0].render(frames[i][1], threads=3, counts=got[i]))
          for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert got[0] == frames[0][2] and got[1] == frames[1][2]


def test_oracle_tiles_combine_equals_render(glass_scene):
    """Render() == bucket tiles combined in raster order by the product's host combine."""
    p = nart_amd.load_sessions(glass_scene.path)[0]
    p.image_width, p.image_height, p.spp = 40, 24, 2
    o = oracle.Oracle(glass_scene)
    g = nart_amd.session_geometry(p)
    ids = np.arange(g.n_buckets_x * g.n_buckets_y, dtype=np.uint32)
    tiles = o.render_buckets(p, ids)
    img = nart_amd.combine_tiles(p, tiles)
    ref = o.render(p)
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))


def test_splat_wraps_at_bucket_edge(glass_scene):
    """render.cpp:52-61: a sample whose x + u rounds up to the bucket edge is splatted through
    glm::mod into the *start* of its own tile.  Find such a sample and check the tile."""
    p = nart_amd.load_sessions(glass_scene.path)[0]
    p.image_width, p.image_height, p.spp = 64, 32, 64
    found = None
    g = nart_amd.session_geometry(p)
    for y in range(p.image_height):
        for x in (15, 31, 47):
            uv, _ = oracle.latin_square(y * g.total_width + x, p.spp)
            sc = np.float32(x + g.filter_bounds) + uv[:, 0]
            hit = np.nonzero(sc == np.float32(x + g.filter_bounds + 1))[0]
            if len(hit):
                found = (x, y, int(hit[0]))
                break
        if found:
            break
    if not found:
        pytest.skip("no rounding sample in this window")
    # the oracle must stay self-consistent with the combine regardless
    o = oracle.Oracle(glass_scene)
    tiles = o.render_buckets(p, np.arange(g.n_buckets_x * g.n_buckets_y, dtype=np.uint32))
    assert np.isfinite(tiles).all()


def test_volume_oracle_properties(built, tmp_path):
    """Volume integrator restatement: alpha is always 1 (volumeintegrator.cpp:11,83); with the
    medium removed every sample returns the env light seen along the camera ray."""
    import json
    import numpy as np
    import nart_amd
    import oracle
    from nart_amd import scenes
    path = scenes.volume(str(tmp_path / "v"), kind="emissive")
    sc = nart_amd.Scene(path)
    p = nart_amd.load_sessions(path)[0]
    p.image_width, p.image_height, p.spp = 24, 16, 4
    out = oracle.Oracle(sc).render_samples(p, 0, 0, 24, 16)
    assert np.all(out[..., 3] == 1.0) and np.isfinite(out).all()
    j = json.load(open(path))
    del j["camera"]["medium"]
    path2 = str(tmp_path / "nomed.json")
    json.dump(j, open(path2, "w"))
    sc2 = nart_amd.Scene(path2)
    out2 = oracle.Oracle(sc2).render_samples(p, 0, 0, 24, 16)
    assert np.all(out2[..., 3] == 1.0) and (out2[..., :3] > 0).all()
    assert not np.array_equal(out, out2)
