"""The followed guides' chain on the CPU (tests/guide_py.py over oracle.trace): which interfaces a
chain crosses and in which order, the nested-dielectric list and eta_outer at each, total internal
reflection, the step-through branch, the max_follow limit and the scenes that never follow.  The GPU
tests (tests/test_gpu_guides.py) compare the device with this restatement step by step."""
import numpy as np
import pytest

import guide_py
import nart_amd
import oracle
from guide_py import FOLLOWED, GUIDE_HIT, MISS, STEPPED
from nart_amd import scenes


def _params(scene, w, h, spp=1):
    p = nart_amd.load_sessions(scene.path)[0]
    p.image_width, p.image_height, p.spp = w, h, spp
    return p


def _centre_ray(orc, p, x, y):
    return oracle.camera_ray(orc, p.image_width, p.image_height, x, y, 0.5, 0.5)


def _pixel_towards(orc, p, point):
    """The total-image pixel whose centre ray passes nearest to `point`."""
    g = nart_amd.session_geometry(p)
    best = None
    for y in range(g.total_height):
        for x in range(g.total_width):
            o, d = _centre_ray(orc, p, x, y)
            v = np.asarray(point, np.float64) - o
            dist = np.linalg.norm(v - d * np.dot(v, d))
            if best is None or dist < best[0]:
                best = (dist, x, y)
    return best[1], best[2]


@pytest.fixture(scope="module")
def glass(glass_scene):
    return guide_py.GuideScene(glass_scene), oracle.Oracle(glass_scene), _params(glass_scene, 64, 36)


SPHERE_CENTRE = (-0.758663, -3.285489, 0.5)  # glassSphere: outer glass (mesh 0) and inner bubble (mesh 1)


def test_glass_sphere_centre_crosses_four_interfaces(glass):
    gs, orc, p = glass
    x, y = _pixel_towards(orc, p, SPHERE_CENTRE)
    o, d = _centre_ray(orc, p, x, y)
    for dtype in (np.float32, np.float64):
        steps = guide_py.walk(gs, orc, o, d, 8, dtype)
        assert [s["mesh"] for s in steps[:4]] == [0, 1, 1, 0], steps
        assert [s["decision"] for s in steps[:4]] == [FOLLOWED] * 4 and not any(s["tir"] for s in steps[:4])
        assert [s["valid"] for s in steps[:4]] == [True] * 4
        # outer glass from air, the bubble (eta 1, priority 3) from glass, out of it into glass, out into air
        assert [s["eta_outer"] for s in steps[:4]] == [1.0, 1.5, 1.5, 1.0]
        assert [s["list"] for s in steps[:5]] == [[], [0], [0, 1], [0], []]
        # behind the sphere: the backdrop (Lambert, the guide hit) or nothing
        assert len(steps) == 5
        last = steps[4]
        assert last["decision"] == MISS or (last["decision"] == GUIDE_HIT and last["mesh"] == 2 and last["lobe"] == "other")
    # the limit: at max_follow = 2 the third interface is the guide hit, on glass
    short = guide_py.walk(gs, orc, o, d, 2)
    assert [s["decision"] for s in short] == [FOLLOWED, FOLLOWED, GUIDE_HIT] and short[2]["lobe"] == "dielectric"
    # max_follow = 0: the first hit
    first = guide_py.walk(gs, orc, o, d, 0)
    assert len(first) == 1 and first[0]["decision"] == GUIDE_HIT and first[0]["mesh"] == 0


def test_total_internal_reflection_reflects(glass):
    """Along the pixel row through the sphere's centre some chain meets an interface beyond the
    critical angle: it is followed as a reflection -- the list is unchanged, and the next segment
    leaves on the side it came from."""
    gs, orc, p = glass
    _x, y = _pixel_towards(orc, p, SPHERE_CENTRE)
    g = nart_amd.session_geometry(p)
    found = 0
    for x in range(g.total_width):
        o, d = _centre_ray(orc, p, x, y)
        steps = guide_py.walk(gs, orc, o, d, 8)
        for k, s in enumerate(steps[:-1]):
            if s["decision"] == FOLLOWED and s["tir"]:
                found += 1
                assert s["lobe"] == "dielectric" and steps[k + 1]["list"] == s["list"]
                f = guide_py.hit_frame(gs.tris[s["tri"]], s["seg_o"], s["seg_d"], np.float64)
                side_in = np.dot(np.asarray(s["seg_d"], np.float64), f["gn"])
                side_out = np.dot(np.asarray(s["d"], np.float64), f["gn"])
                assert side_in * side_out < 0, (x, k)
    assert found > 0


def test_overlapping_spheres_step_through(built, tmp_path):
    sc = nart_amd.Scene(guide_py.two_sphere_scene(str(tmp_path)))
    gs, orc, p = guide_py.GuideScene(sc), oracle.Oracle(sc), _params(sc, 48, 36)
    x, y = _pixel_towards(orc, p, (0.0, 0.0, 1.0))
    o, d = _centre_ray(orc, p, x, y)
    steps = guide_py.walk(gs, orc, o, d, 8)
    assert [s["mesh"] for s in steps] == [0, 1, 0, 1, 2], steps
    assert [s["decision"] for s in steps] == [FOLLOWED, STEPPED, FOLLOWED, FOLLOWED, GUIDE_HIT]
    assert [s["valid"] for s in steps] == [True, False, True, True, True]
    assert [s["list"] for s in steps] == [[], [0], [0, 1], [1], []]
    # leaving the nearer sphere inside the farther one: eta_outer is the farther sphere's
    assert np.allclose([s["eta_outer"] for s in steps], [1.0, 1.3, 1.5, 1.0, 1.0])
    # the step-through keeps the direction and moves the origin along it
    s = steps[1]
    assert np.array_equal(s["d"], s["seg_d"]) and np.dot(s["o"] - s["seg_o"], s["seg_d"]) > 0
    # with the limit on the stepped-through interface it is the guide hit instead (validity is not
    # applied to the hit the chain stops on)
    short = guide_py.walk(gs, orc, o, d, 1)
    assert [s["decision"] for s in short] == [FOLLOWED, GUIDE_HIT] and short[1]["valid"] is False


@pytest.mark.parametrize("max_follow", [3, 8, 10])
def test_nested_glass_stops_on_a_shell(built, tmp_path, max_follow):
    sc = nart_amd.Scene(scenes.nested_glass(str(tmp_path)))
    gs, orc, p = guide_py.GuideScene(sc), oracle.Oracle(sc), _params(sc, 48, 36)
    x, y = _pixel_towards(orc, p, (0.0, 0.0, 1.0))
    o, d = _centre_ray(orc, p, x, y)
    steps = guide_py.walk(gs, orc, o, d, max_follow)
    # 14 shells, priority rising inward: the chain crosses one a segment and ends on shell max_follow
    assert len(steps) == max_follow + 1
    assert [s["mesh"] for s in steps] == list(range(max_follow + 1))
    assert [s["decision"] for s in steps] == [FOLLOWED] * max_follow + [GUIDE_HIT]
    assert steps[-1]["lobe"] == "dielectric" and steps[-1]["list"] == list(range(max_follow))
    assert len(steps[-1]["list"]) <= 10


def test_cornell_never_follows(cornell_scene):
    gs, orc, p = guide_py.GuideScene(cornell_scene), oracle.Oracle(cornell_scene), _params(cornell_scene, 32, 18)
    g = nart_amd.session_geometry(p)
    hits = 0
    for y in range(0, g.total_height, 3):
        for x in range(0, g.total_width, 3):
            o, d = _centre_ray(orc, p, x, y)
            steps = guide_py.walk(gs, orc, o, d, 8)
            assert len(steps) == 1 and steps[0]["decision"] in (GUIDE_HIT, MISS)
            hits += steps[0]["decision"] == GUIDE_HIT
    assert hits > 20


def test_rough_glass_glossy_and_plastic_stop_the_chain(materials_scene):
    """`materials`: only the mirror sphere (mesh 3) and the smooth inner glass (mesh 6) have a delta
    lobe; rough glass, glossy, plastic and Lambert are "other"."""
    gs = guide_py.GuideScene(materials_scene)
    kinds = {}
    for i, (first, _num, _mat, _prio) in enumerate(materials_scene.meshes()):
        kinds[i] = gs.lobe(first)[0]
    assert kinds == {0: "other", 1: "other", 2: "other", 3: "mirror", 4: "other", 5: "other", 6: "dielectric"}
