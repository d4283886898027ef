"""k_primary_px: camera-ray packets of one pixel's samples (kernels.h), against k_primary's 16x4 blocks.

With pixel-major sample rows (the skew / rows splat layouts, the default), spp a multiple of 64 and
packet traversal on, launch_primary (render.hip) runs k_primary_px: a wave per slot, a packet per
64 consecutive samples.  NART_PRIMARY_PIXEL=0 restores k_primary.  hit[] must be word for word the
same, so every image here is compared as uint32 bits, tolerance 0, with the oracle's whole frame or
between the two hook settings.  Every case asserts the build it ran (scene_features()[1]), the path
names (schedule_names()) and, for whole renders, that the camera rays were traced first on a
pixel-major layout, so that none can pass by running another build or layout.

The frame is 41x23: 45x27 = 1,215 traced slots with the filter's border, no multiple of the four
slots of a k_primary_px block (the last block has one dead wave) nor of k_primary's 256.  spp 64 /
128 / 192 are one, two and three packets per slot; 72 and 8 are no multiple of 64 and keep k_primary
whatever the hook says.  The largest oracle frame is 1,215 x 192 samples.
"""
import numpy as np
import pytest

import nart_amd
import oracle
from nart_amd import scenes

pytestmark = pytest.mark.gpu

FT = nart_amd.api.FEATURES
FT_ALL = nart_amd.api.FT_ALL
FM_DIFFUSE = FT["lambert"] | FT["disk"]
FM_GLASS = FT["lambert"] | FT["glass"] | FT["disk"]
FM_ENVTEX = FT["lambert"] | FT["plastic"] | FT["environment"] | FT["texture"] | FT["normal_map"]
PATH_BITS = {"lean", "specialized", "probe_queue", "priority", "spec_pairs", "half_waves", "wave_groups"}
KNOBS = ("NART_RQ_PRIO", "NART_RQ_PAIRS", "NART_RQ_HALF", "NART_RQ_QUAD", "NART_RQ_SETPRIO", "NART_RQ_ORDER",
         "NART_RQ_TOPF", "NART_PROBE_SUB", "NART_QUEUE_K", "NART_LEAN_ROUNDS", "NART_LEAN_STACK", "NART_PRIMARY_PACKET",
         "NART_PRIMARY_PIXEL")
W, H = 41, 23
SLOTS = 45 * 27


def _params(scene, w, h, spp, **kw):
    p = nart_amd.load_sessions(scene.path)[0]
    p.image_width, p.image_height, p.spp = w, h, spp
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _report(a, b):
    ne = _bits(a) != _bits(b)
    return "%d of %d floats differ, max abs diff %g" % (int(ne.sum()), ne.size, float(np.nanmax(np.abs(a - b))))


def _assert_bits(a, b):
    assert np.shape(a) == np.shape(b) and np.array_equal(_bits(a), _bits(b)), _report(a, b)


@pytest.fixture(autouse=True)
def clean_knobs(monkeypatch):
    """Every case starts from the default schedule: no knob of the caller's environment leaks in."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def frames():
    """oracle_frame(scene, p) -> (image, path counts): each oracle frame of the module rendered once,
    read-only, shared by the cases that use it."""
    cache = {}

    def oracle_frame(scene, p):
        key = (scene.path, p.image_width, p.image_height, p.spp, p.bounces)
        if key not in cache:
            counts = {}
            img = oracle.Oracle(scene).render(p, counts=counts)
            img.setflags(write=False)
            cache[key] = (img, counts)
        return cache[key]

    return oracle_frame


@pytest.fixture(scope="module")
def c4_scene(built, tmp_path_factory):
    return nart_amd.Scene(scenes.c4_teapot(str(tmp_path_factory.mktemp("c4px")), env_size=(64, 32)))


def _render(scene, p, specialize=None, counters=False):
    """(image, stats, mask of the build that ran, path names) of one render on a fresh context; the
    camera rays were traced first and the sample rows are pixel-major (what launch_primary asks for)."""
    r = nart_amd.HipRenderer(scene)
    if specialize is not None:
        r.set_specialize(specialize)
    if counters:
        r.set_counters(True)
    st = nart_amd.RenderStats()
    img = r.render(p, st)
    build = r.scene_features()[1]
    r.close()
    names = set(st.schedule_names())
    assert "primary" in names and names & {"splat_rows", "splat_skew"}, names
    assert nart_amd.session_geometry(p).total_width * nart_amd.session_geometry(p).total_height == SLOTS
    return img, st, build, names & PATH_BITS


def _both(monkeypatch, fn):
    """fn() with NART_PRIMARY_PIXEL=1 and =0."""
    out = []
    for v in ("1", "0"):
        with monkeypatch.context() as m:
            m.setenv("NART_PRIMARY_PIXEL", v)
            out.append(fn())
    return out


@pytest.mark.parametrize("spp", [64, 128, 192])
def test_pixel_packets_against_oracle(gpu, glass_scene, frames, monkeypatch, spp):
    """glassSphere (FM_GLASS build) at one, two and three packets per slot: the default render equals
    the oracle's frame, and so do both hook settings (which are then equal to each other)."""
    p = _params(glass_scene, W, H, spp)
    ref = frames(glass_scene, p)[0]
    g, st, build, names = _render(glass_scene, p)
    assert build == FM_GLASS and names == {"specialized"}, (hex(build), names)
    _assert_bits(g, ref)
    for gi, _, bi, ni in _both(monkeypatch, lambda: _render(glass_scene, p)):
        assert bi == FM_GLASS and ni == {"specialized"}, (hex(bi), ni)
        _assert_bits(gi, ref)


@pytest.mark.parametrize("spp", [72, 8])
def test_other_spp_keep_block_packets(gpu, glass_scene, frames, monkeypatch, spp):
    """spp that is no multiple of 64 (72: more than one packet's worth; 8: less) runs k_primary with
    either hook setting: both equal the oracle's frame."""
    p = _params(glass_scene, W, H, spp)
    ref = frames(glass_scene, p)[0]
    for gi, _, bi, ni in _both(monkeypatch, lambda: _render(glass_scene, p)):
        assert bi == FM_GLASS and ni == {"specialized"}, (hex(bi), ni)
        _assert_bits(gi, ref)


@pytest.mark.parametrize("which,mask", [("cornell", FM_DIFFUSE), ("c4", FM_ENVTEX)], ids=["cornell", "c4-teapot"])
def test_other_specialised_builds(gpu, cornell_scene, c4_scene, frames, which, mask):
    """k_primary_px<false, false, FM_DIFFUSE> (Cornell) and the environment-light instantiation
    <false, true, FM_ENVTEX> (C4 teapot) at 64 spp against the oracle."""
    sc = cornell_scene if which == "cornell" else c4_scene
    p = _params(sc, W, H, 64)
    g, st, build, names = _render(sc, p)
    assert build == mask and names == {"specialized"}, (hex(build), names)
    _assert_bits(g, frames(sc, p)[0])


def test_generic_build(gpu, glass_scene, frames):
    """k_primary_px<false, false, FT_ALL>: glassSphere with set_specialize(False), 128 spp."""
    p = _params(glass_scene, W, H, 128)
    g, st, build, names = _render(glass_scene, p, specialize=False)
    assert build == FT_ALL and names == set(), (hex(build), names)
    _assert_bits(g, frames(glass_scene, p)[0])


def test_aov_primary_launch(gpu, glass_scene, monkeypatch):
    """launch_aov_primary (an AOV-only render, a matte-only render with planes, the per-sample AOV
    records: no path kernel ran, so k_primary is launched for them): first-hit AOVs, triangle ids
    and ID mattes identical between the two hook settings, glassSphere 41x23x128."""
    p = _params(glass_scene, W, H, 128)
    g = nart_amd.session_geometry(p)

    def run():
        r = nart_amd.HipRenderer(glass_scene)
        st = nart_amd.RenderStats()
        aov = r.render_aovs(p, beauty=False, stats=st)
        assert st.kernel_launches == 0  # no path kernel: the hits are launch_aov_primary's
        mat = r.render_mattes(p, nart_amd.MatteParams.defaults(), with_planes=True)
        rec, tri = r.render_aov_samples(p, 0, 0, g.total_width, g.total_height)
        r.close()
        return aov, mat, rec, tri

    (aov1, mat1, rec1, tri1), (aov0, mat0, rec0, tri0) = _both(monkeypatch, run)
    assert set(aov1) == set(aov0) and {"albedo", "normal"} <= set(aov1), sorted(aov1)
    for k in aov1:
        if isinstance(aov1[k], np.ndarray):
            _assert_bits(aov1[k], aov0[k])
    assert mat1["n_ids"] == mat0["n_ids"]
    _assert_bits(mat1["ranks"], mat0["ranks"])
    _assert_bits(mat1["planes"], mat0["planes"])
    assert np.array_equal(tri1, tri0) and (tri1 != 0xFFFFFFFF).any() and (tri1 == 0xFFFFFFFF).any()
    _assert_bits(rec1, rec0)


def test_counters(gpu, glass_scene, frames, monkeypatch):
    """The counter pass (k_primary_px<true, ...>, generic build) at 64 spp with both hook settings:
    rays_extend, rays_shadow and bounces equal each other; rays_extend, bounces and traced_samples
    equal the oracle's counts and rays_shadow is bounded by the oracle's visibility queries (the
    device skips occlusion queries whose term is exactly zero, so the oracle only bounds it: the rule
    of tests/test_gpu_build_matrix.py).  node_visits and tri_tests count the steps each lane takes
    part in, which depends on the packets' composition: only non-zero."""
    p = _params(glass_scene, W, H, 64)
    ref, oc = frames(glass_scene, p)
    runs = _both(monkeypatch, lambda: _render(glass_scene, p, counters=True))
    for g, st, build, names in runs:
        assert build == FT_ALL and names == set(), (hex(build), names)
        _assert_bits(g, ref)
        print("node_visits %d tri_tests %d rays_extend %d rays_shadow %d bounces %d" %
              (st.node_visits, st.tri_tests, st.rays_extend, st.rays_shadow, st.bounces))
        got = (st.rays_extend, st.bounces, st.traced_samples)
        assert got == (oc["extension_queries"], oc["shaded_hits"], oc["traced_samples"]), (got, oc)
        assert 0 < st.rays_shadow <= oc["visibility_queries"], (st.rays_shadow, oc)
        assert st.node_visits > 0 and st.tri_tests > 0
    a, b = runs[0][1], runs[1][1]
    assert (a.rays_extend, a.rays_shadow, a.bounces) == (b.rays_extend, b.rays_shadow, b.bounces)
