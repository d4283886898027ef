"""The second-moment image (nart_hip_render_moment) and the denoiser's sample-variance mode
(nart_hip_denoise_moment, nart_hip_render_denoised_moment, `nart --denoise --sample-variance`) on the
device against their numpy restatements (tests/moment_py.py, validated on the CPU by
tests/test_moment_restatement.py): bit for bit, tolerance 0."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import denoise_py as dn
import exr_py
import moment_py as mp
import nart_amd
from test_aov_restatement import total_frame_uv

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NART = os.path.join(REPO, "nart_amd", "bin", "nart")
f32 = np.float32


def _params(scene, w, h, spp, **kw):
    p = nart_amd.load_sessions(scene.path)[0]
    p.image_width, p.image_height, p.spp = w, h, spp
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bits_equal(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _report(a, b):
    ne = _bits(a) != _bits(b)
    idx = np.argwhere(ne)
    with np.errstate(all="ignore"):
        worst = float(np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64)))) if ne.any() else 0.0
    return "%d of %d floats differ, max abs diff %g, first at %s" % (int(ne.sum()), ne.size, worst,
                                                                     idx[0].tolist() if len(idx) else None)


# ---------------------------------------------------------------- 1. the moment image, bit for bit
CONFIGS = {"b16_fw2": dict(bucket_size=16, filter_width=2.0), "b12_fw1": dict(bucket_size=12, filter_width=1.0)}
_restated = {}


def _restated_moment(scene, key, cfg, spp):
    """The restatement over the device's own per-sample Li_alpha of the whole total frame (24x20
    cropped), computed once per configuration and shared read-only."""
    if (key, cfg, spp) not in _restated:
        p = _params(scene, 24, 20, spp, **CONFIGS[cfg])
        g = nart_amd.session_geometry(p)
        r = nart_amd.HipRenderer(scene)
        L = r.render_samples(p, 0, 0, g.total_width, g.total_height)
        r.close()
        _restated[(key, cfg, spp)] = (p, mp.restate_moment(p, total_frame_uv(p), np.ascontiguousarray(L)))
    return _restated[(key, cfg, spp)]


def _ran(st, splat_mode, cfg):
    """The splat kernel family the schedule bits report, against the one the mode selects: rows and
    skew need power-of-two buckets (bucket 12 runs the one-pixel-per-lane kernels in every mode)."""
    names = st.schedule_names()
    pow2 = cfg == "b16_fw2"
    return ("splat_rows" in names) == (pow2 and splat_mode == 5) and ("splat_skew" in names) == (pow2 and splat_mode == 4)


CASES = [("b16_fw2", spp, mode) for spp in (2, 3, 5) for mode in (5, 4, 3, 1, 0)] + \
        [("b12_fw1", 3, 5), ("b12_fw1", 3, 0)]


@pytest.mark.parametrize("cfg,spp,splat_mode", CASES, ids=["%s-%dspp-mode%d" % c for c in CASES])
def test_moment_image_bit_for_bit(gpu, glass_scene, cfg, spp, splat_mode):
    """2, 3 and 5 spp reach the tails of the splat kernels' 4-sample unrolling; every splat family
    gives the restatement's bits; the beauty and the AOVs of the same call are the existing calls'."""
    p, want = _restated_moment(glass_scene, "glass", cfg, spp)
    assert want[..., :3].max() > 0 and want[..., 3].max() > 0
    r = nart_amd.HipRenderer(glass_scene, splat_mode=splat_mode)
    st = nart_amd.RenderStats()
    out = r.render_aovs(p, moment=True, stats=st)
    assert _ran(st, splat_mode, cfg), (splat_mode, st.schedule_names())
    assert _bits_equal(out["moment"], want), _report(out["moment"], want)
    plain = r.render(p)
    assert _bits_equal(out["beauty"], plain)
    assert _bits_equal(out["moment"][..., 4], plain[..., 4])
    aov = r.render_aovs(p)
    for name in ("beauty", "albedo", "normal"):
        assert _bits_equal(out[name], aov[name]), name
    assert out["moment_ms"] > 0 and out["aov_ms"] > 0 and "moment_ms" not in aov
    r.close()


def test_moment_alone_and_without_image(gpu, glass_scene):
    """aovs = 0; and a null image, where the path kernel still runs."""
    p, want = _restated_moment(glass_scene, "glass", "b16_fw2", 2)
    g = nart_amd.session_geometry(p)
    r = nart_amd.HipRenderer(glass_scene)
    st0, st1 = nart_amd.RenderStats(), nart_amd.RenderStats()
    plain = r.render(p, st0)
    out = r.render_aovs(p, albedo=False, normal=False, moment=True, stats=st1)
    assert set(out) == {"beauty", "moment", "moment_ms", "aov_ms"} and out["aov_ms"] == 0
    assert _bits_equal(out["moment"], want) and _bits_equal(out["beauty"], plain)
    assert st1.kernel_launches == st0.kernel_launches and st1.schedule == st0.schedule
    M = np.zeros((g.total_height, g.total_width, 5), f32)
    st2, ms = nart_amd.RenderStats(), ctypes.c_double()
    rc = nart_amd.hip_lib().nart_hip_render_moment(r._ctx, ctypes.byref(p), 0, None, None, None, M.ctypes.data,
                                                   ctypes.byref(st2), None, ctypes.byref(ms))
    assert rc == 0 and _bits_equal(M, want) and st2.kernel_launches == st0.kernel_launches and ms.value > 0
    r.close()


# ---------------------------------------------------------------- 2. volume integrator
def test_moment_volume_session(gpu, volume_scenes):
    vol = volume_scenes["c5"]
    p, want = _restated_moment(vol, "vol", "b16_fw2", 2)
    g = nart_amd.session_geometry(p)
    r = nart_amd.HipRenderer(vol)
    out = r.render_aovs(p, albedo=False, normal=False, moment=True)
    assert want[..., :3].max() > 0
    assert _bits_equal(out["moment"], want), _report(out["moment"], want)
    assert _bits_equal(out["beauty"], r.render(p))
    img = np.zeros((g.total_height, g.total_width, 5), f32)
    rc = nart_amd.hip_lib().nart_hip_render_moment(r._ctx, ctypes.byref(p), nart_amd.api.AOV_ALBEDO, img.ctypes.data,
                                                   img.ctypes.data, None, img.ctypes.data, None, None, None)
    assert rc == -6  # NART_E_UNSUPPORTED: first-hit AOVs need surfaces
    with pytest.raises(nart_amd.NartError) as e:
        r.render_denoised(p, sample_variance=True)
    assert e.value.code == -6
    assert _bits_equal(r.render_aovs(p, albedo=False, normal=False, moment=True)["moment"], want)
    r.close()


# ---------------------------------------------------------------- 3. a frame in several batches
def test_moment_batches(gpu, glass_scene, monkeypatch):
    """NART_BATCH_BYTES=1 leaves 256 slots (tests/test_gpu_entry_points.py
    test_batches_with_aov_slabs): the 28 x 24 total frame's buckets of 256, 192, 128 and 96 traced pixels
    go in three batches (the last two together), each writing at its own offset of the four
    back-to-back tile slabs."""
    p, want = _restated_moment(glass_scene, "glass", "b16_fw2", 2)
    monkeypatch.setenv("NART_BATCH_BYTES", "1")
    r = nart_amd.HipRenderer(glass_scene)
    st = nart_amd.RenderStats()
    out = r.render_aovs(p, moment=True, stats=st)
    g = nart_amd.session_geometry(p)
    assert g.n_buckets_x * g.n_buckets_y == 4 and st.kernel_launches == 3
    assert _bits_equal(out["moment"], want), _report(out["moment"], want)
    monkeypatch.delenv("NART_BATCH_BYTES")
    one = nart_amd.HipRenderer(glass_scene).render_aovs(p)
    for name in ("beauty", "albedo", "normal"):
        assert _bits_equal(out[name], one[name]), name
    r.close()


# ---------------------------------------------------------------- 4. the sample-variance denoiser
@pytest.fixture(scope="module")
def glass_renderer(gpu, glass_scene):
    r = nart_amd.HipRenderer(glass_scene)
    yield r
    r.close()


SIZES = [(1, 1), (5, 3), (70, 3), (37, 29)]


@pytest.mark.parametrize("iterations", [1, 5])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_denoise_moment_synthetic_bit_for_bit(glass_renderer, glass_scene, size, iterations):
    """denoise_py.synthetic's inputs (guide regions, empty and partly covered pixels, a zero-weight, a
    NaN and an Inf beauty pixel) with a moment image holding a pixel with mw = 0, one that clamps to
    0, one of 1e38 and one NaN."""
    W, H = size
    p = _params(glass_scene, W, H, 2)
    g = nart_amd.session_geometry(p)
    fb = g.filter_bounds
    (beauty, albedo, normal), _spots = dn.synthetic(W, H, fb, seed=W * 131 + H)
    moment, mspots = mp.synthetic_moment(W, H, fb, beauty, seed=W)
    if W * H >= 15:
        assert None not in mspots and not np.isfinite(moment).all()
    dp = nart_amd.DenoiseParams.defaults(iterations=iterations)
    got = glass_renderer.denoise(p, beauty, albedo, normal, dp, moment=moment)
    want = mp.denoise(W, H, fb, beauty, albedo, normal, moment, dp)
    assert got.shape == want.shape == (g.total_height, g.total_width, 5)
    assert _bits_equal(got, want), _report(got, want)
    assert np.isfinite(got).all()
    assert glass_renderer.denoise_timings()["variance"] == 0
    # the mode matters: the spatial estimate gives another image (beyond one pixel)
    if W * H >= 15:
        assert not _bits_equal(got, glass_renderer.denoise(p, beauty, albedo, normal, dp))
        assert glass_renderer.denoise_timings()["variance"] > 0


@pytest.mark.parametrize("name,w,h", [("cornell", 64, 48), ("glass", 48, 48)])
def test_render_denoised_sample_variance(gpu, request, name, w, h):
    """denoise(moment=) over render_aovs(moment=True) equals the restatement;
    render_denoised(sample_variance=True), with everything kept on the device, equals that; the
    variance kernel's time is 0 in this mode and > 0 in the default mode, in either order; the default
    mode's image is the same before and after."""
    scene = request.getfixturevalue({"cornell": "cornell_scene", "glass": "glass_scene"}[name])
    p = _params(scene, w, h, 4)
    g = nart_amd.session_geometry(p)
    r = nart_amd.HipRenderer(scene)
    before = r.render_denoised(p)
    assert r.denoise_timings()["variance"] > 0
    aov = r.render_aovs(p, moment=True)
    want = mp.denoise(w, h, g.filter_bounds, aov["beauty"], aov["albedo"], aov["normal"], aov["moment"])
    got = r.denoise(p, aov["beauty"], aov["albedo"], aov["normal"], moment=aov["moment"])
    assert _bits_equal(got, want), _report(got, want)
    assert r.denoise_timings()["variance"] == 0
    out = r.render_denoised(p, sample_variance=True)
    assert _bits_equal(out["denoised"], want), _report(out["denoised"], want)
    assert _bits_equal(out["beauty"], before["beauty"]) and out["denoise_ms"] > 0
    t = r.denoise_timings()
    assert t["variance"] == 0 and t["prepare"] > 0 and t["finalize"] > 0 and all(x > 0 for x in t["passes"][:5])
    after = r.render_denoised(p)
    assert r.denoise_timings()["variance"] > 0
    for key in ("denoised", "beauty"):
        assert _bits_equal(after[key], before[key]), key
    assert not _bits_equal(out["denoised"], before["denoised"])
    only = r.render_denoised(p, beauty=False, sample_variance=True)
    assert "beauty" not in only and _bits_equal(only["denoised"], want)
    assert r.denoise_timings()["variance"] == 0
    # the variance image for users with their own filter
    sv = nart_amd.sample_variance(p, aov["beauty"], aov["moment"])
    assert sv.shape == (h, w, 4) and np.isfinite(sv).all() and (sv >= 0).all() and sv[..., :3].max() > 0
    assert (sv[..., 3] >= 1).all()  # an effective sample count: (sum w)^2 / sum w^2
    r.close()


# ---------------------------------------------------------------- 5. two ranks
def test_two_rank_rehearsal(gpu, glass_scene, glass_renderer):
    p = _params(glass_scene, 64, 48, 4)
    single = glass_renderer.render_aovs(p, moment=True)
    single_dn = glass_renderer.render_denoised(p, sample_variance=True)
    m = nart_amd.HipRenderer(glass_scene, devices=[0, 0])
    assert m.devices() == (2, False)
    got = m.render_aovs(p, moment=True)
    for name in ("beauty", "albedo", "normal", "moment"):
        assert _bits_equal(got[name], single[name]), (name, _report(got[name], single[name]))
    assert got["moment_ms"] > 0
    alone = m.render_aovs(p, albedo=False, normal=False, moment=True)
    assert _bits_equal(alone["moment"], single["moment"])
    got_dn = m.render_denoised(p, sample_variance=True)
    for name in ("denoised", "beauty"):
        assert _bits_equal(got_dn[name], single_dn[name]), (name, _report(got_dn[name], single_dn[name]))
    assert m.denoise_timings()["variance"] == 0
    assert _bits_equal(m.denoise(p, got["beauty"], got["albedo"], got["normal"], moment=got["moment"]),
                       single_dn["denoised"])
    assert _bits_equal(m.render_denoised(p)["denoised"], glass_renderer.render_denoised(p)["denoised"])
    m.close()


# ---------------------------------------------------------------- 6. errors
def test_moment_errors_leave_the_context_usable(gpu, glass_scene, glass_renderer):
    r = glass_renderer
    p = _params(glass_scene, 32, 24, 2)
    g = nart_amd.session_geometry(p)
    good = r.render(p)
    aov = r.render_aovs(p, moment=True)
    p1 = _params(glass_scene, 32, 24, 1)
    one = r.render_aovs(p1, moment=True)  # the moment image itself exists at 1 spp
    for call in (lambda: r.denoise(p1, one["beauty"], one["albedo"], one["normal"], moment=one["moment"]),
                 lambda: r.render_denoised(p1, sample_variance=True)):
        with pytest.raises(nart_amd.NartError) as e:
            call()
        assert e.value.code == -1 and "spp" in str(e.value)
    assert _bits_equal(r.render(p), good)
    lib = nart_amd.hip_lib()
    ptr = lambda a: a.ctypes.data
    out = np.zeros((g.total_height, g.total_width, 5), f32)
    b, a, n = aov["beauty"], aov["albedo"], aov["normal"]
    assert lib.nart_hip_denoise_moment(r._ctx, ctypes.byref(p), None, ptr(b), ptr(a), ptr(n), None, ptr(out), None) == -1
    assert lib.nart_hip_render_moment(r._ctx, ctypes.byref(p), 3, ptr(out), ptr(out), ptr(out), None, None, None,
                                      None) == -1
    assert lib.nart_hip_render_moment(r._ctx, ctypes.byref(p), 0x4, ptr(out), ptr(out), ptr(out), ptr(out), None, None,
                                      None) == -1
    assert lib.nart_hip_render_moment(r._ctx, ctypes.byref(p), 2, ptr(out), ptr(out), None, ptr(out), None, None,
                                      None) == -1
    assert lib.nart_hip_render_aovs(r._ctx, ctypes.byref(p), 0x4, ptr(out), ptr(out), ptr(out), None, None) == -1
    assert _bits_equal(r.render(p), good)
    with pytest.raises(nart_amd.NartError) as e:
        r.render_aovs(p, beauty=False, moment=True)
    assert e.value.code == -1
    with pytest.raises(nart_amd.NartError) as e:
        r.denoise(p, b, a, n, nart_amd.DenoiseParams.defaults(iterations=9), moment=aov["moment"])
    assert e.value.code == -1
    assert _bits_equal(r.render(p), good)
    assert _bits_equal(r.render_aovs(p, moment=True)["moment"], aov["moment"])


# ---------------------------------------------------------------- 7. CLI
def test_cli_sample_variance(gpu, glass_scene, tmp_path):
    base = [NART, glass_scene.path]
    size = ["-w", "48", "-h", "32", "-s", "4"]

    def run(out, extra):
        r = subprocess.run(base + [out] + size + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        return r.stdout

    d_dir, both_dir, bad_dir = tmp_path / "d", tmp_path / "both", tmp_path / "bad"
    for d in (d_dir, both_dir, bad_dir):
        d.mkdir()
    run(str(d_dir / "out"), ["--denoise", "--sample-variance"])
    run(str(both_dir / "out"), ["--aovs", "--denoise", "--sample-variance"])
    assert sorted(os.listdir(d_dir)) == ["out.denoised.exr", "out.exr"]
    assert sorted(os.listdir(both_dir)) == ["out.albedo.exr", "out.denoised.exr", "out.exr", "out.normal.exr"]
    for name in ("out.exr", "out.denoised.exr"):
        assert (d_dir / name).read_bytes() == (both_dir / name).read_bytes(), name
    p = nart_amd.parse_args(["nart", glass_scene.path, "out"] + size)
    p = nart_amd.load_sessions(glass_scene.path, p)[0]
    api = nart_amd.HipRenderer(glass_scene).render_denoised(p, sample_variance=True)
    to_half = nart_amd.scene_lib().nart_float_to_half
    for name, img in (("out.exr", api["beauty"]), ("out.denoised.exr", api["denoised"])):
        halves, _hdr = exr_py.read_rgba_halves(str(d_dir / name))
        final = nart_amd.finalize(p, img)
        want = np.array([to_half(ctypes.c_float(v)) for v in final.reshape(-1)], np.uint16).reshape(final.shape)
        assert halves.shape == (32, 48, 4) and np.array_equal(halves, want), name
    # the flag alone: an error before anything is loaded or rendered
    r = subprocess.run(base + [str(bad_dir / "out")] + size + ["--sample-variance"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "--denoise" in r.stderr and not r.stdout
    assert os.listdir(bad_dir) == []


# ---------------------------------------------------------------- 8. quality (measured, not tuned)
@pytest.mark.parametrize("name", ["cornell", "glass"])
def test_quality_sample_variance(gpu, request, name):
    """128 x 128, 4 spp against 512 spp of the same renderer, with test_quality_cornell's relMSE
    = mean((x - ref)^2 / (ref^2 + 0.01)) over the pixels whose 512-spp coverage is >= 0.999.  Asserted:
    the sample-variance result beats the noisy input.  Printed: both modes and their ratio (the
    figures are in DESIGN.md, "Sample-variance denoising")."""
    scene = request.getfixturevalue({"cornell": "cornell_scene", "glass": "glass_scene"}[name])
    r = nart_amd.HipRenderer(scene)
    p4, p512 = _params(scene, 128, 128, 4), _params(scene, 128, 128, 512)
    ref = r.render_aovs(p512, normal=False)
    spatial = r.render_denoised(p4)
    moment = r.render_denoised(p4, sample_variance=True)
    r.close()
    mask = nart_amd.finalize(p512, ref["albedo"])[..., 3] >= 0.999
    x_ref = nart_amd.finalize(p512, ref["beauty"])[..., :3].astype(np.float64)

    def rel_mse(img):
        x = nart_amd.finalize(p4, img)[..., :3].astype(np.float64)
        return float((((x - x_ref) ** 2) / (x_ref ** 2 + 0.01))[mask].mean())

    noisy, sp, mo = rel_mse(moment["beauty"]), rel_mse(spatial["denoised"]), rel_mse(moment["denoised"])
    print("%s 128x128 4 spp: mask keeps %.3f, relMSE noisy %.5f spatial %.5f sample-variance %.5f, "
          "sample-variance / spatial %.3f" % (name, mask.mean(), noisy, sp, mo, mo / sp))
    assert mask.any() and mo < noisy, (mo, noisy)
