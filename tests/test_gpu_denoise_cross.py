"""The cross-filtered denoiser (nart_hip_denoise_cross, nart_hip_render_denoised_cross,
`nart --denoise-cross`) on the device against its numpy restatement (tests/denoise_cross_py.py, validated
on the CPU by tests/test_denoise_cross_restatement.py): bit for bit, tolerance 0, except the measured
quality figures."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import denoise_cross_py as dx
import exr_py
import nart_amd

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
    return "%d of %d floats differ, max abs diff %g, first at %s" % (
        int(ne.sum()), ne.size, worst, idx[0].tolist() if len(idx) else None)


def _restate(p, images, params=None):
    g = nart_amd.session_geometry(p)
    return dx.denoise(p.image_width, p.image_height, g.filter_bounds, *images, params)


@pytest.fixture(scope="module")
def glass_renderer(gpu, glass_scene):
    r = nart_amd.HipRenderer(glass_scene)
    yield r
    r.close()


# ---------------------------------------------------------------- A. synthetic inputs, bit for bit
SIZES = [(1, 1), (5, 3), (70, 3), (37, 29), (129, 65)]


@pytest.mark.parametrize("fw", [2.0, 1.0], ids=["fw2", "fw1"])
@pytest.mark.parametrize("iterations", [1, 5])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_synthetic_bit_for_bit(glass_renderer, glass_scene, size, iterations, fw):
    """Guide regions, empty pixels, partial coverage, and the invalid pixels of every kind (no weight, a
    NaN half, an Inf half, a half without weight), on sizes that are no tile multiple, smaller than the
    reach of step 16, and one pixel thin.  One iteration stays in the LDS passes, five reach the global
    ones."""
    W, H = size
    p = _params(glass_scene, W, H, 2, filter_width=fw)
    g = nart_amd.session_geometry(p)
    fb = g.filter_bounds
    assert fb == int(fw)
    images, spots = dx.synthetic(W, H, fb, seed=W * 131 + H)
    if W * H >= 15:
        assert None not in spots[:3] and not np.isfinite(images[0]).all() and not np.isfinite(images[1]).all()
    dp = nart_amd.DenoiseParams.defaults(iterations=iterations)
    got = glass_renderer.denoise_cross(p, *images, params=dp)
    want, want_err = _restate(p, images, dp)
    assert got["denoised"].shape == want.shape == (g.total_height, g.total_width, 5)
    assert _bits_equal(got["denoised"], want), _report(got["denoised"], want)
    assert _bits_equal(got["error"], want_err), _report(got["error"], want_err)
    border = np.ones(want.shape[:2], bool)
    border[fb:fb + H, fb:fb + W] = False
    for im in (got["denoised"], got["error"]):
        assert not im[border].any() and (im[~border][:, 4] == 1).all()
    # swapping the halves changes no bit; the error image is optional
    swapped = glass_renderer.denoise_cross(p, images[1], images[0], *images[2:], params=dp)
    assert _bits_equal(swapped["denoised"], want) and _bits_equal(swapped["error"], want_err)
    only = glass_renderer.denoise_cross(p, *images, params=dp, with_error=False)
    assert "error" not in only and _bits_equal(only["denoised"], want)
    assert got["denoise_ms"] > 0
    t = glass_renderer.denoise_cross_timings()
    assert t["prepare"] > 0 and t["variance"] > 0 and t["finalize"] > 0
    assert all(x > 0 for x in t["passes"][:iterations]) and not any(t["passes"][iterations:])


def test_other_parameters_bit_for_bit(glass_renderer, glass_scene):
    """Every parameter away from its default, 8 iterations (step 128 on a 37 x 29 image); identical
    halves give an error image of exactly 0."""
    p = _params(glass_scene, 37, 29, 2)
    g = nart_amd.session_geometry(p)
    images, _spots = dx.synthetic(37, 29, g.filter_bounds, seed=77)
    dp = nart_amd.DenoiseParams.defaults(iterations=8, normal_squarings=2, sigma_color=1.5, sigma_depth=2.5, depth_eps=0.01,
                                         sigma_coverage=0.2, albedo_floor=0.05)
    got = glass_renderer.denoise_cross(p, *images, params=dp)
    want, want_err = _restate(p, images, dp)
    assert _bits_equal(got["denoised"], want), _report(got["denoised"], want)
    assert _bits_equal(got["error"], want_err), _report(got["error"], want_err)
    # null params are the defaults
    assert _bits_equal(glass_renderer.denoise_cross(p, *images)["denoised"],
                       glass_renderer.denoise_cross(p, *images, params=nart_amd.DenoiseParams.defaults())["denoised"])
    same = glass_renderer.denoise_cross(p, images[0], images[0], *images[2:])
    assert not same["error"][..., :3].any()


# ---------------------------------------------------------------- B. renders
@pytest.mark.parametrize("follow", [False, True], ids=["first_hit", "followed"])
def test_render_denoised_cross_matches_denoise_cross(gpu, glass_scene, follow):
    """render_denoised_cross (images kept on the device) equals denoise_cross fed with render_halves'
    images, which equals the restatement; its beauty equals render()."""
    p = _params(glass_scene, 48, 40, 4)
    gp = nart_amd.GuideParams.defaults() if follow else None
    r = nart_amd.HipRenderer(glass_scene)
    h = r.render_halves(p, albedo=True, normal=True, guides=gp)
    images = (h["halves"][0], h["halves"][1], h["beauty"], h["albedo"], h["normal"])
    want, want_err = _restate(p, images)
    got = r.denoise_cross(p, *images)
    assert _bits_equal(got["denoised"], want), _report(got["denoised"], want)
    assert _bits_equal(got["error"], want_err), _report(got["error"], want_err)
    out = r.render_denoised_cross(p, guides=gp)
    assert _bits_equal(out["denoised"], want), _report(out["denoised"], want)
    assert _bits_equal(out["error"], want_err), _report(out["error"], want_err)
    assert _bits_equal(out["beauty"], r.render(p))
    assert out["denoise_ms"] > 0.0
    t = r.denoise_cross_timings()
    assert t["prepare"] > 0 and t["variance"] > 0 and t["finalize"] > 0
    assert all(x > 0 for x in t["passes"][:5]) and not any(t["passes"][5:])
    only = r.render_denoised_cross(p, beauty=False, guides=gp)
    assert "beauty" not in only and _bits_equal(only["denoised"], want)
    fin = nart_amd.finalize(p, out["denoised"])
    assert np.isfinite(fin).all() and not _bits_equal(fin, nart_amd.finalize(p, out["beauty"]))
    assert (out["error"][..., :3] > 0).any()
    r.close()


def test_multi_device_matches_single(gpu, glass_scene, glass_renderer):
    p = _params(glass_scene, 64, 48, 4)
    single = glass_renderer.render_denoised_cross(p)
    m = nart_amd.HipRenderer(glass_scene, devices=[0, 0])
    assert m.devices() == (2, False)
    got = m.render_denoised_cross(p)
    for name in ("denoised", "error", "beauty"):
        assert _bits_equal(got[name], single[name]), (name, _report(got[name], single[name]))
    h = m.render_halves(p, albedo=True, normal=True)
    host = m.denoise_cross(p, h["halves"][0], h["halves"][1], h["beauty"], h["albedo"], h["normal"])
    assert _bits_equal(host["denoised"], single["denoised"]) and _bits_equal(host["error"], single["error"])
    assert _bits_equal(m.render(p), single["beauty"])
    m.close()


# ---------------------------------------------------------------- C. quality (measured, not tuned)
def _box5(a):
    """5 x 5 box mean with edge replication."""
    H, W = a.shape[:2]
    pad = np.pad(a, ((2, 2), (2, 2)) + ((0, 0),) * (a.ndim - 2), mode="edge")
    out = np.zeros_like(a, dtype=np.float64)
    for dy in range(5):
        for dx in range(5):
            out += pad[dy:dy + H, dx:dx + W]
    return out / 25.0


def test_quality_cornell(gpu, cornell_scene):
    """Cornell 128 x 128: 8 spp noisy, plain-denoised and cross-denoised against the same renderer at
    512 spp, with test_gpu_denoise.py's relMSE = mean((x - ref)^2 / (ref^2 + 0.01)) over the pixels whose
    512-spp coverage is >= 0.999.  Asserted: cross < noisy.  Printed: the three figures, the cross / plain
    ratio, and the correlation of the error image with the true squared error, both 5 x 5 box-blurred
    (the figures are in DESIGN.md, "Half buffers and cross-filtered denoising")."""
    r = nart_amd.HipRenderer(cornell_scene)
    p8, p512 = _params(cornell_scene, 128, 128, 8), _params(cornell_scene, 128, 128, 512)
    ref = r.render_aovs(p512, normal=False)
    plain = r.render_denoised(p8)
    cross = r.render_denoised_cross(p8)
    r.close()
    assert _bits_equal(plain["beauty"], cross["beauty"])
    mask = nart_amd.finalize(p512, ref["albedo"])[..., 3] >= 0.999
    x_ref = nart_amd.finalize(p512, ref["beauty"])[..., :3].astype(np.float64)

    def rel_mse(img):
        x = nart_amd.finalize(p8, img)[..., :3].astype(np.float64)
        return float((((x - x_ref) ** 2) / (x_ref ** 2 + 0.01))[mask].mean())

    noisy, den, crs = rel_mse(cross["beauty"]), rel_mse(plain["denoised"]), rel_mse(cross["denoised"])
    true_sq = (nart_amd.finalize(p8, cross["denoised"])[..., :3].astype(np.float64) - x_ref) ** 2
    est = nart_amd.finalize(p8, cross["error"])[..., :3].astype(np.float64)
    a, b = _box5(true_sq.mean(-1))[mask], _box5(est.mean(-1))[mask]
    corr = float(np.corrcoef(a, b)[0, 1])
    print("cornell 128x128 8 spp: mask keeps %.3f, relMSE noisy %.5f plain %.5f cross %.5f, cross/plain %.3f, "
          "cross/noisy %.3f; error image vs true squared error (5x5 box): correlation %.3f, mean estimate / mean true %.3f; "
          "denoise_ms plain %.3f cross %.3f" % (mask.mean(), noisy, den, crs, crs / den, crs / noisy, corr,
                                                float(b.mean() / a.mean()), plain["denoise_ms"], cross["denoise_ms"]))
    assert mask.mean() >= 0.90, mask.mean()
    assert crs < noisy, (crs, noisy)


# ---------------------------------------------------------------- D. errors, volume, CLI
def test_errors_leave_the_context_usable(gpu, glass_scene, glass_renderer, volume_scenes):
    vol = volume_scenes["c5"]
    pv = _params(vol, 32, 24, 2)
    rv = nart_amd.HipRenderer(vol)
    with pytest.raises(nart_amd.NartError) as e:
        rv.render_denoised_cross(pv)
    assert e.value.code == -6 and "volume" in str(e.value)  # NART_E_UNSUPPORTED
    rv.render(pv)
    rv.close()

    r = glass_renderer
    p = _params(glass_scene, 32, 24, 2)
    g = nart_amd.session_geometry(p)
    images, _spots = dx.synthetic(32, 24, g.filter_bounds, seed=1)
    good = r.denoise_cross(p, *images)
    bad = [dict(iterations=0), dict(iterations=9), dict(sigma_color=0.0), dict(sigma_depth=-1.0), dict(depth_eps=0.0),
           dict(sigma_coverage=0.0), dict(albedo_floor=0.0), dict(sigma_color=float("nan"))]
    for kw in bad:
        for call in (lambda dp: r.denoise_cross(p, *images, params=dp), lambda dp: r.render_denoised_cross(p, dp)):
            with pytest.raises(nart_amd.NartError) as e:
                call(nart_amd.DenoiseParams.defaults(**kw))
            assert e.value.code == -1, kw  # NART_E_INVALID
    p1 = _params(glass_scene, 32, 24, 1)  # one sample: a half would be empty
    for call in (lambda: r.denoise_cross(p1, *images), lambda: r.render_denoised_cross(p1)):
        with pytest.raises(nart_amd.NartError) as e:
            call()
        assert e.value.code == -1 and "spp" in str(e.value)
    gp = nart_amd.GuideParams.defaults()
    gp.max_follow = 11
    with pytest.raises(nart_amd.NartError) as e:
        r.render_denoised_cross(p, guides=gp)
    assert e.value.code == -1
    lib = nart_amd.hip_lib()
    out = np.zeros_like(images[0])
    d = [a.ctypes.data for a in images] + [out.ctypes.data]
    for k in range(6):
        args = list(d)
        args[k] = None
        assert lib.nart_hip_denoise_cross(r._ctx, ctypes.byref(p), None, *args, None, None) == -1, k
    assert lib.nart_hip_denoise_cross(r._ctx, None, None, *d, None, None) == -1
    assert lib.nart_hip_render_denoised_cross(r._ctx, ctypes.byref(p), None, None, None, d[5], None, None, None) == -1
    assert lib.nart_hip_render_denoised_cross(r._ctx, ctypes.byref(p), None, None, d[5], None, None, None, None) == -1
    assert not out.any()
    again = r.denoise_cross(p, *images)
    assert _bits_equal(again["denoised"], good["denoised"]) and _bits_equal(again["error"], good["error"])


def test_other_entry_points_keep_their_bits(gpu, glass_scene):
    """render, render_aovs(moment=True) and render_denoised give the same bits, launches and schedule
    before and after cross-denoise calls on the same context."""
    p = _params(glass_scene, 48, 32, 4)
    r = nart_amd.HipRenderer(glass_scene)

    def snapshot():
        st = nart_amd.RenderStats()
        a = r.render(p, st)
        b = r.render_aovs(p, moment=True)
        d = r.render_denoised(p)
        return {"render": a, "albedo": b["albedo"], "normal": b["normal"], "moment": b["moment"], "beauty": b["beauty"],
                "denoised": d["denoised"]}, (st.kernel_launches, st.schedule)

    before, st_before = snapshot()
    out = r.render_denoised_cross(p)
    r.render_denoised_cross(p, guides=nart_amd.GuideParams.defaults())
    h = r.render_halves(p, albedo=True, normal=True)
    host = r.denoise_cross(p, h["halves"][0], h["halves"][1], h["beauty"], h["albedo"], h["normal"])
    assert _bits_equal(host["denoised"], out["denoised"])
    after, st_after = snapshot()
    assert st_before == st_after
    for name in before:
        assert _bits_equal(before[name], after[name]), name
    r.close()


def test_cli_denoise_cross(gpu, glass_scene, tmp_path):
    base = [NART, glass_scene.path]
    size = ["-w", "48", "-h", "32", "-s", "4"]
    a_dir, b_dir, f_dir, bad_dir = tmp_path / "a", tmp_path / "b", tmp_path / "f", tmp_path / "bad"
    for d in (a_dir, b_dir, f_dir, bad_dir):
        d.mkdir()
    runs = ((a_dir, ["--denoise-cross"]), (b_dir, ["--halves", "--denoise-cross", "--aovs"]),
            (f_dir, ["--denoise-cross", "--follow-specular", "3"]))
    for d, extra in runs:
        res = subprocess.run(base + [str(d / "out")] + size + extra, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, (extra, res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    assert sorted(os.listdir(a_dir)) == sorted(os.listdir(f_dir)) == ["out.denoised.exr", "out.error.exr", "out.exr"]
    assert sorted(os.listdir(b_dir)) == ["out.albedo.exr", "out.denoised.exr", "out.error.exr", "out.exr", "out.half.0.exr",
                                         "out.half.1.exr", "out.normal.exr"]
    p = nart_amd.parse_args(["nart", glass_scene.path, "out"] + size)
    p = nart_amd.load_sessions(glass_scene.path, p)[0]
    r = nart_amd.HipRenderer(glass_scene)
    api = r.render_denoised_cross(p)
    halves = r.render_halves(p, albedo=True, normal=True)
    gp = nart_amd.GuideParams.defaults()
    gp.max_follow = 3
    followed = r.render_denoised_cross(p, guides=gp)
    r.close()
    to_half = nart_amd.scene_lib().nart_float_to_half

    def halves_of(img):
        final = nart_amd.finalize(p, img)
        return np.array([to_half(ctypes.c_float(v)) for v in final.reshape(-1)], np.uint16).reshape(final.shape)

    four = {"out.exr": api["beauty"], "out.denoised.exr": api["denoised"], "out.error.exr": api["error"]}
    more = dict(four, **{"out.half.0.exr": halves["halves"][0], "out.half.1.exr": halves["halves"][1],
                         "out.albedo.exr": halves["albedo"], "out.normal.exr": halves["normal"]})
    other = {"out.exr": followed["beauty"], "out.denoised.exr": followed["denoised"], "out.error.exr": followed["error"]}
    for d, names in ((a_dir, four), (b_dir, more), (f_dir, other)):
        for name, img in names.items():
            got, _hdr = exr_py.read_rgba_halves(str(d / name))
            assert got.shape == (32, 48, 4) and np.array_equal(got, halves_of(img)), (str(d), name)
    assert not _bits_equal(api["denoised"], followed["denoised"])
    # refused combinations: one message each, nothing written
    for extra in (["--denoise"], ["--light-groups", "each", "--denoise-parts"], ["--denoise", "--sample-variance"],
                  ["--adaptive", "0.1"], ["--robust"], ["--mattes"], ["--light-groups", "each"], ["--depth-cuts", "1"],
                  ["--cost"]):
        res = subprocess.run(base + [str(bad_dir / "out")] + size + ["--denoise-cross"] + extra, capture_output=True,
                             text=True, timeout=300)
        assert res.returncode != 0 and "--denoise-cross" in res.stderr and not res.stdout, extra
        assert res.stderr.count("Error:") == 1, (extra, res.stderr)
    res = subprocess.run(base + [str(bad_dir / "out"), "-w", "48", "-h", "32", "-s", "1", "--denoise-cross"], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode != 0 and "spp" in res.stderr
    assert os.listdir(bad_dir) == []
