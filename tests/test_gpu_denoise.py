"""The a-trous denoiser on the device (nart_hip_denoise, nart_hip_render_denoised, `nart --denoise`)
against its numpy restatement (tests/denoise_py.py, validated on the CPU by
tests/test_denoise_restatement.py): bit for bit, tolerance 0."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import denoise_py as dn
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
    return "%d of %d floats differ, max abs diff %g, first at (y, x, c) %s" % (
        int(ne.sum()), ne.size, worst, idx[0].tolist() if len(idx) else None)


def _restate(p, beauty, albedo, normal, params=None):
    g = nart_amd.session_geometry(p)
    return dn.denoise(p.image_width, p.image_height, g.filter_bounds, beauty, albedo, normal, params)


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
    """Guide regions, empty pixels, partial coverage, a zero-weight pixel, one NaN and one Inf pixel,
    on sizes that are no tile multiple, smaller than the reach of step 16, and one pixel thin."""
    W, H = size
    p = _params(glass_scene, W, H, 1, filter_width=fw)
    g = nart_amd.session_geometry(p)
    assert g.filter_bounds == int(fw)
    (beauty, albedo, normal), spots = dn.synthetic(W, H, g.filter_bounds, seed=W * 131 + H)
    if W * H >= 15:
        assert None not in spots and not np.isfinite(beauty).all()
    dp = nart_amd.DenoiseParams.defaults(iterations=iterations)
    got = glass_renderer.denoise(p, beauty, albedo, normal, dp)
    want = _restate(p, beauty, albedo, normal, dp)
    assert got.shape == want.shape == (g.total_height, g.total_width, 5)
    assert _bits_equal(got, want), _report(got, want)
    assert np.isfinite(got).all()
    fb = g.filter_bounds
    border = np.ones(got.shape[:2], bool)
    border[fb:fb + H, fb:fb + W] = False
    assert not got[border].any() and (got[~border][:, 4] == 1).all()


def test_other_parameters_bit_for_bit(glass_renderer, glass_scene):
    """Every parameter away from its default, 8 iterations (step 128 on a 37 x 29 image)."""
    p = _params(glass_scene, 37, 29, 1)
    g = nart_amd.session_geometry(p)
    (beauty, albedo, normal), _spots = dn.synthetic(37, 29, g.filter_bounds, seed=77)
    dp = nart_amd.DenoiseParams.defaults(iterations=8, normal_squarings=2, sigma_color=1.5, sigma_depth=2.5, depth_eps=0.01,
                                         sigma_coverage=0.2, albedo_floor=0.05)
    got, want = glass_renderer.denoise(p, beauty, albedo, normal, dp), _restate(p, beauty, albedo, normal, dp)
    assert _bits_equal(got, want), _report(got, want)
    # null params are the defaults
    assert _bits_equal(glass_renderer.denoise(p, beauty, albedo, normal),
                       glass_renderer.denoise(p, beauty, albedo, normal, nart_amd.DenoiseParams.defaults()))


# ---------------------------------------------------------------- B. renders
@pytest.mark.parametrize("name,w,h", [("cornell", 64, 48), ("glass", 48, 48)])
def test_render_denoised_matches_restatement(gpu, request, name, w, h):
    """denoise() over render_aovs() output equals the restatement; render_denoised() (images kept on
    the device) equals that; its beauty equals render().  glassSphere has a glass first hit and a
    visible light."""
    scene = request.getfixturevalue({"cornell": "cornell_scene", "glass": "glass_scene"}[name])
    p = _params(scene, w, h, 4)
    r = nart_amd.HipRenderer(scene)
    aov = r.render_aovs(p)
    want = _restate(p, aov["beauty"], aov["albedo"], aov["normal"])
    got = r.denoise(p, aov["beauty"], aov["albedo"], aov["normal"])
    assert _bits_equal(got, want), _report(got, want)
    out = r.render_denoised(p)
    assert _bits_equal(out["denoised"], want), _report(out["denoised"], want)
    assert _bits_equal(out["beauty"], r.render(p))
    assert out["denoise_ms"] > 0.0
    t = r.denoise_timings()
    assert t["prepare"] > 0 and t["variance"] > 0 and t["finalize"] > 0
    assert all(x > 0 for x in t["passes"][:5]) and not any(t["passes"][5:])
    only = r.render_denoised(p, beauty=False)
    assert "beauty" not in only and _bits_equal(only["denoised"], want)
    # the filter did something, and finalize() takes the image as it takes a render
    fin = nart_amd.finalize(p, out["denoised"])
    assert np.isfinite(fin).all() and not _bits_equal(fin, nart_amd.finalize(p, out["beauty"]))
    r.close()


# ---------------------------------------------------------------- C. quality
def test_quality_cornell(gpu, cornell_scene):
    """Cornell 128 x 128: 4 spp noisy and denoised against the same renderer at 512 spp,
    relMSE = mean((x - ref)^2 / (ref^2 + 0.01)) over the pixels whose 512-spp coverage is >= 0.999
    (all but those where the emitter sits inside the splat footprint)."""
    r = nart_amd.HipRenderer(cornell_scene)
    p4, p512 = _params(cornell_scene, 128, 128, 4), _params(cornell_scene, 128, 128, 512)
    ref = r.render_aovs(p512, normal=False)
    out = r.render_denoised(p4)
    r.close()
    cov = nart_amd.finalize(p512, ref["albedo"])[..., 3]
    mask = cov >= 0.999
    x_ref = nart_amd.finalize(p512, ref["beauty"])[..., :3].astype(np.float64)

    def rel_mse(img):
        x = nart_amd.finalize(p4, img)[..., :3].astype(np.float64)
        return float((((x - x_ref) ** 2) / (x_ref ** 2 + 0.01))[mask].mean())

    noisy, den = rel_mse(out["beauty"]), rel_mse(out["denoised"])
    print("cornell 128x128 4 spp: mask keeps %.3f, relMSE noisy %.5f denoised %.5f ratio %.3f" % (
        mask.mean(), noisy, den, den / noisy))
    assert mask.mean() >= 0.90, mask.mean()
    assert den < noisy, (den, noisy)


# ---------------------------------------------------------------- D. multi-device
def test_multi_device_matches_single(gpu, glass_scene, glass_renderer):
    p = _params(glass_scene, 64, 48, 4)
    single = glass_renderer.render_denoised(p)
    m = nart_amd.HipRenderer(glass_scene, devices=[0, 0])
    assert m.devices() == (2, False)
    got = m.render_denoised(p)
    for name in ("denoised", "beauty"):
        assert _bits_equal(got[name], single[name]), (name, _report(got[name], single[name]))
    aov = m.render_aovs(p)
    assert _bits_equal(m.denoise(p, aov["beauty"], aov["albedo"], aov["normal"]), single["denoised"])
    assert _bits_equal(m.render(p), single["beauty"])
    m.close()


# ---------------------------------------------------------------- E. errors, volume, CLI
def test_errors_leave_the_context_usable(gpu, glass_scene, glass_renderer, volume_scenes):
    vol = volume_scenes["c5"]
    pv = _params(vol, 32, 24, 2)
    rv = nart_amd.HipRenderer(vol)
    with pytest.raises(nart_amd.NartError) as e:
        rv.render_denoised(pv)
    assert e.value.code == -6 and "volume" in str(e.value)  # NART_E_UNSUPPORTED
    rv.close()

    p = _params(glass_scene, 32, 24, 2)
    g = nart_amd.session_geometry(p)
    (beauty, albedo, normal), _spots = dn.synthetic(32, 24, g.filter_bounds, seed=1)
    good = glass_renderer.denoise(p, beauty, albedo, normal)
    bad = [dict(iterations=0), dict(iterations=9), dict(sigma_color=0.0), dict(sigma_depth=-1.0), dict(depth_eps=0.0),
           dict(sigma_coverage=0.0), dict(albedo_floor=0.0), dict(sigma_color=float("nan"))]
    for kw in bad:
        for call in (lambda dp: glass_renderer.denoise(p, beauty, albedo, normal, dp),
                     lambda dp: glass_renderer.render_denoised(p, dp)):
            with pytest.raises(nart_amd.NartError) as e:
                call(nart_amd.DenoiseParams.defaults(**kw))
            assert e.value.code == -1, kw  # NART_E_INVALID
    lib = nart_amd.hip_lib()
    out = np.zeros_like(beauty)
    ptr = lambda a: a.ctypes.data
    for args in [(None, ptr(albedo), ptr(normal), ptr(out)), (ptr(beauty), None, ptr(normal), ptr(out)),
                 (ptr(beauty), ptr(albedo), None, ptr(out)), (ptr(beauty), ptr(albedo), ptr(normal), None)]:
        assert lib.nart_hip_denoise(glass_renderer._ctx, ctypes.byref(p), None, *args, None) == -1
    assert lib.nart_hip_denoise(glass_renderer._ctx, None, None, ptr(beauty), ptr(albedo), ptr(normal), ptr(out), None) == -1
    assert lib.nart_hip_render_denoised(glass_renderer._ctx, ctypes.byref(p), None, None, None, None, None) == -1
    assert _bits_equal(glass_renderer.denoise(p, beauty, albedo, normal), good)


def test_cli_denoise(gpu, glass_scene, tmp_path):
    def run(out, extra):
        r = subprocess.run([NART, glass_scene.path, out, "-w", "48", "-h", "32", "-s", "4"] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        return r.stdout

    d_dir, both_dir = tmp_path / "d", tmp_path / "both"
    d_dir.mkdir()
    both_dir.mkdir()
    log = run(str(d_dir / "out"), ["--denoise"])
    run(str(both_dir / "out"), ["--aovs", "--denoise"])
    assert sorted(os.listdir(d_dir)) == ["out.denoised.exr", "out.exr"]
    assert sorted(os.listdir(both_dir)) == ["out.albedo.exr", "out.denoised.exr", "out.exr", "out.normal.exr"]
    assert ("Writing to %s..." % (d_dir / "out.denoised.exr")) in log
    for name in ("out.exr", "out.denoised.exr"):
        assert (d_dir / name).read_bytes() == (both_dir / name).read_bytes(), name
    p = nart_amd.parse_args(["nart", glass_scene.path, "out", "-w", "48", "-h", "32", "-s", "4"])
    p = nart_amd.load_sessions(glass_scene.path, p)[0]
    api = nart_amd.HipRenderer(glass_scene).render_denoised(p)
    to_half = nart_amd.scene_lib().nart_float_to_half
    for name, img in (("out.exr", api["beauty"]), ("out.denoised.exr", api["denoised"])):
        halves, _hdr = exr_py.read_rgba_halves(str(d_dir / name))
        final = nart_amd.finalize(p, img)
        want = np.array([to_half(ctypes.c_float(v)) for v in final.reshape(-1)], np.uint16).reshape(final.shape)
        assert halves.shape == (32, 48, 4) and np.array_equal(halves, want), name
