"""Properties of the denoiser's numpy restatement (tests/denoise_py.py), the yardstick of
tests/test_gpu_denoise.py, checked without a GPU so that it is validated independently of the
kernels; and the parts of the denoise ABI that need no device (defaults, null arguments)."""
import ctypes

import numpy as np

import denoise_py as dn
import nart_amd

f32 = np.float32


def _rgb(out, fb):
    H, W = out.shape[0] - 2 * fb, out.shape[1] - 2 * fb
    return out[fb:fb + H, fb:fb + W, :3]


def _half_planes(W, H, fb, rgb):
    """Two half-planes meeting at x = W / 2 with orthogonal normals, equal depth, full coverage."""
    left = np.mgrid[0:H, 0:W][1] < W // 2
    n = np.where(left[..., None], f32([0, 0, 1]), f32([1, 0, 0])).astype(f32)
    z = np.full((H, W), 5, f32)
    one = np.ones((H, W), f32)
    return left, dn.images_of(W, H, fb, rgb, one, np.full((H, W, 3), 0.5, f32), one, n, z)


def test_edge_is_kept():
    """No tap crosses the normal edge: every output pixel lies within [min, max] of its own side's
    input (relative slack 1e-5), while the two sides differ by far more than their noise."""
    W, H, fb = 48, 20, 2
    rng = np.random.default_rng(1)
    left0 = np.mgrid[0:H, 0:W][1] < W // 2
    rgb = (np.where(left0, 0.2, 3.0)[..., None] * rng.uniform(0.8, 1.25, (H, W, 3))).astype(f32)
    left, imgs = _half_planes(W, H, fb, rgb)
    out = _rgb(dn.denoise(W, H, fb, *imgs), fb)
    for side in (left, ~left):
        for ch in range(3):
            lo, hi = rgb[..., ch][side].min(), rgb[..., ch][side].max()
            got = out[..., ch][side]
            assert got.min() >= lo * (1 - 1e-5) and got.max() <= hi * (1 + 1e-5), (ch, lo, hi, got.min(), got.max())
    # and it did filter: each side's spread shrank
    assert out[..., 0][left].std() < 0.5 * rgb[..., 0][left].std()


def test_constant_signal_comes_back():
    W, H, fb = 37, 29, 2
    (beauty, albedo, normal), _spots = dn.synthetic(W, H, fb, seed=3, bad_pixels=False)
    # a constant demodulated signal over the synthetic guides: beauty = 1.7 * a_d, weights kept
    with np.errstate(all="ignore"):
        st = dn.prepare(W, H, fb, beauty, albedo, normal, dn.params_of())
    w = beauty[fb:fb + H, fb:fb + W, 4]
    beauty[fb:fb + H, fb:fb + W, :3] = (f32(1.7) * st["a_d"]) * w[..., None]
    out = _rgb(dn.denoise(W, H, fb, beauty, albedo, normal), fb)
    want = f32(1.7) * st["a_d"]
    live = w > 0
    assert np.allclose(out[live], want[live], rtol=1e-6, atol=0)
    # the zero-weight pixel is a valid black pixel (c = 0) without coverage: it stays black and,
    # its coverage being 0 among covered neighbours, reaches none of them
    assert (~live).sum() == 1 and not out[~live].any()


def test_non_finite_pixels_do_not_spread():
    """One NaN and one Inf beauty pixel: the output is finite everywhere, and pixels beyond the
    filter's reach of them (Chebyshev distance > 2 * (1 + 2 + ... + 2^(iterations-1)), plus the
    3-pixel variance window and the 1-pixel variance blur) are bit-identical to the run on inputs
    where those two pixels are finite."""
    W, H, fb, it = 70, 40, 2, 3
    (beauty, albedo, normal), spots = dn.synthetic(W, H, fb, seed=5)
    clean = beauty.copy()
    for x, y in spots[1:]:
        assert not np.isfinite(beauty[y + fb, x + fb]).all()
        clean[y + fb, x + fb, :4] = 0.5 * clean[y + fb, x + fb, 4]
    out = dn.denoise(W, H, fb, beauty, albedo, normal, iterations=it)
    ref = dn.denoise(W, H, fb, clean, albedo, normal, iterations=it)
    assert np.isfinite(out).all()
    # a changed pixel changes signal within 2 * step per pass and variance within 3 (window) + 1
    # (blur) more: everything farther away is untouched
    reach = 2 * ((1 << it) - 1) + 4
    yy, xx = np.mgrid[0:H, 0:W]
    far = np.ones((H, W), bool)
    for x, y in spots[1:]:
        far &= np.maximum(np.abs(xx - x), np.abs(yy - y)) > reach
    assert far.sum() > 100
    a, b = _rgb(out, fb)[far], _rgb(ref, fb)[far]
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # and near the bad pixels the result is the neighbourhood's, not zero
    for x, y in spots[1:]:
        assert (_rgb(out, fb)[y, x] > 0).all()


def test_noise_variance_drops_on_a_flat_region():
    W, H, fb = 40, 40, 2
    rng = np.random.default_rng(9)
    rgb = rng.gamma(4.0, 0.25, (H, W, 3)).astype(f32)
    one = np.ones((H, W), f32)
    n = np.zeros((H, W, 3), f32)
    n[..., 2] = 1
    imgs = dn.images_of(W, H, fb, rgb, one, np.full((H, W, 3), 0.5, f32), one, n, np.full((H, W), 3, f32))
    out = _rgb(dn.denoise(W, H, fb, *imgs), fb)
    inner = (slice(8, -8), slice(8, -8))
    assert out[inner].var() < 0.1 * rgb[inner].var()
    assert abs(float(out[inner].mean()) - float(rgb[inner].mean())) < 0.05


def test_coverage_term_stops_a_partially_covered_rim():
    """Pixels whose coverage differs by more than 8 * sigma_coverage exchange nothing, whatever
    their normals and depths: a bright half-covered rim does not bleed into its covered neighbours."""
    W, H, fb = 24, 12, 2
    one = np.ones((H, W), f32)
    cov = one.copy()
    cov[:, 10] = 0.5
    rgb = np.full((H, W, 3), 0.2, f32)
    rgb[:, 10] = 20.0
    n = np.zeros((H, W, 3), f32)
    n[..., 2] = 1
    imgs = dn.images_of(W, H, fb, rgb, one, np.full((H, W, 3), 0.5, f32) * cov[..., None], cov, n, np.full((H, W), 3, f32))
    out = _rgb(dn.denoise(W, H, fb, *imgs), fb)
    keep = np.ones(W, bool)
    keep[10] = False
    assert np.allclose(out[:, keep], 0.2, rtol=1e-5)


def test_defaults(built):
    from nart_amd import build as nb
    nb.build_hip_lib()
    dp = nart_amd.DenoiseParams.defaults()
    got = {k: getattr(dp, k) for k in dn.DEFAULTS}
    want = {k: (v if isinstance(v, int) else float(f32(v))) for k, v in dn.DEFAULTS.items()}
    assert got == want, got
    assert (dp.iterations, dp.normal_squarings, dp.sigma_color, dp.sigma_depth) == (5, 5, 4.0, 1.0)
    assert (dp.depth_eps, dp.sigma_coverage, dp.albedo_floor) == (float(f32(1e-3)), float(f32(0.05)), float(f32(0.01)))


def test_denoise_entry_points_reject_null_without_gpu(built):
    from nart_amd import build as nb
    nb.build_hip_lib()
    lib = nart_amd.hip_lib()
    p = nart_amd.default_params()
    buf = np.zeros((4, 4, 5), f32)  # never read: a null context is rejected first
    img = buf.ctypes.data
    assert lib.nart_hip_denoise(None, ctypes.byref(p), None, img, img, img, img, None) == -1  # NART_E_INVALID
    assert lib.nart_hip_render_denoised(None, ctypes.byref(p), None, None, img, None, None) == -1
    assert lib.nart_hip_denoise_timings(None, None, None, None, None) == -1
