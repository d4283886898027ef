"""The restatement behind the cross-filtered denoiser (tests/denoise_cross_py.py), validated without a
GPU: the symmetry in the halves, identical halves against the plain restatement, the border, the invalid
pixels, and the entry points' argument checks -- on synthetic images and on half buffers restated over
the oracle's per-sample Li_alpha (glassSphere 16 x 12, with flat guides: the CPU has no AOV frame)."""
import ctypes

import numpy as np
import pytest

import denoise_cross_py as dx
import denoise_py as dn
import halves_py as hp
import nart_amd
import oracle
from test_aov_restatement import restate_render

f32 = np.float32
SIZES = [(1, 1), (5, 3), (37, 29)]


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _bits_equal(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _crop(im, W, H, fb):
    return im[fb:fb + H, fb:fb + W]


# ---------------------------------------------------------------- 1. symmetry, border, invalid pixels
@pytest.mark.parametrize("iterations", [1, 5])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_swapping_the_halves_changes_no_bit(size, iterations):
    W, H = size
    fb = 2
    (ha, hb, beauty, alb, nrm), spots = dx.synthetic(W, H, fb, seed=W * 131 + H)
    out, err = dx.denoise(W, H, fb, ha, hb, beauty, alb, nrm, iterations=iterations)
    out2, err2 = dx.denoise(W, H, fb, hb, ha, beauty, alb, nrm, iterations=iterations)
    assert _bits_equal(out, out2) and _bits_equal(err, err2)
    # the border is zero and the weight is 1, in both images
    border = np.ones(out.shape[:2], bool)
    border[fb:fb + H, fb:fb + W] = False
    for im in (out, err):
        assert not im[border].any() and (im[~border][:, 4] == 1).all()
    assert _bits_equal(out[..., 3], err[..., 3])
    e = _crop(err, W, H, fb)[..., :3]
    assert (e[np.isfinite(e)] >= 0).all()
    if W * H >= 15:
        assert None not in spots and (e > 0).any()


def test_prepare_marks_the_invalid_pixels():
    W, H, fb = 37, 29, 2
    (ha, hb, beauty, alb, nrm), spots = dx.synthetic(W, H, fb, seed=5)
    with np.errstate(all="ignore"):
        st = dx.prepare(W, H, fb, ha, hb, beauty, alb, nrm, dn.params_of())
    bad = np.zeros((H, W), bool)
    for (x, y) in spots:  # no weight at all, a NaN and an Inf half, a half without weight, an Inf half
        bad[y, x] = True
    assert np.array_equal(st["v"][0] < 0, bad) and _bits_equal(st["v"][0], st["v"][1])
    assert not st["s"][:, bad].any()
    # v = 0.5 d^2 with d the halves' luminance difference
    d = dn.lum(st["s"][0]) - dn.lum(st["s"][1])
    assert _bits_equal(st["v"][0][~bad], (f32(0.5) * (d * d))[~bad])
    # one pass fills an invalid pixel from its valid neighbours, in both halves; the invalid pixel itself
    # is never averaged, so nothing non-finite spreads
    out, err = dx.denoise(W, H, fb, ha, hb, beauty, alb, nrm, iterations=1)
    assert np.isfinite(out).all() and np.isfinite(err).all()


def test_a_pixel_left_invalid_gets_the_beauty_and_no_error():
    """Half 1 without weight anywhere: no pixel is ever valid, the output is the beauty's mean (0 where
    the beauty has no weight either) and the error image is 0 but for alpha and the weight."""
    W, H, fb = 5, 3, 1
    (ha, hb, beauty, alb, nrm), spots = dx.synthetic(W, H, fb, seed=2, bad_pixels=False)
    hb = hb.copy()
    hb[..., :4] = 0
    out, err = dx.denoise(W, H, fb, ha, hb, beauty, alb, nrm, iterations=3)
    c = _crop(beauty, W, H, fb)
    with np.errstate(all="ignore"):
        mean = np.where((c[..., 4] > 0)[..., None], c[..., :4] / c[..., 4:5], 0).astype(f32)
    assert _bits_equal(_crop(out, W, H, fb)[..., :4], mean)
    assert not _crop(err, W, H, fb)[..., :3].any()
    (zx, zy) = spots[0]
    assert not _crop(out, W, H, fb)[zy, zx, :4].any()


# ---------------------------------------------------------------- 2. identical halves
@pytest.mark.parametrize("iterations", [1, 5])
def test_identical_halves_give_the_plain_filter_at_variance_zero(iterations):
    """With H_0 = H_1 = H: d = 0 and v = 0 in every valid pixel and stay 0 (sv sums w^2 * 0), both halves
    run the same sums, (s + s) * 0.5 = s and s - s = 0 exactly.  So the error is exactly 0, and out.rgb
    has the bits of the plain restatement's prepare, a-trous passes and finalise at variance 0 (its
    variance pass left out) over a beauty whose mean is H's: {H.rgb, ., H[3]}.  Where the plain filter
    leaves a pixel invalid it writes 0 and the cross filter the beauty's mean: compared where valid."""
    W, H, fb = 37, 29, 2
    (ha, _hb, beauty, alb, nrm), spots = dx.synthetic(W, H, fb, seed=9)
    as_beauty = ha.copy()
    as_beauty[..., 4] = ha[..., 3]
    as_beauty[..., 3] = ha[..., 3] * f32(0.25)  # some alpha
    out, err = dx.denoise(W, H, fb, ha, ha, as_beauty, alb, nrm, iterations=iterations)
    plain, st = dx.plain_without_variance(W, H, fb, as_beauty, alb, nrm, iterations=iterations)
    valid = ~(st["v"] < 0)
    assert valid.mean() > 0.9
    assert not _crop(err, W, H, fb)[..., :3].any()
    assert _bits_equal(_crop(out, W, H, fb)[valid][:, :3], _crop(plain, W, H, fb)[valid][:, :3])
    assert _bits_equal(out[..., 3:], plain[..., 3:])
    # and it is not the plain denoiser with its spatial variance estimate
    full = dn.denoise(W, H, fb, as_beauty, alb, nrm, iterations=iterations)
    assert not _bits_equal(full, plain)


# ---------------------------------------------------------------- 3. rendered halves
def _flat_guides(p):
    g = nart_amd.session_geometry(p)
    W, H, fb = p.image_width, p.image_height, g.filter_bounds
    one = np.ones((H, W), f32)
    n = np.zeros((H, W, 3), f32)
    n[..., 2] = 1
    _b, alb, nrm = dn.images_of(W, H, fb, np.zeros((H, W, 3), f32), one, np.ones((H, W, 3), f32) * f32(0.5), one, n,
                                one * f32(3))
    return alb, nrm


@pytest.mark.parametrize("spp", [1, 2, 5, 8])
def test_rendered_halves(glass_scene, spp):
    """Half buffers over the oracle's samples, bucket size not dividing the width.  At spp 1 half 1 is
    empty and every pixel stays invalid: the beauty's mean, error 0.  From 2 spp on the filter runs and
    leaves finite images and a positive error somewhere; at every count swapping changes no bit."""
    p = nart_amd.load_sessions(glass_scene.path)[0]
    p.image_width, p.image_height, p.spp, p.bucket_size = 16, 12, spp, 12
    g = nart_amd.session_geometry(p)
    W, H, fb = 16, 12, g.filter_bounds
    assert g.total_width % p.bucket_size
    orc = oracle.Oracle(glass_scene)
    L, uv = orc.render_samples(p, 0, 0, g.total_width, g.total_height, with_uv=True)
    beauty = restate_render(p, uv, L)
    halves = hp.restate_halves(p, uv, L)
    alb, nrm = _flat_guides(p)
    out, err = dx.denoise(W, H, fb, halves[0], halves[1], beauty, alb, nrm)
    out2, err2 = dx.denoise(W, H, fb, halves[1], halves[0], beauty, alb, nrm)
    assert _bits_equal(out, out2) and _bits_equal(err, err2)
    c = _crop(beauty, W, H, fb)
    mean = (c[..., :3] / c[..., 4:5]).astype(f32)
    if spp == 1:
        assert _bits_equal(_crop(out, W, H, fb)[..., :3], mean) and not _crop(err, W, H, fb)[..., :3].any()
        return
    assert np.isfinite(out).all() and np.isfinite(err).all()
    assert not _bits_equal(_crop(out, W, H, fb)[..., :3], mean)
    assert (_crop(err, W, H, fb)[..., :3] > 0).any()


# ---------------------------------------------------------------- 4. arguments
def test_cross_entry_points_reject_bad_arguments_without_gpu(built):
    from nart_amd import build as nb
    nb.build_hip_lib()
    lib = nart_amd.hip_lib()
    p = nart_amd.default_params()
    x = np.zeros(8, f32)
    d = x.ctypes.data
    P = ctypes.byref(p)
    assert lib.nart_hip_denoise_cross(None, P, None, d, d, d, d, d, d, d, None) == -1
    assert lib.nart_hip_render_denoised_cross(None, P, None, None, d, d, None, None, None) == -1
    assert lib.nart_hip_denoise_cross_timings(None, None, None, None, None) == -1
    fake = ctypes.c_void_p(d)  # never dereferenced: every call below fails on a null argument
    assert lib.nart_hip_denoise_cross(fake, None, None, d, d, d, d, d, d, d, None) == -1
    for k in range(6):  # a null input or output image; the error image alone may be null
        args = [d] * 6
        args[k] = None
        assert lib.nart_hip_denoise_cross(fake, P, None, *args, d, None) == -1, k
    assert lib.nart_hip_render_denoised_cross(fake, P, None, None, None, d, None, None, None) == -1
    assert lib.nart_hip_render_denoised_cross(fake, P, None, None, d, None, None, None, None) == -1
    assert not x.any()
