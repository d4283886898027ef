"""The restatements behind the second-moment image and the denoiser's sample-variance mode
(tests/moment_py.py), validated without a GPU: the moment restatement against the oracle's
framebuffer (its filter weight sum) and against a float64 accumulation of its own terms; the moment
prepare on inputs whose variance is known; nart_amd.sample_variance against the restatement; and the
new entry points' argument checks."""
import ctypes

import numpy as np
import pytest

import denoise_py as dn
import moment_py as mp
import nart_amd
import oracle

f32 = np.float32
EPS = float(np.finfo(np.float32).eps)


def _params(scene, w, h, spp, **kw):
    p = nart_amd.load_sessions(scene.path)[0]
    p.image_width, p.image_height, p.spp = w, h, spp
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


@pytest.mark.parametrize("spp,kw", [(2, dict(bucket_size=16)), (3, dict(bucket_size=12, filter_width=1.0))],
                         ids=["b16_fw2_2spp", "b12_fw1_3spp"])
def test_moment_restatement_against_oracle_samples(glass_scene, spp, kw):
    """glassSphere 24x20 over the oracle's per-sample Li_alpha: the moment image's filter weight sum
    has the bits of the oracle's framebuffer, and every contribution channel agrees with a float64
    accumulation of the same float32 terms within the float32 summation bound
    n * eps * sum |term| (n additions into the pixel: its sample terms and its tiles; eps = 2^-23)."""
    p = _params(glass_scene, 24, 20, spp, **kw)
    g = nart_amd.session_geometry(p)
    orc = oracle.Oracle(glass_scene)
    L, uv = orc.render_samples(p, 0, 0, g.total_width, g.total_height, with_uv=True)
    M, M64, count, mag = mp.restate_moment(p, uv, L, with_bound=True)
    ref = orc.render(p)
    assert _bits_equal(M[..., 4], ref[..., 4])
    assert ref[..., 4].max() > 0 and M[..., :3].max() > 0 and np.isfinite(M).all()
    bound = count[..., None] * EPS * mag[..., :4]
    err = np.abs(M[..., :4].astype(np.float64) - M64[..., :4])
    assert (err <= bound).all(), float((err - bound).max())
    # sum w^2 <= (sum w)^2, and one sample's pixel-footprint worth of weight at least
    inside = M[..., 4] > 0
    assert (M[..., 3][inside] > 0).all() and (M[..., 3] <= M[..., 4] * M[..., 4] * (1 + 1e-6)).all()
    # the second moment dominates the squared mean (Cauchy-Schwarz), up to rounding
    with np.errstate(all="ignore"):
        mean = ref[..., :3][inside] / ref[..., 4][inside][:, None]
        m2 = M[..., :3][inside] / M[..., 4][inside][:, None]
    assert (m2 >= mean * mean * (1 - 1e-5)).all()


def _synthetic(W, H, fb, seed):
    (beauty, albedo, normal), spots = dn.synthetic(W, H, fb, seed=seed)
    moment, mspots = mp.synthetic_moment(W, H, fb, beauty, seed=seed)
    return beauty, albedo, normal, moment, spots, mspots


def test_moment_prepare_cases():
    W, H, fb = 37, 29, 2
    dp = dn.params_of()
    beauty, albedo, normal, moment, spots, mspots = _synthetic(W, H, fb, 5)
    st, V = mp.prepare(W, H, fb, beauty, albedo, normal, moment, dp)
    v = st["v"]
    (zx, zy), (cx, cy), (bx, by), (nx, ny) = mspots
    assert v[zy, zx] == 0 and not V[zy, zx].any()              # mw = 0
    assert v[cy, cx] == 0 and not V[cy, cx].any()              # M.ch / mw < c^2 clamps to 0
    assert v[by, bx] == f32(1e30) and v[ny, nx] == f32(1e30)   # 1e38, NaN: finite beauty there
    for (x, y) in spots[1:]:                                   # non-finite beauty: invalid, as in the spatial mode
        assert v[y, x] == -1 and not st["s"][y, x].any()
    spatial = dn.prepare(W, H, fb, beauty, albedo, normal, dp)
    assert np.array_equal(spatial["v"] < 0, v < 0)
    for key in ("n", "z", "cov", "s", "a_d", "alpha", "slope"):
        assert _bits_equal(st[key], spatial[key]), key
    ok = ~(v < 0)
    assert (v[ok] >= 0).all() and np.isfinite(v).all()
    out = mp.denoise(W, H, fb, beauty, albedo, normal, moment)
    assert np.isfinite(out).all()
    # sample_variance() is the restatement's V, bit for bit, and 0 where mw <= 0
    p = nart_amd.default_params()
    p.image_width, p.image_height, p.filter_width = W, H, float(fb)
    assert nart_amd.session_geometry(p).filter_bounds == fb
    sv = nart_amd.sample_variance(p, beauty, moment)
    assert sv.shape == (H, W, 4) and sv.dtype == f32
    assert _bits_equal(sv[..., :3], V)
    assert not sv[zy, zx].any()
    assert sv[H // 2 + 1, 3, 3] == f32(4)  # 1 / k: synthetic_moment's 4 equally weighted samples


def test_moment_prepare_constant_radiance():
    """Every sample of a pixel carrying the same radiance: M.ch / mw equals c^2 up to rounding, so
    v stays below 1e-6 l^2 (l the demodulated luminance)."""
    W, H, fb = 16, 9, 2
    rng = np.random.default_rng(3)
    (beauty, albedo, normal), _spots = dn.synthetic(W, H, fb, seed=9, bad_pixels=False)
    spp = 5
    w = rng.uniform(0.05, 1.0, (H, W, spp)).astype(f32)
    rad = rng.uniform(0.1, 3.0, (H, W, 3)).astype(f32)
    B = np.zeros((H, W, 5), f32)
    M = np.zeros((H, W, 5), f32)
    for s in range(spp):
        ws = w[..., s]
        B[..., :3] += rad * ws[..., None]
        B[..., 3] += f32(1) * ws
        B[..., 4] += ws
        M[..., :3] += (rad * rad) * ws[..., None]
        M[..., 3] += ws * ws
        M[..., 4] += ws
    moment = np.zeros_like(beauty)
    beauty[fb:fb + H, fb:fb + W] = B
    moment[fb:fb + H, fb:fb + W] = M
    st, _V = mp.prepare(W, H, fb, beauty, albedo, normal, moment, dn.params_of())
    l = dn.lum(st["s"])
    assert (l > 0).all() and (st["v"] >= 0).all()
    assert (st["v"] < 1e-6 * l * l).all(), float((st["v"] / (l * l)).max())


def test_moment_entry_points_reject_null_without_gpu(built):
    from nart_amd import build as nb
    nb.build_hip_lib()
    lib = nart_amd.hip_lib()
    p = nart_amd.default_params()
    buf = np.zeros(8, f32).ctypes.data
    assert lib.nart_hip_render_moment(None, ctypes.byref(p), 0, None, None, None, buf, None, None, None) == -1
    assert lib.nart_hip_denoise_moment(None, ctypes.byref(p), None, buf, buf, buf, buf, buf, None) == -1
    assert lib.nart_hip_render_denoised_moment(None, ctypes.byref(p), None, None, buf, None, None) == -1
