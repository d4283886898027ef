"""The restatement behind the firefly cascade (tests/cascade_py.py), validated without a GPU: the
split on hand-made samples; the layer images over the oracle's per-sample Li_alpha against the
oracle's framebuffer; the reweighting on synthetic layer images whose weights are known; and the new
entry points' argument checks and defaults."""
import ctypes

import numpy as np
import pytest

import cascade_py as cp
import nart_amd
import oracle

f32 = np.float32
EPS = float(np.finfo(np.float32).eps)
# the tests' parameters: eight layers from 2^-7 to 2^7, so that glassSphere's samples (median
# luminance about 0.006, fireflies near 260) reach every layer and pass the top one
TEST = dict(start=2.0 ** -7, base=4.0, layers=8)
# glassSphere's luminances are bimodal (few samples lie between 8 and the fireflies): at 24 x 20 no
# configuration reaches all eight layers; of the sizes up to 48 x 40 in steps of 4, 24 x 40 is the
# smallest at which both configurations below do (the test asserts it)
SIZE = (24, 40)


def _params(scene, w, h, spp, **kw):
    p = nart_amd.load_sessions(scene.path)[0]
    p.image_width, p.image_height, p.spp = w, h, spp
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _bits_equal(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------- 1. the split
def test_levels_and_defaults(built):
    from nart_amd import build as nb
    nb.build_hip_lib()
    d = nart_amd.CascadeParams.defaults()
    assert (d.layers, d.start, d.base, d.kappa) == (6, 1.0, 8.0, 2.0)
    assert _bits_equal(nart_amd.cascade_levels(), cp.levels_of(1, 8, 6))
    assert nart_amd.cascade_levels().tolist() == [1, 8, 64, 512, 4096, 32768]
    t = nart_amd.CascadeParams.defaults(**TEST)
    assert _bits_equal(nart_amd.cascade_levels(t), cp.levels_of(**TEST))
    odd = nart_amd.CascadeParams.defaults(start=0.3, base=2.7, layers=5)
    assert _bits_equal(nart_amd.cascade_levels(odd), cp.levels_of(0.3, 2.7, 5))


def test_split_hand_made_samples():
    levels = cp.levels_of(**TEST)
    K, base = len(levels), TEST["base"]
    up = lambda v: np.nextafter(f32(v), f32(np.inf))
    cases = []  # (record, the layers that may be non-zero, the layer that takes it whole or None)
    # a grey's luminance is not exactly its level; records with l exactly on a level: green only,
    # scaled so that 0.7152 * g rounds to the level (checked below)
    def on_level(b):
        g = f32(b) / cp.LG
        for cand in (g, np.nextafter(g, f32(0)), up(g)):
            rec = np.array([0, cand, 0, 0.25], f32)
            if cp.lum(rec) == f32(b):
                return rec
        raise AssertionError("no green with luminance %r" % b)
    def above(b):
        rec = on_level(b).copy()
        while not cp.lum(rec) > f32(b):
            rec[1] = up(rec[1])
        return rec
    cases.append((on_level(levels[0]), {0}, 0))                 # l == b_0: whole to layer 0
    cases.append((above(levels[0]), {0, 1}, None))              # just above: almost all of it in layer 0
    cases.append((on_level(levels[3]), {2, 3}, None))           # an inner level: w_lo = 0, w_hi = 1
    cases.append((above(levels[3]), {3, 4}, None))
    cases.append((on_level(levels[K - 1]), {K - 2, K - 1}, None))
    cases.append((above(levels[K - 1]), {K - 1}, K - 1))        # above the top: whole to layer K-1
    cases.append((np.array([900, 700, 800, 1], f32), {K - 1}, K - 1))
    cases.append((np.zeros(4, f32), {0}, 0))                    # l = 0
    cases.append((np.array([np.nan, 1, 1, 1], f32), {0}, 0))    # not finite: whole to layer 0
    cases.append((np.array([1, np.inf, 1, 1], f32), {0}, 0))
    cases.append((np.array([-3, -3, -3, 1], f32), {0}, 0))      # negative luminance
    L = np.stack([c[0] for c in cases])
    out = cp.split(L, levels, base)
    w, whole, part = cp.split_weights(L, levels, base)
    assert out.shape == (K, len(cases), 4)
    assert ((w >= 0) & (w <= 1)).all()
    for i, (rec, may, takes) in enumerate(cases):
        for k in range(K):
            if k not in may:
                assert not _bits(out[k, i]).any(), (i, k)       # exactly +0
        if takes is not None:
            assert _bits_equal(out[takes, i], rec), i
        else:
            lo, hi = sorted(may)
            assert part[lo, i] and part[hi, i]
            assert w[hi, i] == f32(1) - w[lo, i]
            total = out[lo, i].astype(np.float64) + out[hi, i].astype(np.float64)
            assert np.allclose(total, rec.astype(np.float64), rtol=4 * EPS, atol=0), i
    # on an inner level and on the top one the upper layer has weight exactly 1
    assert w[3, 2] == 1 and w[2, 2] == 0 and w[K - 1, 4] == 1 and w[K - 2, 4] == 0
    assert 0 < w[1, 1] < 1e-6 and 0 < w[4, 3] < 1e-6
    # sum_j w_j * l / b_j = 1: a layer's brightness reads as a sample count
    l = cp.lum(L[3]).astype(np.float64)
    assert abs(sum(float(w[k, 3]) * l / float(levels[k]) for k in range(K)) - 1) < 1e-5


# ---------------------------------------------------------------- 2. the layers over the oracle's samples
@pytest.mark.parametrize("spp,kw", [(3, dict(bucket_size=16)), (2, dict(bucket_size=12, filter_width=1.0))],
                         ids=["b16_fw2_3spp", "b12_fw1_2spp"])
def test_layers_against_oracle_samples(glass_scene, spp, kw):
    """glassSphere over the oracle's per-sample Li_alpha with the test parameters: every layer's
    filter weight sum has the bits of the oracle's framebuffer, and the sum of the layers agrees with
    the oracle's contributions within the float32 summation bound n * eps * sum |term| (eps = 2^-23).
    n counts the additions into the pixel's layer sum: one per (sample, layer) term of a layer the
    sample reaches, one per tile per layer, one per layer.  With m samples from t tiles touching the
    pixel that is at least m + 8 t + 8, against the oracle's own m + t additions: each side's
    summation error is at most half its count times eps * sum |term|, and the split adds at most
    3/2 eps per term (w_hi = 1 - w_lo is off by eps / 2 at most, and two products round), so
    (n + m + t + 3) / 2 <= n covers both."""
    p = _params(glass_scene, SIZE[0], SIZE[1], spp, **kw)
    g = nart_amd.session_geometry(p)
    orc = oracle.Oracle(glass_scene)
    L, uv = orc.render_samples(p, 0, 0, g.total_width, g.total_height, with_uv=True)
    levels = cp.levels_of(**TEST)
    K = len(levels)
    # the condition the GPU tests rest on: every layer receives a sample, one lies above the top level
    w, whole, part = cp.split_weights(L, levels, TEST["base"])
    reached = [(int(((whole[k] | part[k]) & (w[k] > 0)).sum())) for k in range(K)]
    lm = cp.lum(L)
    print("samples per layer", reached, "above the top level", int((lm > levels[-1]).sum()), "median l",
          float(np.median(lm)), "max l", float(lm.max()))
    assert all(n >= 1 for n in reached), reached
    assert (lm > levels[-1]).any()
    assert np.isfinite(L).all()
    images, mag, count = cp.restate_layers(p, uv, L, levels, TEST["base"], with_bound=True)
    ref = orc.render(p)
    for k in range(K):
        assert _bits_equal(images[k][..., 4], ref[..., 4]), k
    total = images[0][..., :4].copy()
    for k in range(1, K):  # in float32, layer by layer, as the reweighting adds them
        total = (total + images[k][..., :4]).astype(f32)
    total = total.astype(np.float64)
    bound = count[..., None] * EPS * mag
    err = np.abs(total - ref[..., :4].astype(np.float64))
    assert (err <= bound).all(), float((err - bound).max())
    assert ref[..., :3].max() > 0 and all(images[k][..., :3].max() > 0 for k in range(K))


# ---------------------------------------------------------------- 3. the reweighting
def _frame(W, H, fb, K, Wt=1.0):
    beauty = np.zeros((H + 2 * fb, W + 2 * fb, 5), f32)
    layers = np.zeros((K,) + beauty.shape, f32)
    beauty[fb:fb + H, fb:fb + W, 3:] = Wt
    layers[:, fb:fb + H, fb:fb + W, 4] = Wt
    return beauty, layers


def test_reweight_constant_region_is_trusted():
    W, H, fb, spp, kappa = 9, 7, 2, 4, 2.0
    levels = cp.levels_of(1, 4, 4)
    for j in (1, 2, 3):
        beauty, layers = _frame(W, H, fb, 4, Wt=2.0)
        # the mean of layer j is b_j * kappa / spp in every pixel: N * lambda / b_j = kappa
        layers[j, fb:fb + H, fb:fb + W, :3] = f32(2.0) * f32(levels[j] * kappa / spp) * f32(1.001)
        beauty[..., :3] = layers[:, ..., :3].sum(axis=0)
        m, omega, ok = cp.weights_of(W, H, fb, beauty, layers, levels, spp, kappa)
        assert ok.all() and (omega[j] == 1).all()
        out = cp.reweight(W, H, fb, beauty, layers, levels, spp, kappa)
        assert _bits_equal(out[fb:fb + H, fb:fb + W, :3], m[j]) and (out[fb:fb + H, fb:fb + W, 3:] == 1).all()
        assert not out[:fb].any() and not out[:, :fb].any() and not out[-fb:].any() and not out[:, -fb:].any()


@pytest.mark.parametrize("where,cnt", [((4, 3), 9), ((0, 0), 4), ((8, 0), 4), ((3, 0), 6), ((0, 2), 6), ((8, 6), 4)],
                         ids=["interior", "corner", "corner_x", "edge_top", "edge_left", "corner_xy"])
def test_reweight_single_lit_pixel(where, cnt):
    """One lit pixel in layer j with N * lambda / b_j = 1 and empty neighbours: omega_j there is
    (1 / cnt) / kappa, cnt the taps inside the image: 9, 6 at an edge, 4 at a corner."""
    W, H, fb, spp, kappa, j = 9, 7, 2, 4, 2.0, 2
    levels = cp.levels_of(1, 4, 4)
    beauty, layers = _frame(W, H, fb, 4)
    x, y = where
    mean = np.array([4, 4, 4], f32)  # b_2 / spp = 16 / 4, luminance 4 up to rounding
    layers[j, y + fb, x + fb, :3] = mean
    beauty[y + fb, x + fb, :3] = mean
    m, omega, ok = cp.weights_of(W, H, fb, beauty, layers, levels, spp, kappa)
    lam = cp.lum(mean)
    want = f32(f32(f32(f32(lam * f32(spp)) / levels[j]) / f32(cnt)) / f32(kappa))
    assert omega[j, y, x] == want and abs(float(want) - 1.0 / cnt / kappa) < 1e-6
    # the neighbouring layers see the same samples in their own level's units
    assert omega[j + 1, y, x] == f32(f32(f32(f32(lam * f32(spp)) / levels[j + 1]) / f32(cnt)) / f32(kappa))
    out = cp.reweight(W, H, fb, beauty, layers, levels, spp, kappa)
    assert _bits_equal(out[y + fb, x + fb, :3], (want * mean).astype(f32))
    assert np.count_nonzero(out[..., :3]) == 3


def test_reweight_synthetic_properties():
    W, H, fb, spp = 37, 29, 2, 4
    levels = cp.levels_of(**TEST)
    K = len(levels)
    beauty, layers, (zero_xy, nan_xy) = cp.synthetic(W, H, fb, levels, spp, seed=3)
    out = cp.reweight(W, H, fb, beauty, layers, levels, spp, 2.0)
    crop = out[fb:fb + H, fb:fb + W]
    # W = 0 gives a zero pixel, weight included
    assert not out[zero_xy[1] + fb, zero_xy[0] + fb].any()
    # kappa = 1e-30: every weight that matters is 1 and the output is the ordered sum of the m_j
    m, omega, ok = cp.weights_of(W, H, fb, beauty, layers, levels, spp, 1e-30)
    assert ((omega == 1) | (cp.lum(m) == 0) | ~np.isfinite(cp.lum(m))).all()
    plain = cp.reweight(W, H, fb, beauty, layers, levels, spp, 1e-30)
    with np.errstate(all="ignore"):
        ordered = m[0].copy()
        for j in range(1, K):
            ordered = (ordered + m[j]).astype(f32)
    ordered = np.where(ok[..., None], ordered, 0).astype(f32)
    assert _bits_equal(plain[fb:fb + H, fb:fb + W, :3], ordered)
    # rgb never exceeds the ordered sum of the non-negative m_j
    fin = np.isfinite(ordered).all(axis=-1)
    assert (m[:, fin] >= 0).all() and (crop[..., :3][fin] <= ordered[fin]).all()
    assert (crop[..., :3][fin] < ordered[fin]).any()  # and the reweighting does something here
    # a NaN layer pixel stays within its own 3x3 reach
    nx, ny = nan_xy
    assert np.isnan(crop[ny, nx, 1])
    clean = layers.copy()
    clean[1, ny + fb, nx + fb, 1] = 1.0
    ref = cp.reweight(W, H, fb, beauty, clean, levels, spp, 2.0)
    far = np.ones((H, W), bool)
    far[ny - 1:ny + 2, nx - 1:nx + 2] = False
    assert np.isfinite(ref).all()
    assert _bits_equal(crop[far], ref[fb:fb + H, fb:fb + W][far])
    assert np.isfinite(crop[far]).all()


# ---------------------------------------------------------------- 4. arguments
BAD = [dict(layers=1), dict(layers=9), dict(start=0.0), dict(start=-1.0), dict(start=float("nan")),
       dict(start=float("inf")), dict(base=1.0), dict(base=0.5), dict(base=float("nan")), dict(base=float("inf")),
       dict(kappa=0.0), dict(kappa=-2.0), dict(kappa=float("nan")), dict(kappa=float("inf")),
       dict(start=1e30, base=1e3, layers=4),   # a level overflows
       dict(start=1e-45, base=1.25, layers=3)]  # the levels do not increase


def test_cascade_entry_points_reject_bad_arguments_without_gpu(built):
    from nart_amd import build as nb
    nb.build_hip_lib()
    lib = nart_amd.hip_lib()
    p = nart_amd.default_params()
    buf = np.zeros(8, f32).ctypes.data
    n, lv = ctypes.c_uint32(), (ctypes.c_float * 8)()
    assert lib.nart_hip_cascade_levels(None, lv, ctypes.byref(n)) == 0 and n.value == 6
    assert lib.nart_hip_cascade_levels(None, None, ctypes.byref(n)) == 0 and n.value == 6
    assert lib.nart_hip_cascade_levels(None, lv, None) == -1
    for kw in BAD:
        c = nart_amd.CascadeParams.defaults(**kw)
        assert lib.nart_hip_cascade_levels(ctypes.byref(c), lv, ctypes.byref(n)) == -1, kw
        with pytest.raises(nart_amd.NartError):
            nart_amd.cascade_levels(c)
        assert lib.nart_hip_render_cascade(None, ctypes.byref(p), ctypes.byref(c), buf, None, None, None) == -1, kw
        assert lib.nart_hip_cascade_reweight(None, ctypes.byref(p), ctypes.byref(c), buf, buf, buf) == -1, kw
    assert lib.nart_hip_render_cascade(None, ctypes.byref(p), None, buf, None, None, None) == -1
    assert lib.nart_hip_cascade_reweight(None, ctypes.byref(p), None, buf, buf, buf) == -1
    assert lib.nart_hip_cascade_timings(None, None, None) == -1
