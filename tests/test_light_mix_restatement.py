"""The numpy restatement of the light-group mix (tests/lightgroup_py.py mix; include/nart_hip.h,
"Light groups": acc = 0.f; for g ascending: acc = acc + gains[g][c] * I_g[c]; alpha and filter weight sum
from image 0) against hand-computed cases, on the CPU.  The GPU test compares k_light_mix with it."""
import numpy as np
import pytest

import lightgroup_py as lg

f32 = np.float32


def _img(h, w, rgb, alpha=1.0, weight=2.0):
    a = np.empty((h, w, 5), f32)
    a[..., :3] = np.asarray(rgb, f32)
    a[..., 3] = alpha
    a[..., 4] = weight
    return a


def test_one_pixel_by_hand():
    I = np.stack([_img(1, 1, (1.0, 2.0, 3.0), 0.5, 7.0), _img(1, 1, (10.0, 20.0, 30.0), 0.25, 9.0)])
    out = lg.mix(I, [[1.0, 0.5, 0.0], [2.0, 0.0, -1.0]])
    assert out.dtype == f32 and out.shape == (1, 1, 5)
    assert out[0, 0].tolist() == [21.0, 1.0, -30.0, 0.5, 7.0]  # alpha and weight: image 0's
    # a scalar gain per group applies to r, g and b
    assert lg.mix(I, [2.0, 0.5])[0, 0].tolist() == [7.0, 14.0, 21.0, 0.5, 7.0]


def test_gains_zero_and_one():
    I = np.stack([_img(1, 1, (0.1, 0.2, 0.3)), _img(1, 1, (0.7, 0.8, 0.9))])
    assert lg.bits_equal(lg.mix(I, [1.0, 0.0])[..., :3], I[0][..., :3])  # 0 + 1 x = x, x + 0 y = x for finite y >= 0
    assert lg.bits_equal(lg.mix(I, [0.0, 1.0])[..., :3], I[1][..., :3])
    want = (f32(0.1) + f32(0.7), f32(0.2) + f32(0.8), f32(0.3) + f32(0.9))  # float32 sums, not float64
    assert lg.bits_equal(lg.mix(I, [1.0, 1.0])[0, 0, :3], np.array(want, f32))


def test_rounding_is_float32_and_unfused():
    # 1 + 3 * 2^-24: the product rounds to 3 * 2^-24, the sum 1 + 3 * 2^-24 rounds to 1 + 2^-22 (ties to
    # even); a fused multiply-add of (1 + 2^-23) * (1 - 2^-23) + (-1) would keep -2^-46, unfused gives 0
    a, b = f32(1.0) + f32(2.0 ** -23), f32(1.0) - f32(2.0 ** -23)
    I = np.stack([_img(1, 1, (a, 1.0, 0.0)), _img(1, 1, (1.0, 0.0, 0.0))])
    out = lg.mix(I, [[b, 1.0, 1.0], [-1.0, 1.0, 1.0]])
    assert out[0, 0, 0] == 0.0  # RN(a b) = 1 exactly
    I2 = np.stack([_img(1, 1, (1.0, 0.0, 0.0)), _img(1, 1, (f32(2.0 ** -24), 0.0, 0.0))])
    assert lg.mix(I2, [[1.0, 1, 1], [3.0, 1, 1]])[0, 0, 0] == f32(1.0) + f32(2.0 ** -22)


def test_order_is_ascending():
    big = f32(2.0 ** 24)
    I = np.stack([_img(1, 1, (big, 0, 0)), _img(1, 1, (1.0, 0, 0)), _img(1, 1, (1.0, 0, 0)), _img(1, 1, (-big, 0, 0))])
    assert lg.mix(I, [1.0, 1.0, 1.0, 1.0])[0, 0, 0] == 0.0       # ((2^24 + 1) + 1) - 2^24: each 1 is absorbed
    assert lg.mix(I[[1, 2, 0, 3]], [1.0, 1.0, 1.0, 1.0])[0, 0, 0] == 2.0  # (1 + 1 + 2^24) - 2^24


def test_negative_zero():
    nz = f32(-0.0)
    I = np.stack([_img(1, 1, (nz, 1.0, nz))])
    out = lg.mix(I, [[1.0, nz, -1.0]])
    # acc starts at +0: +0 + (-0) = +0; 1 * -0 = -0 and +0 + -0 = +0; -0 * -1 = +0
    assert lg.bits(out[0, 0, :3]).tolist() == [0, 0, 0]
    I = np.stack([_img(1, 1, (-1.0, 0, 0)), _img(1, 1, (1.0, 0, 0))])
    assert lg.bits(lg.mix(I, [1.0, 1.0])[0, 0, :1]).tolist() == [0]  # -1 + 1 = +0 (round to nearest)


def test_inf_and_nan_in_the_images():
    inf, nan = f32(np.inf), f32(np.nan)
    I = np.stack([_img(1, 3, (1.0, 1.0, 1.0)), _img(1, 3, (2.0, 2.0, 2.0))])
    I[0, 0, 0, 0] = inf      # pixel 0, r: inf
    I[1, 0, 1, 1] = nan      # pixel 1, g of group 1: NaN
    I[0, 0, 2, 2] = inf      # pixel 2, b: inf - inf
    I[1, 0, 2, 2] = inf
    I[0, 0, 1, 3] = nan      # alpha NaN is copied
    out = lg.mix(I, [[1.0, 1.0, 1.0], [1.0, 1.0, -1.0]])
    assert out[0, 0, 0] == inf and out[0, 0, 1] == 3.0
    assert np.isnan(out[0, 1, 1]) and out[0, 1, 0] == 3.0 and np.isnan(out[0, 1, 3])
    assert np.isnan(out[0, 2, 2])
    zero = lg.mix(I, [[0.0, 1.0, 1.0], [1.0, 0.0, 1.0]])
    assert np.isnan(zero[0, 0, 0])   # 0 * inf: a gain of 0 does not switch an infinite group off
    assert np.isnan(zero[0, 1, 1])   # nor a NaN one
    assert zero[0, 1, 0] == 2.0


@pytest.mark.parametrize("w,h,fb", [(1, 1, 0), (50, 37, 2)])
def test_whole_images_against_a_scalar_loop(w, h, fb):
    """Every pixel of the total image, the filter's border included, against the definition written as a
    scalar loop over float32 values."""
    rng = np.random.RandomState(11)
    H, W, G = h + 2 * fb, w + 2 * fb, 3
    I = rng.standard_normal((G, H, W, 5)).astype(f32)
    I[:, 0, 0, :3] = 0.0
    gains = rng.uniform(-2, 2, (G, 3)).astype(f32)
    out = lg.mix(I, gains)
    want = np.empty((H, W, 5), f32)
    for y in range(H):
        for x in range(W):
            for c in range(3):
                acc = f32(0.0)
                for g in range(G):
                    acc = f32(acc + f32(gains[g, c] * I[g, y, x, c]))
                want[y, x, c] = acc
            want[y, x, 3:] = I[0, y, x, 3:]
    assert lg.bits_equal(out, want), lg.report(out, want)
    assert out.shape == (H, W, 5)
