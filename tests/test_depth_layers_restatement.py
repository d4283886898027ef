"""depthcut_py.layers, the numpy restatement the device's k_depth_layers is compared with, against its own
definition (include/nart_hip.h, "Depth cuts"): layer_0 is I_0, every other layer one float32 subtraction
computed element by element here, alpha and filter weight sum the beauty's; and summed ascending the
layers meet the beauty within the bound derived in layers' docstring from the K subtractions and K
additions -- no measured tolerance."""
import numpy as np
import pytest

import depthcut_py as dc

f32 = np.float32


def _images(rng, K, h=9, w=11, ascending=False):
    I = rng.standard_normal((K + 1, h, w, 5)).astype(f32)
    I *= f32(10.0) ** rng.randint(-6, 7, I.shape).astype(f32)
    if ascending:  # what rendered cuts look like: non-negative and growing with the depth
        I[..., :3] = np.cumsum(np.abs(I[..., :3]), axis=0, dtype=f32)
    return I[:K], I[K]


@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_layers_are_single_subtractions(K):
    rng = np.random.RandomState(K)
    I, B = _images(rng, K)
    L = dc.layers(I, B)
    assert L.shape == (K + 1,) + B.shape and L.dtype == f32
    assert dc.bits_equal(L[0][..., :3], I[0][..., :3])  # layer_0 is I_0
    upper = list(I[1:]) + [B]
    for j in range(1, K + 1):
        for y, x, c in ((0, 0, 0), (4, 7, 1), (8, 10, 2), (3, 3, 0)):
            assert L[j][y, x, c].tobytes() == f32(f32(upper[j - 1][y, x, c]) - f32(I[j - 1][y, x, c])).tobytes()
    for j in range(K + 1):
        assert dc.bits_equal(L[j][..., 3:], B[..., 3:])  # alpha and filter weight sum: the beauty's


def test_signed_zero_and_special_values():
    I = np.zeros((2, 1, 4, 5), f32)
    B = np.zeros((1, 4, 5), f32)
    I[0, 0, :, 0] = [-0.0, 0.0, np.inf, 1e-45]
    I[1, 0, :, 0] = [-0.0, 1.0, np.inf, 3e-45]
    B[0, :, 0] = [0.0, 1.0, np.nan, 3e-45]
    L = dc.layers(I, B)
    assert np.signbit(L[0][0, 0, 0])            # layer_0 copies -0
    assert L[1][0, 1, 0] == 1 and np.isnan(L[1][0, 2, 0]) and np.isnan(L[2][0, 2, 0])
    assert L[1][0, 3, 0] == f32(3e-45) - f32(1e-45) and L[2][0, 3, 0] == 0  # denormals subtract exactly


@pytest.mark.parametrize("K", [1, 2, 5, 8])
@pytest.mark.parametrize("ascending", [False, True])
def test_layers_sum_back_to_the_beauty(K, ascending):
    rng = np.random.RandomState(100 + K)
    I, B = _images(rng, K, 64, 64, ascending)
    err = np.abs(dc.layers_sum(dc.layers(I, B)).astype(np.float64) - B[..., :3])
    bound = dc.layers_bound(I, B)
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    if K > 1 and not ascending:
        assert err.max() > 0  # (the bound is not vacuous: rounding does happen)
