"""The fused restatement of the parts denoise (tests/denoise_parts_py.py: shared w_n and d_g per offset,
per-part d_l) against the denoiser's own restatement run on every part alone (tests/denoise_py.py), bit
for bit, on the CPU; and that the designed inputs hold what they are designed to hold.

The inputs cannot hold everything at every size and K: a 1 x 1 image has one pixel, and the roles of the
parts (denoise_parts_py.ROLES) are fixed by their index, so K = 1 has only the plain part.  Each property is
therefore asserted wherever the size and K allow it, which is written next to it; K = 5 and 9 on 70 x 3
and 37 x 29 hold all of them."""
import numpy as np
import pytest

import denoise_parts_py as dnp
import denoise_py as dn

f32 = np.float32
SIZES = [(1, 1), (5, 3), (70, 3), (37, 29)]
FB = 2


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_designed(W, H, fb, parts, albedo, normal, outs=None):
    """Asserts what the designed inputs contain; returns the per-part validity masks."""
    K = len(parts)
    dp = dn.params_of()
    with np.errstate(all="ignore"):
        sh = dnp.prepare_shared(W, H, fb, albedo, normal, dp)
        valid = np.stack([~(dnp.prepare_part(W, H, fb, p, sh["a_d"])["v"] < 0) for p in parts])
    assert (sh["z"] == 0).any(), "an empty-guide region"
    e = dnp.everywhere(W, H)
    if e is not None:  # (W * H >= 15)
        assert not valid[:, e[1], e[0]].any(), "a pixel invalid in every part"
    if K >= 2 and W * H >= 64:
        mixed = valid.any(0) & ~valid.all(0)
        assert int(mixed.sum()) >= 8, "at least 8 pixels valid in one part and invalid in another"
        crop = parts[:, fb:fb + H, fb:fb + W, :3]
        assert np.isnan(crop).any() and np.isinf(crop).any()
    if K >= 3:
        assert not valid[2].any(), "one part wholly invalid"
    if K >= 4:
        z = np.array(parts[3], copy=True)
        if e is not None:
            z[fb + e[1], fb + e[0]] = 0
        assert not z.any(), "one all-zero part"
    if outs is not None and K >= 2 and W * H >= 15:
        differ = (_bits(outs[0]) != _bits(outs[1]))[fb:fb + H, fb:fb + W].any(-1)
        assert differ.mean() > 0.5, "two parts whose outputs differ in more than half the crop"
    return valid


@pytest.mark.parametrize("iterations", [1, 5])
@pytest.mark.parametrize("K", [1, 2, 5, 9])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_fused_restatement_equals_the_denoiser_per_part(size, K, iterations):
    W, H = size
    parts, albedo, normal = dnp.synthetic_parts(W, H, FB, K, seed=W * 131 + H)
    got = dnp.denoise_parts(W, H, FB, parts, albedo, normal, iterations=iterations)
    assert got.shape == (K, H + 2 * FB, W + 2 * FB, 5)
    for k in range(K):
        want = dn.denoise(W, H, FB, parts[k], albedo, normal, iterations=iterations)
        ne = _bits(got[k]) != _bits(want)
        assert not ne.any(), (k, dnp.ROLES[k], int(ne.sum()), np.argwhere(ne)[:4].tolist())
    check_designed(W, H, FB, parts, albedo, normal, got)
    assert np.isfinite(got).all()  # no invalid pixel leaks, whatever its neighbours' parts hold


def test_part_k_is_the_same_image_for_every_K():
    """What lets the GPU tests share one reference per part."""
    big, a9, n9 = dnp.synthetic_parts(37, 29, FB, 9, seed=5)
    for K in (1, 2, 5):
        small, a, n = dnp.synthetic_parts(37, 29, FB, K, seed=5)
        assert np.array_equal(_bits(small), _bits(big[:K])) and np.array_equal(_bits(a), _bits(a9))
        assert np.array_equal(_bits(n), _bits(n9))


def test_parts_sum():
    rng = np.random.default_rng(3)
    ims = rng.normal(size=(4, 6, 7, 5)).astype(f32)
    ims[:, 0, 0, :3] = f32(-0.0)       # -0 + -0 = -0: no +0 is added first
    ims[1, 1, 1, 0] = np.inf
    ims[2, 1, 1, 0] = -np.inf          # inf + -inf = NaN, as float32 has it
    got = dnp.parts_sum(ims)
    with np.errstate(invalid="ignore"):
        want = ((ims[0][..., :3] + ims[1][..., :3]) + ims[2][..., :3]) + ims[3][..., :3]
    assert np.array_equal(_bits(got[..., :3]), _bits(want))
    assert np.array_equal(_bits(got[..., 3:]), _bits(ims[0][..., 3:]))
    assert np.signbit(got[0, 0, :3]).all() and np.isnan(got[1, 1, 0])
    one = dnp.parts_sum(ims[:1])
    assert np.array_equal(_bits(one), _bits(ims[0]))
