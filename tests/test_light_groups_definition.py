"""The definition of a light group's image (include/nart_hip.h, "Light groups") rests on one yardstick:
the unchanged oracle on the scene file with every other light's intensity set to 0.  This checks, with
the oracle alone, the conditions that comparison needs on every frame the GPU tests use it on: the
zero-intensity images are free of NaN and inf (no 0 * inf was formed), their alpha and filter weight sum
have the beauty's bits (no draw, pdf, hit or alpha depends on a light's emission), every light's image
is non-zero somewhere, and the images sum to the beauty within the bound for two orders of summing the
same non-negative terms (a sanity bound, not the parity bar)."""
import numpy as np
import pytest

import lightgroup_py as lg

FRAMES = sorted(lg.DEFINITION_FRAMES)


@pytest.fixture(scope="module")
def frames(built, tmp_path_factory):
    return lg.shared_frames(tmp_path_factory)


@pytest.mark.parametrize("name", FRAMES)
def test_zero_intensity_frames(frames, name):
    w, h, spp = lg.DEFINITION_FRAMES[name]
    p = frames.params(name, w, h, spp)
    n = lg.n_lights(frames.base[name])
    assert n >= 2
    beauty = frames.oracle(name, p)
    groups = [frames.oracle(name, p, lit=[l]) for l in range(n)]
    assert np.isfinite(beauty).all()
    total = np.zeros(beauty.shape[:2] + (3,), np.float64)
    for l, img in enumerate(groups):
        assert np.isfinite(img).all(), l                                  # no 0 * inf: the comparison's condition
        assert lg.bits_equal(img[..., 3:], beauty[..., 3:]), l            # alpha and filter weight sum
        assert (img[..., :3] > 0).any(), l                                # non-trivial
        assert (img[..., :3] >= 0).all(), l
        total += img[..., :3]
    bound = lg.sum_bound(spp, p.filter_width, p.bounces, n)
    err = np.abs(total - beauty[..., :3].astype(np.float64))
    rel = float((err / np.maximum(total, 1e-300)).max())
    print("%s: %d lights, sum of the groups against the beauty: %.3g relative, bound %.3g" % (name, n, rel, bound))
    assert (err <= bound * total).all(), (name, rel, bound)


def test_nested_frame_reaches_the_deep_lists(frames):
    """bounces 16 > ILIST_REG: the frame runs the EXT build on the device."""
    p = frames.params("nested", *lg.DEFINITION_FRAMES["nested"])
    assert p.bounces == 16


def test_merged_lights(frames):
    """Two lights in one group: lights 1 and 2 of veach lit together."""
    p = frames.params("veach", *lg.DEFINITION_FRAMES["veach"])
    both, one, two, beauty = (frames.oracle("veach", p, lit=l) for l in ([1, 2], [1], [2], None))
    assert np.isfinite(both).all() and lg.bits_equal(both[..., 3:], beauty[..., 3:])
    total = one[..., :3].astype(np.float64) + two[..., :3]
    assert (np.abs(total - both[..., :3]) <= lg.sum_bound(p.spp, p.filter_width, p.bounces, 2) * total).all()
