"""The definition of a depth-cut image (include/nart_hip.h, "Depth cuts") rests on one yardstick: the
unchanged oracle at `bounces = d`, which agrees with the cut where the RNG start states agree -- the whole
frame at 1 spp.  This checks, with the oracle alone, what that comparison needs on every frame the GPU
tests use it on (depthcut_py.FRAMES_1SPP): the `bounces = d` frames are finite, their alpha and filter
weight sum have the beauty's bits (alpha is settled at bounce 0, the splat weights do not depend on the
paths), and the first two cuts differ from their neighbours somewhere, so a kernel that wrote the wrong
cut's L could not pass.  The layers of those frames sum back to the beauty within the bound of
depthcut_py.layers."""
import numpy as np
import pytest

import depthcut_py as dc

KEYS = sorted(dc.FRAMES_1SPP)


@pytest.fixture(scope="module")
def frames(built, tmp_path_factory):
    return dc.lg.shared_frames(tmp_path_factory)


@pytest.mark.parametrize("key", KEYS)
def test_bounce_limited_frames(frames, key):
    name, p, cuts = dc.frame_params(frames, key)
    assert p.spp == 1 and cuts == sorted(set(cuts)) and 1 <= cuts[0] and cuts[-1] <= p.bounces
    beauty = frames.oracle(name, p)
    images = [frames.oracle(name, dc.with_bounces(p, d)) for d in cuts]
    assert np.isfinite(beauty).all()
    for d, img in zip(cuts, images):
        assert np.isfinite(img).all(), d
        assert dc.bits_equal(img[..., 3:], beauty[..., 3:]), d  # alpha and filter weight sum
        if d == p.bounces:
            assert dc.bits_equal(img, beauty)
    # The first two cuts differ from a neighbouring cut somewhere: the first from the second, the second
    # from the first or the third.  (Not always from the third: in the nested-glass frame the bounces 4
    # and 5 of every path add nothing -- the oracle's frames at bounces = 3, 4 and 5 are the same bits --
    # so cut 3 equals cut 5 there; it differs from cut 1 and from cut 16.)  At least three of a frame's
    # cut images are distinct, so a kernel that wrote a cut's L into another cut's record cannot pass.
    nxt = images[1:] + [beauty]
    differ = [int((dc.bits(images[j]) != dc.bits(nxt[j])).sum()) for j in range(len(cuts))]
    for j in range(len(cuts)):
        print("%s: cut %d against %s: %d floats differ" % (key, cuts[j], cuts[j + 1] if j + 1 < len(cuts) else "the beauty", differ[j]))
    assert differ[0] > 0, (key, cuts[0], cuts[1])
    assert differ[0] > 0 or differ[1] > 0, (key, cuts[1])
    assert len({img.tobytes() for img in images}) >= 3, key
    assert (images[0][..., :3] > 0).any()
    # the layers of these frames: layer_0 is the first cut, and summed ascending they meet the beauty
    L = dc.layers(np.stack(images), beauty)
    assert dc.bits_equal(L[0][..., :3], images[0][..., :3]) and dc.bits_equal(L[..., 3:], np.broadcast_to(beauty[..., 3:], L[..., 3:].shape))
    err = np.abs(dc.layers_sum(L).astype(np.float64) - beauty[..., :3])
    assert (err <= dc.layers_bound(np.stack(images), beauty)).all(), float(err.max())


def test_nested_frame_reaches_the_deep_lists(frames):
    """bounces 16 > ILIST_REG: the frame runs the EXT build on the device."""
    _name, p, cuts = dc.frame_params(frames, "nested")
    assert p.bounces == 16 and cuts[-1] == 16
