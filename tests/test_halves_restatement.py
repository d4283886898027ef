"""The restatement behind the half buffers (tests/halves_py.py), validated without a GPU over the
oracle's per-sample Li_alpha: half h against the splat of its own samples alone, the beauty at one
sample per pixel, the weight sums, and a planted NaN."""
import numpy as np
import pytest

import halves_py as hp
import nart_amd
import oracle
from test_aov_restatement import restate_render

f32 = np.float32
EPS = float(np.finfo(np.float32).eps)
SIZE = (16, 12)
CONFIG = dict(bucket_size=12)  # the total frame is 20 x 16: the bucket size divides neither


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


_cache = {}


def _samples(scene, spp):
    """(p, uv, L, beauty, halves) of glassSphere at `spp`, computed once and shared read-only."""
    if spp not in _cache:
        p = _params(scene, SIZE[0], SIZE[1], spp, **CONFIG)
        g = nart_amd.session_geometry(p)
        assert g.total_width % p.bucket_size and g.total_height % p.bucket_size
        orc = oracle.Oracle(scene)
        L, uv = orc.render_samples(p, 0, 0, g.total_width, g.total_height, with_uv=True)
        assert np.isfinite(L).all()
        beauty = restate_render(p, uv, L)
        assert _bits_equal(beauty, orc.render(p))
        _cache[spp] = (p, uv, L, beauty, hp.restate_halves(p, uv, L))
        for a in _cache[spp][2:]:
            a.setflags(write=False)
    return _cache[spp]


def test_split_records():
    L = np.arange(2 * 5 * 4, dtype=f32).reshape(2, 5, 4) + f32(0.5)
    L[0, 1, 0], L[1, 2, 1] = np.nan, np.inf
    for h in (0, 1):
        rec = hp.split(L, h)
        mine = np.arange(5) % 2 == h
        assert _bits_equal(rec[:, mine, :3], L[:, mine, :3]) and (rec[:, mine, 3] == 1).all()
        assert not _bits(rec[:, ~mine]).any()  # exactly +0
    # a non-finite colour reaches one record stream only
    assert np.isnan(hp.split(L, 1)[0, 1, 0]) and np.isfinite(hp.split(L, 0)[0]).all()
    assert np.isinf(hp.split(L, 0)[1, 2, 1]) and np.isfinite(hp.split(L, 1)[1]).all()


@pytest.mark.parametrize("spp", [1, 2, 5, 8])
def test_half_is_the_splat_of_its_own_samples(glass_scene, spp):
    """Adding the zero records changes nothing: the contribution has the bits of the splat of the
    samples of parity h alone (whose weight sum is the half's own, contribution[3]), and
    filter_weight_sum has the beauty's bits."""
    p, uv, L, beauty, halves = _samples(glass_scene, spp)
    for h in (0, 1):
        alone = hp.restate_half_alone(p, uv, L, h)
        assert _bits_equal(halves[h][..., :4], alone[..., :4]), h
        assert _bits_equal(alone[..., 4], alone[..., 3]), h
        assert _bits_equal(halves[h][..., 4], beauty[..., 4]), h
    assert halves[0][..., :3].max() > 0
    assert (halves[1][..., :3].max() > 0) == (spp > 1)


def test_one_sample_per_pixel(glass_scene):
    """At spp 1 half 0's rgb is the beauty's, its own weight sum is the weight sum, and half 1 is zero
    but for the weight sum."""
    p, uv, L, beauty, halves = _samples(glass_scene, 1)
    assert _bits_equal(halves[0][..., :3], beauty[..., :3])
    assert _bits_equal(halves[0][..., 3], beauty[..., 4])
    assert not _bits(halves[1][..., :4]).any()
    assert _bits_equal(halves[1][..., 4], beauty[..., 4])


@pytest.mark.parametrize("spp", [2, 5, 8])
def test_weight_sums_and_colours_add_up(glass_scene, spp):
    """H_0[3] + H_1[3] against the weight sum, and H_0.rgb + H_1.rgb against the beauty: the same
    non-negative (weights) or finite (colours) float32 terms summed in two groupings.  A pixel receives
    at most n = spp * (2 fb + 1)^2 sample terms and 4 tile sums; each side's summation error is below
    (n + 4) * eps * sum |term|, and the magnitudes' sum is bounded by the float64 sum of the terms,
    which the restatement over |L| gives."""
    p, uv, L, beauty, halves = _samples(glass_scene, spp)
    g = nart_amd.session_geometry(p)
    n = spp * (2 * g.filter_bounds + 1) ** 2 + 4
    total_w = halves[0][..., 3].astype(np.float64) + halves[1][..., 3].astype(np.float64)
    W = beauty[..., 4].astype(np.float64)
    with np.errstate(all="ignore"):
        print("spp %d: H_0[3] + H_1[3] off the weight sum by at most %.2f ulp" % (spp, np.nanmax(np.abs(total_w - W) / (EPS * W))))
    assert (np.abs(total_w - W) <= 2 * n * EPS * W).all()
    mag = restate_render(p, uv, np.abs(L)).astype(np.float64)[..., :3]
    total = halves[0][..., :3].astype(np.float64) + halves[1][..., :3].astype(np.float64)
    assert (np.abs(total - beauty[..., :3]) <= 2 * n * EPS * mag * (1 + n * EPS)).all()
    # finalize of the halves adds up to the beauty's
    fin = nart_amd.finalize(p, halves[0])[..., :3].astype(np.float64) + nart_amd.finalize(p, halves[1])[..., :3]
    ref = nart_amd.finalize(p, beauty)[..., :3].astype(np.float64)
    assert np.allclose(fin, ref, rtol=0, atol=float(4 * n * EPS * (np.abs(ref).max() + 1)))
    # the means are normalised by the halves' own weights
    m = hp.half_mean(halves[0])
    assert _bits_equal(m, nart_amd.half_mean(halves[0]))
    ok = halves[0][..., 3] > 0
    assert ok.any() and _bits_equal(m[ok], (halves[0][..., :3][ok] / halves[0][..., 3][ok][:, None]).astype(f32))


@pytest.mark.parametrize("s_bad", [0, 1, 4])
def test_planted_nan_reaches_one_half(glass_scene, s_bad):
    p, uv, L, beauty, halves = _samples(glass_scene, 5)
    g = nart_amd.session_geometry(p)
    bad = L.copy()
    y, x = g.total_height // 2, g.total_width // 2
    bad[y, x, s_bad, 1] = np.nan
    h_bad = s_bad % 2
    got = hp.restate_halves(p, uv, bad)
    assert np.isnan(got[h_bad][..., :3]).any()
    assert np.isfinite(got[1 - h_bad]).all()
    assert _bits_equal(got[1 - h_bad], halves[1 - h_bad])
    # and only within the sample's footprint (pixel (x, y)'s samples lie at (x + fb + u, y + fb + v): add_sample)
    ys, xs = np.nonzero(np.isnan(got[h_bad]).any(axis=-1))
    fb = g.filter_bounds
    assert (np.abs(ys - (y + fb)) <= fb + 1).all() and (np.abs(xs - (x + fb)) <= fb + 1).all()
    assert np.isfinite(got[h_bad][..., 3:]).all()
