"""Adaptive sampling without a GPU: the level list of the C ABI (nart_hip_adaptive_levels, host only)
against its Python restatement, the parameter defaults, and the numpy restatement of the per-bucket
error (tests/adaptive_py.py, the yardstick of tests/test_gpu_adaptive.py) on synthetic tiles whose
values are worked out by hand here."""
import ctypes

import numpy as np
import pytest

import adaptive_py as ad
import nart_amd
import oracle
from test_aov_restatement import total_frame_uv

f32 = np.float32


@pytest.fixture(scope="module")
def hip(built):
    from nart_amd import build as nb
    nb.build_hip_lib()
    return nart_amd.hip_lib()


# ---------------------------------------------------------------- levels and defaults
def test_parameter_defaults(hip):
    ap = nart_amd.AdaptiveParams.defaults()
    assert (ap.min_spp, ap.growth) == (16, 4)
    assert f32(ap.threshold) == f32(0.1) and f32(ap.floor) == f32(0.01)
    assert nart_amd.AdaptiveParams.defaults(min_spp=4, threshold=0.5).min_spp == 4
    assert nart_amd.adaptive_levels(None, 256) == [16, 64, 256]


def test_levels_match_restatement(hip):
    for min_spp in (2, 3, 5, 16, 64, 300):
        for growth in (2, 3, 4, 16):
            for spp in (2, 3, 7, 8, 16, 17, 64, 255, 256, 257, 1000, 2 ** 32 - 1):
                ap = nart_amd.AdaptiveParams.defaults(min_spp=min_spp, growth=growth)
                got = nart_amd.adaptive_levels(ap, spp)
                assert got == ad.levels(min_spp, growth, spp), (min_spp, growth, spp)
                assert got[-1] == spp and len(got) <= 32 and all(a < b for a, b in zip(got, got[1:]))
    assert nart_amd.adaptive_levels(nart_amd.AdaptiveParams.defaults(min_spp=8), 8) == [8]          # min == max
    assert nart_amd.adaptive_levels(nart_amd.AdaptiveParams.defaults(min_spp=64), 8) == [8]         # min > max
    assert nart_amd.adaptive_levels(nart_amd.AdaptiveParams.defaults(min_spp=16), 100) == [16, 64, 100]  # no power
    assert nart_amd.adaptive_levels(nart_amd.AdaptiveParams.defaults(min_spp=2, growth=2), 8) == [2, 4, 8]
    assert nart_amd.adaptive_levels(nart_amd.AdaptiveParams.defaults(min_spp=2, growth=16), 1000) == [2, 32, 512, 1000]
    # the cap: 2, 4, ... 2^31 are 31 levels, the 32nd is the maximum
    cap = nart_amd.adaptive_levels(nart_amd.AdaptiveParams.defaults(min_spp=2, growth=2), 2 ** 32 - 1)
    assert len(cap) == 32 and cap[:31] == [2 ** i for i in range(1, 32)] and cap[31] == 2 ** 32 - 1


def test_levels_query_and_invalid(hip):
    n = ctypes.c_uint32()
    ap = nart_amd.AdaptiveParams.defaults(min_spp=2, growth=2)
    assert hip.nart_hip_adaptive_levels(ctypes.byref(ap), 8, None, ctypes.byref(n)) == 0 and n.value == 3
    assert hip.nart_hip_adaptive_levels(None, 256, None, ctypes.byref(n)) == 0 and n.value == 3
    assert hip.nart_hip_adaptive_levels(ctypes.byref(ap), 8, None, None) == -1
    bad = [dict(min_spp=1), dict(min_spp=0), dict(growth=1), dict(growth=17), dict(threshold=-1.0),
           dict(threshold=float("nan")), dict(floor=0.0), dict(floor=-1.0), dict(floor=float("inf")),
           dict(floor=float("nan"))]
    for kw in bad:
        with pytest.raises(nart_amd.NartError) as e:
            nart_amd.adaptive_levels(nart_amd.AdaptiveParams.defaults(**kw), 8)
        assert e.value.code == -1, kw
    with pytest.raises(nart_amd.NartError):
        nart_amd.adaptive_levels(None, 1)  # one sample has no variance
    assert nart_amd.adaptive_levels(nart_amd.AdaptiveParams.defaults(threshold=float("inf")), 64) == [16, 64]


# ---------------------------------------------------------------- the error on synthetic tiles
B, FB, TILE = 4, 1, 6
FLOOR = 0.01


def _tiles(fill=0.0):
    return np.full((TILE, TILE, 5), fill, f32), np.full((TILE, TILE, 5), fill, f32)


def _noisy_pixel(T, M, dx, dy):
    """c = 1 per channel, m2 = 2, so var = 1; k = 1/4, so V = 1/4 and sqrt(V) = 1/2."""
    T[FB + dy, FB + dx] = [1, 1, 1, 1, 1]
    M[FB + dy, FB + dx] = [2, 2, 2, 0.25, 1]


SD1 = f32(f32(f32(0.2126) * f32(0.5) + f32(0.7152) * f32(0.5)) + f32(0.0722) * f32(0.5))
L1 = f32(f32(f32(0.2126) + f32(0.7152)) + f32(0.0722))


def test_error_constant_tile_is_zero():
    T, M = _tiles()
    T[...] = [1.0, 0.5, 0.25, 2, 2]        # c = (0.5, 0.25, 0.125), w = 2
    M[...] = [0.5, 0.125, 0.03125, 1, 2]   # m2 = c^2 exactly: no variance
    E = ad.bucket_error(T, M, B, B, FB, FLOOR)
    assert E == 0 and not np.signbit(E)
    black = _tiles()
    assert ad.bucket_error(*black, B, B, FB, FLOOR) == 0   # every T.w == 0


def test_error_single_lit_pixel_by_hand():
    """One noisy pixel, every other own pixel with T.w == 0 (sd = l = 0; adding 0 changes no sum)."""
    T, M = _tiles()
    _noisy_pixel(T, M, 2, 1)
    want = f32(SD1 / f32(L1 + f32(f32(FLOOR) * f32(16))))
    got = ad.bucket_error(T, M, B, B, FB, FLOOR)
    assert got.dtype == f32 and got.view(np.uint32) == want.view(np.uint32)
    # a pixel with T.w == 0 contributes nothing, whatever else it holds
    T[FB, FB] = [5, 5, 5, 1, 0]
    M[FB, FB] = [9, 9, 9, 1, 0]
    assert ad.bucket_error(T, M, B, B, FB, FLOOR).view(np.uint32) == want.view(np.uint32)
    # the tile's border (other buckets' pixels) is not the bucket's own
    T[0, :] = 1e30
    M[:, TILE - 1] = np.nan
    assert ad.bucket_error(T, M, B, B, FB, FLOOR).view(np.uint32) == want.view(np.uint32)


def test_error_all_pixels_by_hand_in_order():
    """Sixteen equal noisy pixels: row sums of four terms from 0, then four rows from 0."""
    T, M = _tiles()
    for dy in range(B):
        for dx in range(B):
            _noisy_pixel(T, M, dx, dy)
    rs, rl = f32(0), f32(0)
    for _ in range(B):
        rs, rl = f32(rs + SD1), f32(rl + L1)
    S, Ls = f32(0), f32(0)
    for _ in range(B):
        S, Ls = f32(S + rs), f32(Ls + rl)
    want = f32(S / f32(Ls + f32(f32(FLOOR) * f32(16))))
    assert ad.bucket_error(T, M, B, B, FB, FLOOR).view(np.uint32) == want.view(np.uint32)


def test_error_clamps_and_nan():
    T, M = _tiles()
    _noisy_pixel(T, M, 0, 0)
    M[FB, FB, :3] = 0.5                     # m2 < c^2: var clamps to 0
    assert ad.bucket_error(T, M, B, B, FB, FLOOR) == 0
    _noisy_pixel(T, M, 1, 1)
    T[FB + 1, FB + 1, 1] = np.nan           # a NaN radiance: E is NaN (and the bucket refines)
    assert np.isnan(ad.bucket_error(T, M, B, B, FB, FLOOR))
    T[FB + 1, FB + 1, 1] = -3.0             # negative luminance counts as 0 in the denominator
    T[FB + 1, FB + 1, 0] = -3.0
    T[FB + 1, FB + 1, 2] = -3.0
    M[FB + 1, FB + 1, :3] = 9.0             # m2 = c^2 = 9
    E = ad.bucket_error(T, M, B, B, FB, FLOOR)
    assert E == 0  # pixel (0,0) clamps to 0, pixel (1,1) has no variance; l = L1 + 0


def test_error_ragged_bucket():
    """nx = 3 < B, ny = 2: columns and rows past them belong to pixels the bucket does not trace."""
    T, M = _tiles()
    _noisy_pixel(T, M, 2, 1)
    T[FB:, FB + 3:] = 1e30
    M[FB:, FB + 3:] = 1e30
    T[FB + 2:, :] = np.nan
    want = f32(SD1 / f32(L1 + f32(f32(FLOOR) * f32(6))))
    assert ad.bucket_error(T, M, 3, 2, FB, FLOOR).view(np.uint32) == want.view(np.uint32)


# ---------------------------------------------------------------- tiles and the selection loop
def _params(scene, w, h, spp, **kw):
    p = nart_amd.load_sessions(scene.path)[0]
    p.image_width, p.image_height, p.spp = w, h, spp
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_restated_tiles_and_selection_against_oracle(glass_scene):
    """glassSphere 24 x 20, bucket 16 (ragged buckets, extra rows): the restated beauty tiles over
    the oracle's per-sample Li_alpha are the oracle's tiles bit for bit, the own pixels of a bucket
    are exactly the tile pixels that hold its samples' centres, and the selection loop over the
    oracle's samples stops the buckets a threshold between two level-0 errors says it stops."""
    p = _params(glass_scene, 24, 20, 4, bucket_size=16)
    g = nart_amd.session_geometry(p)
    orc = oracle.Oracle(glass_scene)
    nb = g.n_buckets_x * g.n_buckets_y

    def samples_of(spp):
        q = p.copy()
        q.spp = spp
        return orc.render_samples(q, 0, 0, g.total_width, g.total_height)

    p2 = p.copy()
    p2.spp = 2
    beauty, moment = ad.restate_tiles(p2, total_frame_uv(p2), samples_of(2), list(range(nb)))
    want = orc.render_buckets(p2, np.arange(nb)).reshape(beauty.shape)
    assert np.array_equal(beauty.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(moment[..., 4].view(np.uint32), beauty[..., 4].view(np.uint32))
    fb = g.filter_bounds
    for b in range(nb):
        nx, ny = ad.own_size(p, g, b)
        assert 0 < nx <= p.bucket_size and 0 < ny <= p.bucket_size
        # the Gaussian's centre weight is the largest: every own pixel has weight, and the heaviest
        # pixels of the tile are own pixels
        w = beauty[b, :, :, 4]
        assert (w[fb:fb + ny, fb:fb + nx] > 0).all()
        iy, ix = np.unravel_index(np.argmax(w), w.shape)
        assert fb <= iy < fb + ny and fb <= ix < fb + nx

    first = []
    mid = lambda E: float((np.sort(np.unique(E))[0].astype(np.float64) + np.sort(np.unique(E))[1]) / 2)
    spp, err, lists, thr = ad.select(p, 2, 2, mid, 0.01, samples_of, first_errors=first)
    assert len(first) == nb and len(set(first)) >= 2
    assert lists[0] == list(range(nb)) and 0 < len(lists[1]) < nb
    stopped = [b for b in range(nb) if first[b] <= thr]
    assert sorted(stopped + lists[1]) == list(range(nb))
    assert all(spp[b] == 2 and err[b] == f32(first[b]) for b in stopped)
    assert all(spp[b] == 4 for b in lists[1]) and len(lists) == 2
    inf = ad.select(p, 2, 2, float("inf"), 0.01, samples_of)
    assert (inf[0] == 2).all() and len(inf[2]) == 1
