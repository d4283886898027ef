"""The restatement behind the first-hit ID mattes (tests/matte_py.py), validated without a GPU: the
ranking and the extraction on hand-made pixels; the planes over the oracle's first hits on the
materials scene (which fixes the frame size the GPU test reuses); and the new entry points' id counts,
defaults and argument checks."""
import ctypes

import numpy as np
import pytest

import aov_py
import matte_py as mp
import nart_amd
import oracle
from nart_amd import scenes

f32 = np.float32
# The materials scene's frame of the matte tests, chosen here on the CPU: at this size and 2 spp a
# cropped pixel sees three ids (so ranks = 2 truncates) and the second plane (ids 4..6) is reached;
# test_first_hits_on_materials_scene asserts both.
MATERIALS_SIZE = (40, 24)
MATERIALS_SPP = 2


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


def _pixels(rows, n, fb=1):
    """Plane images of a one-row frame: rows is a list of (W, [c_0 .. c_{n-1}]) per pixel, given as
    contributions (not yet divided by W)."""
    W = len(rows)
    planes = np.zeros((mp.n_planes(n), 1 + 2 * fb, W + 2 * fb, 5), f32)
    planes[...] = 0.375  # the border is not read
    for x, (wt, cs) in enumerate(rows):
        assert len(cs) == n
        planes[:, fb, x + fb] = 0
        planes[:, fb, x + fb, 4] = wt
        for m, c in enumerate(cs):
            planes[m // 4, fb, x + fb, m % 4] = c
    return planes


def _pairs(ranks, x, fb=1):
    """[(id, c)] of pixel x of a one-row frame."""
    R = 2 * ranks.shape[0]
    return [(float(ranks[r // 2, fb, x + fb, 2 * (r % 2)]), float(ranks[r // 2, fb, x + fb, 2 * (r % 2) + 1]))
            for r in range(R)]


# ---------------------------------------------------------------- 1. ranking and extraction
def test_rank_hand_made_pixels():
    nan, inf = float("nan"), float("inf")
    # n = 5, weights of 2: c = contribution / 2
    rows = [(2.0, [0.5, 1.0, 0.5, 0.0, 1.0]),      # ties: 1 before 4, 0 before 2; id 3 is zero
            (2.0, [0.0, -1.0, nan, 0.25, 0.0]),     # zero, negative and NaN never rank
            (0.0, [1.0, 1.0, 1.0, 1.0, 1.0]),       # W = 0
            (-2.0, [1.0, 1.0, 1.0, 1.0, 1.0]),      # W < 0
            (nan, [1.0, 1.0, 1.0, 1.0, 1.0]),       # W = NaN
            (2.0, [0.0, 0.0, 0.0, 0.0, 2.0]),       # one id, in the second plane
            (2.0, [0.25, inf, 0.5, 0.0, 0.0])]      # an infinite coverage ranks first
    planes = _pixels(rows, 5)
    W = len(rows)
    r2 = mp.rank(W, 1, 1, planes, 5, 2)
    r8 = mp.rank(W, 1, 1, planes, 5, 8)
    assert r2.shape == (1, 3, W + 2, 5) and r8.shape == (4, 3, W + 2, 5)
    E = (-1.0, 0.0)
    assert _pairs(r8, 0) == [(1, 0.5), (4, 0.5), (0, 0.25), (2, 0.25), E, E, E, E]
    assert _pairs(r2, 0) == [(1, 0.5), (4, 0.5)]     # N > R truncates
    assert _pairs(r8, 1) == [(3, 0.125)] + [E] * 7
    for x in (2, 3, 4):
        assert _pairs(r8, x) == [E] * 8 and _pairs(r2, x) == [E] * 2
    assert _pairs(r8, 5) == [(4, 1.0)] + [E] * 7
    assert _pairs(r8, 6) == [(1, inf), (2, 0.25), (0, 0.125)] + [E] * 5
    # the weight is 1 in every cropped pixel, W <= 0 included; the border is all zero
    for r in (r2, r8):
        assert (r[:, 1, 1:W + 1, 4] == 1).all()
        assert not _bits(r[:, 0]).any() and not _bits(r[:, 2]).any()
        assert not _bits(r[:, :, 0]).any() and not _bits(r[:, :, -1]).any()
    # the first R ranks do not depend on R
    assert _bits_equal(r2[0], r8[0])


@pytest.mark.parametrize("n", [1, 4, 5, 32])
def test_rank_id_counts(n):
    """n ids with distinct coverages (m + 1) / 64 in one pixel, all equal ones in another: the ranks are
    the ids by falling coverage, then by rising id; channels beyond n are never ids."""
    fb = 2
    rows = [(4.0, [(m + 1) / 16.0 for m in range(n)]), (4.0, [1.0] * n)]
    planes = _pixels(rows, n, fb)
    for q in range(mp.n_planes(n)):  # what the padding channels of the last plane hold is not an id
        for c in range(4):
            if 4 * q + c >= n:
                planes[q, fb, fb:fb + 2, c] = 100.0
    for R in (2, 8):
        rk = mp.rank(2, 1, fb, planes, n, R)
        want0 = [(float(m), (m + 1) / 64.0) for m in range(n - 1, -1, -1)][:R]
        want1 = [(float(m), 0.25) for m in range(n)][:R]
        pad = [(-1.0, 0.0)] * R
        assert _pairs(rk, 0, fb) == (want0 + pad)[:R]
        assert _pairs(rk, 1, fb) == (want1 + pad)[:R]
    # no ids at all: empty ranks
    rk = mp.rank(2, 1, fb, np.zeros((0, 5, 6, 5), f32), 0, 2)
    assert _pairs(rk, 0, fb) == [(-1.0, 0.0)] * 2 and rk[0, fb, fb, 4] == 1


def test_extract_hand_sums():
    rows = [(2.0, [0.5, 1.0, 0.5, 0.0, 1.0]), (2.0, [0.0, 0.0, 0.0, 0.25, 0.0]), (0.0, [1.0] * 5),
            (3.0, [0.1, 0.7, 0.3, 0.9, 0.2])]
    planes = _pixels(rows, 5)
    W = len(rows)
    for R in (2, 8):
        rk = mp.rank(W, 1, 1, planes, 5, R)
        empty = mp.extract(W, 1, 1, rk, 0)
        assert not _bits(empty[..., :4]).any() and (empty[1, 1:W + 1, 4] == 1).all()
        assert not _bits(empty[0]).any() and not _bits(empty[2]).any() and not _bits(empty[:, 0]).any()
        full = mp.extract(W, 1, 1, rk, (1 << 64) - 1)
        for x in range(W):
            s = f32(0)
            for i, c in _pairs(rk, x):
                if i >= 0:
                    s = f32(s + f32(c))
            assert (_bits(full[1, x + 1, :4]) == _bits(s)).all() and full[1, x + 1, 4] == 1
        assert full[1, 3, 0] == 0  # W = 0: nothing ranked
    r8 = mp.rank(W, 1, 1, planes, 5, 8)
    # pixel 0 by hand: ids {0, 4} cover 0.25 + 0.5, summed in rank order (4 before 0)
    got = mp.extract(W, 1, 1, r8, (1 << 0) | (1 << 4))
    assert got[1, 1, 0] == f32(f32(0.5) + f32(0.25)) and got[1, 2, 0] == 0
    # pixel 3: all five ids in rank order 3, 1, 2, 4, 0
    c = [f32(f32(v) / f32(3.0)) for v in (0.9, 0.7, 0.3, 0.2, 0.1)]
    s = f32(0)
    for v in c:
        s = f32(s + v)
    assert mp.extract(W, 1, 1, r8, 0b11111)[1, 4, 0] == s
    # with R = 2 only the two greatest are left to extract
    r2 = mp.rank(W, 1, 1, planes, 5, 2)
    assert mp.extract(W, 1, 1, r2, 0b11111)[1, 4, 0] == f32(c[0] + c[1])


def test_records():
    ids = np.array([-1, 0, 3, 4, 6, 7, 31, 32, 40], np.int64)
    r0, r1, r7 = mp.records(ids, 0, 7), mp.records(ids, 1, 7), mp.records(ids, 7, 32)
    assert r0.dtype == f32 and r0.shape == (9, 4)
    assert r0.tolist() == [[0] * 4, [1, 0, 0, 0], [0, 0, 0, 1]] + [[0] * 4] * 6
    assert r1.tolist() == [[0] * 4] * 3 + [[1, 0, 0, 0], [0, 0, 1, 0]] + [[0] * 4] * 4   # id 7 >= n = 7: no id
    assert r7.tolist() == [[0] * 4] * 6 + [[0, 0, 0, 1]] + [[0] * 4] * 2
    assert not np.signbit(r0).any()


# ---------------------------------------------------------------- 2. first hits from the oracle
def materials_first_hits(scene, p):
    """(uv, tri) of every sample of the total frame from the oracle: (totalH, totalW, spp, 2) float32
    and (totalH, totalW, spp) int64 (negative: a miss)."""
    g = nart_amd.session_geometry(p)
    orc = oracle.Oracle(scene)
    r = aov_py.trace_block(orc, p, 0, 0, g.total_width, g.total_height)
    return r["uv"], r["tri"]


def test_first_hits_on_materials_scene(materials_scene):
    p = _params(materials_scene, MATERIALS_SIZE[0], MATERIALS_SIZE[1], MATERIALS_SPP)
    g = nart_amd.session_geometry(p)
    fb, W, H = g.filter_bounds, p.image_width, p.image_height
    uv, tri = materials_first_hits(materials_scene, p)
    counts = materials_scene.counts()
    assert counts["meshes"] == 7 and counts["materials"] == 7
    for kind, n in ((0, counts["meshes"]), (1, counts["materials"])):
        ids = mp.ids_of(materials_scene, tri, kind)
        assert ids.max() < n and (ids >= 0).any() and (ids < 0).any() == bool((tri < 0).any())
        planes, terms = mp.restate_planes(p, uv, ids, n, with_terms=True)
        assert planes.shape == (2, g.total_height, g.total_width, 5)
        assert _bits_equal(planes[1][..., 4], planes[0][..., 4])
        crop = planes[:, fb:fb + H, fb:fb + W]
        positive = sum((crop[q][..., c] > 0).astype(int) for q in range(2) for c in range(4))
        print("kind", kind, "ids seen", sorted(set(ids[ids >= 0].tolist())), "pixels by ids covering them",
              np.bincount(positive.ravel()).tolist())
        assert positive.max() >= 3            # ranks = 2 truncates somewhere
        assert crop[1][..., :3].max() > 0     # ids 4..6 reach the second plane
        assert not crop[1][..., 3].any()      # the padding channel (id 7) stays empty
        r2 = mp.rank(W, H, fb, planes, n, 2)
        r6 = mp.rank(W, H, fb, planes, n, 6)
        assert _bits_equal(r2[0], r6[0])
        full = (positive >= 3)
        assert (r6[1][fb:fb + H, fb:fb + W, 0][full] >= 0).all()
        # every hit sample is in exactly one id's plane: the coverages sum to the hit coverage
        hit = np.zeros(ids.shape + (4,), f32)
        hit[..., 3] = ids >= 0
        cov = mp.restate_render(p, uv, hit)[fb:fb + H, fb:fb + W]
        with np.errstate(all="ignore"):
            total = (crop[..., :4].astype(np.float64) / crop[0][..., 4:5]).sum(axis=(0, -1))
            want = cov[..., 3].astype(np.float64) / cov[..., 4]
        tol = (terms[fb:fb + H, fb:fb + W] + n) * 2.0 ** -24
        ok = cov[..., 4] > 0
        assert ok.all() and (np.abs(total - want)[ok] <= tol[ok] * want[ok]).all()


# ---------------------------------------------------------------- 3. entry points without a GPU
def test_matte_ids_of_scenes(glass_scene, materials_scene, tmp_path):
    from nart_amd import build as nb
    nb.build_hip_lib()
    for scene in (glass_scene, materials_scene):
        c = scene.counts()
        assert nart_amd.matte_ids(scene, nart_amd.api.MATTE_MESH) == c["meshes"]
        assert nart_amd.matte_ids(scene, nart_amd.api.MATTE_MATERIAL) == c["materials"]
        assert nart_amd.matte_ids(scene) == c["meshes"]
    big = nart_amd.Scene(scenes.nested_glass(str(tmp_path), n=33))
    assert big.counts()["meshes"] == 34
    lib = nart_amd.hip_lib()
    n = ctypes.c_uint32()
    assert lib.nart_hip_matte_ids(big.blob, 0, ctypes.byref(n)) == -6 and n.value == 34
    with pytest.raises(nart_amd.NartError) as e:
        nart_amd.matte_ids(big)
    assert e.value.code == -6
    with pytest.raises(nart_amd.NartError):
        nart_amd.matte_ids(glass_scene, 2)
    assert lib.nart_hip_matte_ids(None, 0, ctypes.byref(n)) == -1
    assert lib.nart_hip_matte_ids(glass_scene.blob, 0, None) == -1
    assert lib.nart_hip_matte_ids(glass_scene.blob, 2, ctypes.byref(n)) == -1


BAD = [dict(kind=2), dict(kind=0xFFFFFFFF), dict(ranks=0), dict(ranks=1), dict(ranks=3), dict(ranks=7), dict(ranks=10),
       dict(ranks=9), dict(kind=1, ranks=5)]


def test_matte_entry_points_reject_bad_arguments_without_gpu(built):
    from nart_amd import build as nb
    nb.build_hip_lib()
    lib = nart_amd.hip_lib()
    for name in ("nart_hip_matte_defaults", "nart_hip_matte_ids", "nart_hip_render_mattes", "nart_hip_matte_rank",
                 "nart_hip_matte_extract", "nart_hip_matte_timings"):
        assert name in nart_amd.HIP_SYMBOLS
    d = nart_amd.MatteParams.defaults()
    assert (d.kind, d.ranks) == (nart_amd.api.MATTE_MESH, 6)
    lib.nart_hip_matte_defaults(None)  # a null pointer is ignored
    p = nart_amd.default_params()
    buf = np.zeros(8, f32).ctypes.data
    good = nart_amd.MatteParams.defaults(kind=1, ranks=8)
    for c in [None, ctypes.byref(good)] + [ctypes.byref(nart_amd.MatteParams.defaults(**kw)) for kw in BAD]:
        assert lib.nart_hip_render_mattes(None, ctypes.byref(p), c, buf, None, None, None) == -1
        assert lib.nart_hip_matte_rank(None, ctypes.byref(p), c, 4, buf, buf) == -1
        assert lib.nart_hip_matte_extract(None, ctypes.byref(p), c, buf, 1, buf) == -1
    assert lib.nart_hip_matte_rank(None, ctypes.byref(p), None, 33, buf, buf) == -1
    assert lib.nart_hip_matte_timings(None, None, None) == -1
