"""The device ray traversal on chosen rays (nart_hip_trace) against the reference octree restated on the CPU
(oracle.trace_n): the winning triangle, the bits of t and the Isect fields, bit for bit, for every scene
of trace_cases.py, on the host SAH tree and on the device LBVH, through every traversal entry point of the
render kernels.  No tolerance ("Probing the traversal").  test_trace_cases.py shows on the CPU
that the rays reach every class of trouble; the rays trace_cases.set_aside names (the one documented
non-emulated case, test_octree_nan_case.py) are the only ones not compared.
"""
import ctypes
import os

import numpy as np
import pytest

import nart_amd
import oracle
import trace_cases as tc

pytestmark = pytest.mark.gpu

f32 = np.float32
CLOSEST, ANY = nart_amd.TRACE_CLOSEST, nart_amd.TRACE_ANY
# (variant, sk): sk 0 = the whole stack in LDS, "depth" = a short stack that holds every level
VARIANTS = [("plain", 0), ("lds", 0), ("step", 0), ("step", 1), ("step", 2), ("step", "depth"),
            ("step_rot", 0), ("step_rot", 1), ("step_rot", 2), ("step_rot", "depth"), ("packet", 0)]
RESULT = np.r_[0:2, 6:26]  # the words that answer the query (2-5 are the counters)


@pytest.fixture(scope="module")
def scene_dir(gpu, tmp_path_factory):
    return str(tmp_path_factory.mktemp("trace"))


_CTX = {}


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    """The contexts _context made live as long as this module's tests."""
    yield
    for _, r in _CTX.values():
        r.close()
    _CTX.clear()


def _context(name, build, scene_dir):
    """(prepared scene, its context on the given tree builder), made once per module (closed by _close_contexts)."""
    if (name, build) not in _CTX:
        prep = tc.prepared(name, scene_dir)
        old = os.environ.pop("NART_BVH_BUILD", None)
        try:
            if build == "device":
                os.environ["NART_BVH_BUILD"] = "device"
            r = nart_amd.HipRenderer(prep["scene"])
        finally:
            os.environ.pop("NART_BVH_BUILD", None)
            if old is not None:
                os.environ["NART_BVH_BUILD"] = old
        assert r.bvh()["on_device"] == (build == "device")
        _CTX[(name, build)] = (prep, r)
    return _CTX[(name, build)]


def _sk(r, sk):
    return r.bvh()["stack_depth"] if sk == "depth" else min(sk, r.bvh()["stack_depth"])


def _closest(prep):
    return prep["rays"][:, 7].view(np.uint32) == CLOSEST


@pytest.mark.parametrize("variant,sk", VARIANTS, ids=["%s-sk%s" % v for v in VARIANTS])
@pytest.mark.parametrize("build", tc.BUILDERS)
@pytest.mark.parametrize("name", tc.SCENES)
def test_device_matches_oracle(scene_dir, name, build, variant, sk):
    prep, r = _context(name, build, scene_dir)
    keep = ~tc.set_aside(prep)
    if variant == "packet":  # closest queries only; a wave's 64 rays drawn from all classes
        keep &= _closest(prep)
        idx = np.random.default_rng(7).permutation(np.nonzero(keep)[0])
    else:
        idx = np.nonzero(keep)[0]
    got = np.zeros_like(prep["want"])
    got[idx] = r.trace(prep["rays"][idx], variant, _sk(r, sk))
    bad = np.intersect1d(tc.compare(got, prep["want"]), idx)
    print("%s %s %s sk %s: %d rays, %d differ" % (name, build, variant, sk, len(idx), len(bad)))
    assert len(bad) == 0, tc.describe(prep, got, prep["want"], bad)


@pytest.mark.parametrize("build", tc.BUILDERS)
@pytest.mark.parametrize("name", tc.SCENES)
def test_variants_agree_and_counting_changes_nothing(scene_dir, name, build):
    """Every entry point returns the same record for every compared ray -- the packet for waves of coherent
    rays (the sets in their order) as for incoherent ones -- and the counting builds return the answers of
    the plain ones."""
    prep, r = _context(name, build, scene_dir)
    keep = ~tc.set_aside(prep)
    rays = prep["rays"]
    base = r.trace(rays, "plain")
    assert not base[:, 2:6].any() and not base[:, 26:].any()
    for variant, sk in VARIANTS[1:]:
        m = keep & _closest(prep) if variant == "packet" else keep
        for count in (False, True):
            got = r.trace(rays[m], variant, _sk(r, sk), count=count)
            assert np.array_equal(got[:, RESULT], base[m][:, RESULT]), (variant, sk, count)
    counted = r.trace(rays, "plain", count=True)
    assert np.array_equal(counted[keep][:, RESULT], base[keep][:, RESULT])
    if r.bvh()["num_leaf_tris"]:
        assert counted[:, 3].max() > 0  # triangle tests were counted


@pytest.mark.parametrize("name", [n for n in tc.SCENES if n != "empty"])
def test_origins_beyond_the_padding_are_measured(scene_dir, name):
    """Origins at trace_cases.BEYOND scene radii, where an ulp of the origin exceeds the padding of the BVH2's
    boxes (trace_cases.designed): the count of rays that differ from the oracle is printed (DESIGN.md has the
    figures), not asserted.  Asserted: the per-lane entry points walk the same tree in the same order, so
    they still agree with each other bit for bit."""
    prep, r = _context(name, "host", scene_dir)
    rays, want = prep["beyond"], prep["beyond_want"]
    base = r.trace(rays, "plain")
    print("%s: %d of %d rays beyond the padding differ from the oracle" % (name, len(tc.compare(base, want)), len(rays)))
    for variant, sk in (("lds", 0), ("step", 0), ("step", 1), ("step_rot", 2)):
        assert np.array_equal(r.trace(rays, variant, _sk(r, sk)), base), (variant, sk)


@pytest.mark.parametrize("n", [1, 63, 65, 257])
@pytest.mark.parametrize("variant", ["packet", "step"])
def test_record_count_off_the_wave_and_block_size(scene_dir, variant, n):
    """Exactly n records come back when n is no multiple of the wave (a partial last packet) or the block;
    the rest of the caller's buffer is not written."""
    prep, r = _context("glassSphere", "host", scene_dir)
    idx = np.random.default_rng(11).permutation(np.nonzero(~tc.set_aside(prep) & _closest(prep))[0])[:n + 300]
    rays, want = np.ascontiguousarray(prep["rays"][idx]), prep["want"][idx]
    got = r.trace(rays[:n], variant, 2)
    assert got.shape == (n, nart_amd.TRACE_OUT_WORDS)
    assert len(tc.compare(got, want[:n])) == 0
    buf = np.full((n + 300, nart_amd.TRACE_OUT_WORDS), 0xA5A5A5A5, np.uint32)
    assert nart_amd.hip_lib().nart_hip_trace(r._ctx, nart_amd.TRACE_VARIANTS[variant], 2, 0, rays.ctypes.data, n,
                                             buf.ctypes.data) == 0
    assert len(tc.compare(buf[:n], want[:n])) == 0
    assert np.all(buf[n:] == 0xA5A5A5A5)


def test_replay_and_check_paths_are_reached(scene_dir):
    """A reach condition read from the device's counters (correctness never rests on it): the designed ties
    and NaNs replay the octree search, and hits on the lattice's flat chunk boxes take the exact ancestor
    check."""
    prep, r = _context("lattice", "host", scene_dir)
    c = r.trace(prep["rays"], "plain", count=True)
    flags = prep["want"][:, 2]
    ties = tc.of_class(prep, "edge_axis") & ((flags & oracle.TRACE_TIE_CLOSEST) != 0)
    assert (c[ties, 5] > 0).sum() >= 32, (c[ties, 5] > 0).sum()
    # face hits: rays of the face classes whose hit lies on one of the flat layers (z of the hit point, word 8)
    w = prep["want"]
    on_layer = (w[:, 0] != nart_amd.TRACE_NO_HIT) & np.isin(w[:, 8].view(f32), [-2.0, -0.5, 0.25, 1.0])
    face = (tc.of_class(prep, "edge_axis") | tc.of_class(prep, "origin_on_face")) & on_layer & _closest(prep)
    assert (c[face, 4] > 0).sum() >= 32, (c[face, 4] > 0).sum()
    for name in ("inner_256", "glassSphere"):
        prep, r = _context(name, "host", scene_dir)
        c = r.trace(prep["rays"], "plain", count=True)
        nans = tc.of_class(prep, "nan_plane") & ((prep["want"][:, 2] & oracle.TRACE_NAN_ACCEPTED) != 0)
        assert (c[nans, 5] > 0).sum() >= 32, (name, (c[nans, 5] > 0).sum())


@pytest.mark.parametrize("build", tc.BUILDERS)
def test_short_stack_really_spills(scene_dir, build):
    """The deep soup: one LDS level and the rest in the global column returns the bits of the whole stack in
    LDS, with and without rotated node quarters."""
    prep, r = _context("cluster", build, scene_dir)
    depth = r.bvh()["stack_depth"]
    assert depth >= 4
    for variant in ("step", "step_rot"):
        full = r.trace(prep["rays"], variant, depth)
        for sk in (1, 2, depth - 1):
            assert np.array_equal(r.trace(prep["rays"], variant, sk), full), (variant, sk)
        assert np.array_equal(r.trace(prep["rays"], variant, 0), full), variant


def test_multi_device_context_answers_as_one_device(scene_dir):
    prep, r = _context("glassSphere", "host", scene_dir)
    m = nart_amd.HipRenderer(prep["scene"], devices=[0, 0])
    rays = prep["rays"][::7]
    for variant, sk in (("plain", 0), ("step", 2)):
        assert np.array_equal(m.trace(rays, variant, sk), r.trace(rays, variant, sk)), variant


def test_argument_validation_on_a_live_context(scene_dir):
    prep, r = _context("glassSphere", "host", scene_dir)
    lib, P, V = nart_amd.hip_lib(), ctypes.c_void_p, nart_amd.TRACE_VARIANTS
    depth = r.bvh()["stack_depth"]
    x = np.ascontiguousarray(prep["rays"][:4])
    x[:, 7] = np.zeros(4, np.uint32).view(f32)
    y = np.full((4, nart_amd.TRACE_OUT_WORDS), 3, np.uint32)
    tr = lambda ctx, v, sk, i, n, o: lib.nart_hip_trace(ctx, v, sk, 0, i, n, o)  # noqa: E731
    assert tr(r._ctx, V["plain"], 0, x.ctypes.data, 0, y.ctypes.data) == 0 and np.all(y == 3)
    assert tr(P(), V["plain"], 0, x.ctypes.data, 4, y.ctypes.data) == -1
    assert tr(r._ctx, V["plain"], 0, P(), 4, y.ctypes.data) == -1
    assert tr(r._ctx, V["plain"], 0, x.ctypes.data, 4, P()) == -1
    assert tr(r._ctx, len(V), 0, x.ctypes.data, 4, y.ctypes.data) == -1
    assert tr(r._ctx, 0xFFFFFFFF, 0, x.ctypes.data, 4, y.ctypes.data) == -1
    for v in ("step", "step_rot"):
        assert tr(r._ctx, V[v], depth + 1, x.ctypes.data, 4, y.ctypes.data) == -1
        assert tr(r._ctx, V[v], 0xFFFFFFFF, x.ctypes.data, 4, y.ctypes.data) == -1
    assert tr(r._ctx, V["plain"], 0, x.ctypes.data, (1 << 24) + 1, y.ctypes.data) == -1
    assert tr(r._ctx, V["plain"], 0, x.ctypes.data, 0xFFFFFFFF, y.ctypes.data) == -1
    bad = x.copy()
    bad[2, 7] = np.uint32(2).view(f32)  # no such query kind
    assert tr(r._ctx, V["plain"], 0, bad.ctypes.data, 4, y.ctypes.data) == -1
    bad[2, 7] = np.uint32(ANY).view(f32)  # the packet answers closest queries only
    assert tr(r._ctx, V["packet"], 0, bad.ctypes.data, 4, y.ctypes.data) == -1
    assert np.all(y == 3)
    assert tr(r._ctx, V["step"], depth, x.ctypes.data, 4, y.ctypes.data) == 0 and not np.all(y == 3)
    with pytest.raises(ValueError):
        r.trace(np.zeros((4, 3), f32))
