"""The cost image on the device (nart_hip_render_cost, nart_hip_render_cost_samples, nart_hip_cost_image,
`nart --cost`; include/nart_hip.h, "Cost image").  Integers are compared exactly everywhere.  Yardsticks:
the unchanged oracle's path counts for the sums of words 0 and 2 (and a bound for word 1: the device skips
a shadow ray whose term is exactly zero), the counter pass of a plain render for words 0, 1 and 2, and for
all four words, `steps` included, a counter-pass render of every bucket on its own with variant 3: a
one-lane-per-pixel k_render launch without probe, queue or k_primary, every ray through the same
trav_step.  The beauty of every cost render must have render()'s bits.  Oracle counts are rendered once
per session and shared (cost_py.oracle_counts)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cost_py
import exr_py
import nart_amd

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NART = os.path.join(REPO, "nart_amd", "bin", "nart")
E_INVALID, E_UNSUPPORTED = -1, -6
PLAIN = {"priority", "spec_pairs", "half_waves", "lean", "specialized", "primary"}  # what a cost frame never runs
bits_equal, report = cost_py.dc.bits_equal, cost_py.dc.report


@pytest.fixture(scope="module")
def frames(gpu, tmp_path_factory):
    return cost_py.dc.lg.shared_frames(tmp_path_factory)


def _check(frames, key, spp=1):
    """render_cost of a frame on a fresh context: the grid's shape, the totals against the oracle and
    against the counter pass of a plain render, the beauty against render().  Returns (renderer, p, out,
    schedule names)."""
    name, p = cost_py.frame_params(frames, key, spp)
    r = nart_amd.HipRenderer(frames.scene(name))
    st = nart_amd.RenderStats()
    out = r.render_cost(p, with_beauty=True, stats=st)
    cost = out["cost"]
    g = nart_amd.session_geometry(p)
    assert cost.dtype == np.uint32 and cost.shape == nart_amd.cost_grid(p) + (4,) == cost_py.grid_shape(p, g) + (4,)
    want = cost_py.oracle_counts(frames, key, spp)
    sums = [int(cost[..., k].sum(dtype=np.uint64)) for k in range(4)]
    print(key, spp, "cost sums", sums, "oracle", want)
    assert out["totals"] == tuple(sums)
    assert sums[0] == want["extension_queries"]
    assert sums[2] == want["shaded_hits"]
    assert 0 < sums[1] <= want["visibility_queries"]
    assert sums[3] > 0
    assert st.traced_samples == want["traced_samples"] == cost.shape[0] * cost.shape[1] * spp
    assert np.array_equal(out["buckets"], cost_py.bucket_sums(p, g, cost))
    assert out["reduce_ms"] > 0
    assert r.scene_features()[1] == nart_amd.api.FT_ALL  # the generic build
    names = set(st.schedule_names())
    assert not names & PLAIN, names
    plain = r.render(p)
    assert bits_equal(out["beauty"], plain), report(out["beauty"], plain)
    # the parent's counter pass: a plain render of the frame on the default variant
    rc = nart_amd.HipRenderer(frames.scene(name))
    rc.set_counters(True)
    cs = nart_amd.RenderStats()
    assert bits_equal(rc.render(p, stats=cs), plain)
    print(key, spp, "counter pass", cs.rays_extend, cs.rays_shadow, cs.bounces)
    assert (cs.rays_extend, cs.rays_shadow, cs.bounces) == (sums[0], sums[1], sums[2])
    return r, p, out, names


def test_materials_direct(frames):
    """50x37, bucket 16, filter width 1.5: ragged buckets, one lane per pixel."""
    _r, _p, _out, names = _check(frames, "materials_direct")
    assert not names & {"probe_queue", "wave_groups"}, names


def test_materials_pixel_queue(frames):
    """432x300: the probe-ordered pixel queue, without priority lanes or speculative pairs."""
    _r, _p, _out, names = _check(frames, "materials_queue")
    assert "probe_queue" in names, names


def test_materials_wave_groups(frames):
    """1056x750: the persistent grid's waves take 64-slot groups, a lane several pixels in turn."""
    _r, _p, _out, names = _check(frames, "materials_groups")
    assert "wave_groups" in names, names


@pytest.mark.parametrize("key", ["veach", "ring"])
def test_reference_scenes(frames, key):
    _check(frames, key)


@pytest.mark.parametrize("key", ["env", "envc"])
def test_environment(frames, key):
    """The ENV build."""
    _check(frames, key)


def test_nested_glass_deep_lists(frames):
    """bounces 16: the EXT build."""
    _r, p, _out, _names = _check(frames, "nested")
    assert p.bounces == 16


def test_eight_spp(frames):
    _check(frames, "materials_direct", 8)


def test_every_bucket_alone_on_k_render(frames):
    """All four words per bucket, `steps` included: materials 50x37, bucket 16, 4 spp; every bucket on its
    own through variant 3 with the counters on."""
    import torch
    name, p = cost_py.frame_params(frames, "materials_direct", 4)
    out = nart_amd.HipRenderer(frames.scene(name)).render_cost(p)
    g = nart_amd.session_geometry(p)
    nb = g.n_buckets_x * g.n_buckets_y
    assert out["buckets"].shape == (g.n_buckets_y, g.n_buckets_x, 4) and nb == 12
    rk = nart_amd.HipRenderer(frames.scene(name), variant=3)
    rk.set_counters(True)
    tiles = torch.zeros((1, g.tile_size * g.tile_size, 5), dtype=torch.float32, device="cuda")
    got = np.zeros((nb, 4), np.uint64)
    for b in range(nb):
        st = nart_amd.RenderStats()
        rk.render_buckets_async(p, np.array([b], np.uint32), tiles.data_ptr(), torch.cuda.current_stream().cuda_stream, st)
        torch.cuda.synchronize()
        assert not set(st.schedule_names()) & {"probe_queue", "wave_groups", "primary"}
        got[b] = (st.rays_extend, st.rays_shadow, st.bounces, st.node_visits + st.tri_tests)
    want = out["buckets"].reshape(nb, 4)
    print("k_render per bucket", got.tolist(), "cost buckets", want.tolist())
    assert np.array_equal(got[:, :3], want[:, :3])
    assert np.array_equal(got[:, 3], want[:, 3])
    assert (want[:, 3] > 0).all()


def _rect_check(frames, key, spp, x0, y0):
    name, p = cost_py.frame_params(frames, key, spp)
    r = nart_amd.HipRenderer(frames.scene(name))
    rec = r.render_cost_samples(p, x0, y0, 8, 8)
    assert rec.shape == (8, 8, spp, 4) and rec.dtype == np.uint32
    assert cost_py.sample_invariants(rec, p.bounces) == []
    assert (rec[..., 3] > 0).all()  # the scene renders geometry: every camera ray visits the root
    # the rect is another launch shape than the frame: the records depend on the sample alone
    grid = r.render_cost(p)["cost"]
    assert np.array_equal(rec.sum(axis=2, dtype=np.uint64), grid[y0:y0 + 8, x0:x0 + 8].astype(np.uint64))
    return rec


def test_per_sample_records(frames):
    rec = _rect_check(frames, "materials_direct", 8, 20, 14)
    assert (rec[..., 0] > 1).any() and (rec[..., 1] > 0).any()
    assert len(np.unique(rec[..., 3])) > 8  # the steps differ from sample to sample


def test_per_sample_records_nested(frames):
    rec = _rect_check(frames, "nested", 4, 20, 14)
    assert (rec[..., 0] > 10).any()  # paths beyond the register list's depth


def test_several_batches(frames, monkeypatch):
    """NART_BATCH_BYTES so small that the frame takes several batches: the records are sized per batch and
    every batch reduces into the one grid."""
    name, p = cost_py.frame_params(frames, "materials_direct", 8)
    r = nart_amd.HipRenderer(frames.scene(name))
    whole = r.render_cost(p, with_beauty=True)
    monkeypatch.setenv("NART_BATCH_BYTES", str(300000))
    st = nart_amd.RenderStats()
    out = r.render_cost(p, with_beauty=True, stats=st)
    assert st.kernel_launches >= 3
    assert np.array_equal(out["cost"], whole["cost"]) and bits_equal(out["beauty"], whole["beauty"])


def test_two_devices(frames):
    name, p = cost_py.frame_params(frames, "materials_direct", 4)
    one = nart_amd.HipRenderer(frames.scene(name)).render_cost(p, with_beauty=True)
    r = nart_amd.HipRenderer(frames.scene(name), devices=[0, 0])
    two = r.render_cost(p, with_beauty=True)
    assert np.array_equal(two["cost"], one["cost"]) and two["totals"] == one["totals"]
    assert bits_equal(two["beauty"], one["beauty"])
    assert np.array_equal(r.render_cost_samples(p, 20, 14, 2, 2),  # (runs on the first device)
                          nart_amd.HipRenderer(frames.scene(name)).render_cost_samples(p, 20, 14, 2, 2))


def test_cost_image(frames):
    """Bit for bit against cost_py.cost_image, grid columns and rows beyond the total image included."""
    name, p = cost_py.frame_params(frames, "materials_direct", 8)
    r = nart_amd.HipRenderer(frames.scene(name))
    g = nart_amd.session_geometry(p)
    gh, gw = nart_amd.cost_grid(p)
    assert gw + g.filter_bounds > g.total_width and gh + g.filter_bounds > g.total_height  # some fall outside
    cost = r.render_cost(p)["cost"]
    img = r.cost_image(p, cost)
    assert img.shape == (g.total_height, g.total_width, 5)
    assert bits_equal(img, cost_py.cost_image(p, g, cost)), report(img, cost_py.cost_image(p, g, cost))
    assert r.cost_timings()["image_ms"] > 0
    mean = nart_amd.finalize(p, img)
    want = cost[:p.image_height, :p.image_width].astype(np.float32) / np.float32(p.spp)
    assert bits_equal(mean, want)
    # counts that float32 cannot hold exactly round to nearest even
    rng = np.random.RandomState(11)
    big = rng.randint(0, 2 ** 32, size=cost.shape, dtype=np.uint64).astype(np.uint32)
    big[0, 0] = (2 ** 24 + 1, 2 ** 24 + 3, 2 ** 32 - 1, 2 ** 32 - 129)
    got = r.cost_image(p, big)
    assert bits_equal(got, cost_py.cost_image(p, g, big)), report(got, cost_py.cost_image(p, g, big))
    with pytest.raises(ValueError):
        r.cost_image(p, big[:-1])


def _halves(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float32).astype(np.float16).view(np.uint16)


def test_cli(frames, tmp_path):
    path = frames.base["materials"]
    out = str(tmp_path / "out")
    flags = ["-w", "50", "-h", "37", "-s", "4"]
    run = subprocess.run([NART, path, out] + flags + ["--cost"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    p = nart_amd.load_sessions(path, nart_amd.parse_args(["nart", path, out] + flags))[0]
    assert p.spp == 4
    r = nart_amd.HipRenderer(frames.scene("materials"))
    res = r.render_cost(p)
    assert ("Writing to %s.cost.exr..." % out) in run.stdout
    assert ("Cost: %d extension rays, %d shadow rays, %d shaded hits, %d traversal steps" % res["totals"]) in run.stdout
    halves, _hdr = exr_py.read_rgba_halves(out + ".cost.exr")
    assert np.array_equal(halves, _halves(nart_amd.finalize(p, r.cost_image(p, res["cost"]))))
    plain = subprocess.run([NART, path, out + "p"] + flags, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and not os.path.exists(out + "p.cost.exr")
    a, _ = exr_py.read_rgba_halves(out + ".exr")
    b, _ = exr_py.read_rgba_halves(out + "p.exr")
    assert np.array_equal(a, b)
    # refused combinations: a message, a non-zero exit, nothing rendered
    for extra in (["--depth-cuts", "1,2"], ["--light-groups", "each"], ["--adaptive", "0.1"], ["--robust"], ["--mattes"],
                  ["--aovs"], ["--denoise"], ["--aovs", "--follow-specular"]):
        bad = subprocess.run([NART, path, out + "x"] + flags + ["--cost"] + extra, capture_output=True, text=True, timeout=300)
        assert bad.returncode != 0 and bad.stderr.startswith("Error: --cost is not offered"), (extra, bad.stdout, bad.stderr)
        assert "Rendering" not in bad.stdout and not os.path.exists(out + "x.exr")


def _raises(code, call):
    with pytest.raises(nart_amd.NartError) as e:
        call()
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


def test_errors_leave_the_context_usable(frames, volume_scenes):
    name, p = cost_py.frame_params(frames, "materials_direct", 8)
    r = nart_amd.HipRenderer(frames.scene(name))
    want = r.render(p)
    good = r.render_cost(p)["cost"]

    def usable():
        assert bits_equal(r.render(p), want)

    # a null grid, image or record buffer
    _raises(E_INVALID, lambda: r.render_cost(p, cost=False))
    assert r._lib.nart_hip_render_cost_samples(r._ctx, ctypes.byref(p), 0, 0, 2, 2, None) == E_INVALID
    assert r._lib.nart_hip_cost_image(r._ctx, ctypes.byref(p), None, good.ctypes.data) == E_INVALID
    assert r._lib.nart_hip_cost_image(r._ctx, ctypes.byref(p), good.ctypes.data, None) == E_INVALID
    w = ctypes.c_uint32()
    assert r._lib.nart_hip_cost_grid(ctypes.byref(p), None, ctypes.byref(w)) == E_INVALID
    usable()
    # a bad rect
    g = nart_amd.session_geometry(p)
    _raises(E_INVALID, lambda: r.render_cost_samples(p, 0, 0, 0, 2))
    _raises(E_INVALID, lambda: r.render_cost_samples(p, g.total_width - 1, 0, 2, 2))
    usable()
    # variant 3 runs k_render, which has no cost build
    r.set_variant(3)
    assert "cost image" in _raises(E_UNSUPPORTED, lambda: r.render_cost(p))
    assert "cost image" in _raises(E_UNSUPPORTED, lambda: r.render_cost_samples(p, 0, 0, 2, 2))
    usable()
    r.set_variant(0)
    assert np.array_equal(r.render_cost(p)["cost"], good)
    # with the counters on a cost render reports no work counts: the grid holds them
    r.set_counters(True)
    st = nart_amd.RenderStats()
    assert np.array_equal(r.render_cost(p, stats=st)["cost"], good)
    assert (st.rays_extend, st.rays_shadow, st.bounces, st.node_visits, st.tri_tests) == (0, 0, 0, 0, 0)
    assert st.traced_samples == good.shape[0] * good.shape[1] * p.spp
    r.set_counters(False)
    usable()
    # the volume integrator has no cost build
    vs = volume_scenes["c5"]
    rv = nart_amd.HipRenderer(vs)
    pv = nart_amd.load_sessions(vs.path)[0]
    pv.image_width, pv.image_height, pv.spp = 32, 24, 2
    assert pv.integrator == 1 and pv.bounces >= 1
    before = rv.render(pv)
    assert "cost image" in _raises(E_UNSUPPORTED, lambda: rv.render_cost(pv))
    assert "cost image" in _raises(E_UNSUPPORTED, lambda: rv.render_cost_samples(pv, 0, 0, 2, 2))
    assert bits_equal(rv.render(pv), before)
