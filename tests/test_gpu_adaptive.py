"""Adaptive sampling (nart_hip_render_adaptive, `nart --adaptive`) on the device.  The per-bucket
sample counts and errors against the numpy restatement (tests/adaptive_py.py, validated on the CPU by
tests/test_adaptive_restatement.py), bit for bit; the frame against the oracle's tiles at the sample
count every bucket ended on, bit for bit; and the paths around it."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import adaptive_py as ad
import exr_py
import moment_py as mp
import nart_amd
import oracle
from test_aov_restatement import total_frame_uv

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NART = os.path.join(REPO, "nart_amd", "bin", "nart")
f32 = np.float32
INF = float("inf")
IMAGES = ("beauty", "albedo", "normal", "moment")


def _params(scene, w, h, spp, **kw):
    p = nart_amd.load_sessions(scene.path)[0]
    p.image_width, p.image_height, p.spp = w, h, spp
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _at(p, spp):
    q = p.copy()
    q.spp = spp
    return q


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bits_equal(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _report(a, b):
    ne = _bits(a) != _bits(b)
    idx = np.argwhere(ne)
    return "%d of %d floats differ, first at %s" % (int(ne.sum()), ne.size, idx[0].tolist() if len(idx) else None)


def _ap(**kw):
    return nart_amd.AdaptiveParams.defaults(**kw)


@pytest.fixture(scope="module")
def glass_renderer(gpu, glass_scene):
    r = nart_amd.HipRenderer(glass_scene)
    yield r
    r.close()


# ---------------------------------------------------------------- 1. sample counts and errors, bit for bit
CONFIGS = {"b16_fw2": dict(bucket_size=16, filter_width=2.0), "b12_fw1": dict(bucket_size=12, filter_width=1.0),
           # buckets of 92 x 4 and 3 x 4 traced pixels: beyond 89 pixels a side k_bucket_error does not stage in LDS
           "b92_fw1": dict(bucket_size=92, filter_width=1.0)}
SIZES = {"b92_fw1": (93, 2)}
FLOOR = 0.01
_restated = {}


def _median_gap(E):
    """The midpoint of two adjacent distinct level-0 errors near the median, as a float32 strictly
    between them: some buckets stop at level 0 and some refine."""
    d = np.unique(np.asarray(E, f32)[np.isfinite(E)])
    assert len(d) >= 2, d
    k = len(d) // 2
    thr = f32((np.float64(d[k - 1]) + np.float64(d[k])) / 2)
    assert d[k - 1] < thr < d[k], (d[k - 1], thr, d[k])
    return float(thr)


def _restated_selection(scene, cfg):
    """The restated selection loop of glassSphere 24 x 20 (93 x 2 for the wide bucket), levels
    2 / 4 / 8, over the device's own per-sample Li_alpha; once per configuration, shared read-only."""
    if cfg not in _restated:
        w, h = SIZES.get(cfg, (24, 20))
        p = _params(scene, w, h, 8, **CONFIGS[cfg])
        g = nart_amd.session_geometry(p)
        r = nart_amd.HipRenderer(scene)
        samples = {}

        def samples_of(spp):
            if spp not in samples:
                samples[spp] = np.ascontiguousarray(r.render_samples(_at(p, spp), 0, 0, g.total_width, g.total_height))
            return samples[spp]

        first, tiles = [], []
        spp, err, lists, thr = ad.select(p, 2, 2, _median_gap, FLOOR, samples_of, first_errors=first, tiles_out=tiles)
        r.close()
        _restated[cfg] = dict(p=p, spp=spp, err=err, lists=lists, thr=thr, first=first, tiles=tiles)
    return _restated[cfg]


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_bucket_spp_and_error_bit_for_bit(gpu, glass_scene, cfg):
    want = _restated_selection(glass_scene, cfg)
    p = want["p"]
    g = nart_amd.session_geometry(p)
    print(cfg, "level-0 errors", want["first"], "threshold", want["thr"], "spp", want["spp"].tolist())
    assert nart_amd.adaptive_levels(_ap(min_spp=2, growth=2), 8) == [2, 4, 8]
    r = nart_amd.HipRenderer(glass_scene)
    st = nart_amd.RenderStats()
    out = r.render_adaptive(p, _ap(min_spp=2, growth=2, threshold=want["thr"], floor=FLOOR), stats=st)
    r.close()
    assert out["levels"] == [2, 4, 8] and out["adaptive_ms"] > 0
    assert out["bucket_spp"].shape == out["bucket_error"].shape == (g.n_buckets_y, g.n_buckets_x)
    assert out["bucket_spp"].dtype == np.uint32 and out["bucket_error"].dtype == f32
    assert len(np.unique(out["bucket_spp"])) >= 2, out["bucket_spp"]
    assert np.array_equal(out["bucket_spp"].reshape(-1), want["spp"]), (out["bucket_spp"], want["spp"])
    assert _bits_equal(out["bucket_error"].reshape(-1), want["err"]), (out["bucket_error"], want["err"])
    # stats add up over the levels: every list at its level's sample count
    own = [ad.own_size(p, g, b) for b in range(g.n_buckets_x * g.n_buckets_y)]
    traced = sum(L * sum(own[b][0] * own[b][1] for b in ids) for L, ids in zip([2, 4, 8], want["lists"]))
    assert st.traced_samples == traced and st.kernel_launches == len(want["lists"])
    spp_map = nart_amd.spp_image(p, out["bucket_spp"])
    H, W = p.image_height, p.image_width
    assert spp_map.shape == (H, W) and spp_map.dtype == np.uint32
    assert st.samples == sum(int((spp_map >= L).sum()) * L for L in [2, 4, 8][:len(want["lists"])])
    B = p.bucket_size
    assert spp_map[0, 0] == out["bucket_spp"][0, 0]
    assert spp_map[H - 1, W - 1] == out["bucket_spp"][(H - 1) // B, (W - 1) // B]


# ---------------------------------------------------------------- 2. the frame against the oracle
@pytest.mark.parametrize("cfg", ["b16_fw2", "b12_fw1"])
def test_frame_against_oracle(gpu, glass_scene, cfg):
    """Every bucket's tile is its tile of a uniform render at the sample count it ended on: the
    beauty assembled from the oracle's tiles, the moment image and the AOVs from the restated tiles
    (the device's per-sample records, splatted by the AddSample restatement)."""
    want = _restated_selection(glass_scene, cfg)
    p, spp = want["p"], want["spp"]
    g = nart_amd.session_geometry(p)
    nb, tpx = g.n_buckets_x * g.n_buckets_y, g.tile_size * g.tile_size
    r = nart_amd.HipRenderer(glass_scene)
    out = r.render_adaptive(p, _ap(min_spp=2, growth=2, threshold=want["thr"], floor=FLOOR), albedo=True,
                            normal=True, moment=True)
    assert np.array_equal(out["bucket_spp"].reshape(-1), spp)
    orc = oracle.Oracle(glass_scene)
    tiles = {name: np.zeros((nb, tpx, 5), f32) for name in IMAGES}
    for L, ids, _beauty, moment in want["tiles"]:
        ended = [b for b in ids if spp[b] == L]
        if not ended:
            continue
        pl = _at(p, L)
        tiles["beauty"][ended] = orc.render_buckets(pl, ended)
        tiles["moment"][ended] = moment[[ids.index(b) for b in ended]].reshape(len(ended), tpx, 5)
        rec, _tri = r.render_aov_samples(pl, 0, 0, g.total_width, g.total_height)
        uv = total_frame_uv(pl)
        for name, lo in (("albedo", 0), ("normal", 4)):
            t, _ = ad.restate_tiles(pl, uv, np.ascontiguousarray(rec[..., lo:lo + 4]), ended, with_moment=False)
            tiles[name][ended] = t.reshape(len(ended), tpx, 5)
    for name in IMAGES:
        img = nart_amd.combine_tiles(p, tiles[name])
        assert _bits_equal(out[name], img), (name, _report(out[name], img))
    # the beauty alone, and each image without the others, are the same images
    assert _bits_equal(r.render_adaptive(p, _ap(min_spp=2, growth=2, threshold=want["thr"], floor=FLOOR))["beauty"],
                       out["beauty"])
    r.close()


def test_single_level_frames_are_the_uniform_frames(gpu, glass_scene, glass_renderer):
    r = glass_renderer
    p = _params(glass_scene, 24, 20, 8, bucket_size=16)
    low = r.render_aovs(_at(p, 2), moment=True)
    out = r.render_adaptive(p, _ap(min_spp=2, growth=2, threshold=INF), albedo=True, normal=True, moment=True)
    for name in IMAGES:
        assert _bits_equal(out[name], low[name]), (name, _report(out[name], low[name]))
    top = r.render_aovs(p, moment=True)
    for kw in (dict(min_spp=8), dict(min_spp=100)):
        out = r.render_adaptive(p, _ap(threshold=0.0, **kw), albedo=True, normal=True, moment=True)
        for name in IMAGES:
            assert _bits_equal(out[name], top[name]), (kw, name, _report(out[name], top[name]))


# ---------------------------------------------------------------- 3. degenerate loops
def test_degenerate_loops(gpu, glass_scene, glass_renderer):
    r = glass_renderer
    p = _params(glass_scene, 24, 20, 8, bucket_size=16)
    st0, st = nart_amd.RenderStats(), nart_amd.RenderStats()
    r.render(_at(p, 2), st0)
    out = r.render_adaptive(p, _ap(min_spp=2, growth=2, threshold=INF), stats=st)
    assert (out["bucket_spp"] == 2).all() and out["levels"] == [2, 4, 8]
    assert st.samples == st0.samples == 24 * 20 * 2 and st.traced_samples == st0.traced_samples
    assert st.kernel_launches == st0.kernel_launches
    first = out["bucket_error"].copy()
    for min_spp in (8, 64):
        st = nart_amd.RenderStats()
        out = r.render_adaptive(p, _ap(min_spp=min_spp, growth=2, threshold=0.0), stats=st)
        assert out["levels"] == [8] and (out["bucket_spp"] == 8).all() and st.samples == 24 * 20 * 8
    out = r.render_adaptive(p, _ap(min_spp=2, growth=2, threshold=0.0))
    assert ((out["bucket_spp"] == 8) == (first > 0)).all() and (out["bucket_spp"][first == 0] == 2).all()
    assert (first > 0).any()


# ---------------------------------------------------------------- 4. batches
def _batches(sizes, limit=256):
    """render_buckets' greedy batching of buckets of `sizes` traced pixels."""
    n, fill = 0, None
    for s in sizes:
        if fill is None or fill + s > limit:
            n, fill = n + 1, 0
        fill += s
    return n


def test_adaptive_batches(gpu, glass_scene, monkeypatch):
    """NART_BATCH_BYTES=1 leaves 256 slots (tests/test_gpu_moment.py test_moment_batches): every
    level's list goes in several batches, each writing at its own offset of the scratch slabs."""
    want = _restated_selection(glass_scene, "b16_fw2")
    p = want["p"]
    g = nart_amd.session_geometry(p)
    ap = _ap(min_spp=2, growth=2, threshold=0.0, floor=FLOOR)
    one = nart_amd.HipRenderer(glass_scene)
    ref = one.render_adaptive(p, ap, albedo=True, normal=True, moment=True)
    one.close()
    monkeypatch.setenv("NART_BATCH_BYTES", "1")
    r = nart_amd.HipRenderer(glass_scene)
    st = nart_amd.RenderStats()
    out = r.render_adaptive(p, ap, albedo=True, normal=True, moment=True, stats=st)
    r.close()
    spp = ref["bucket_spp"].reshape(-1)
    per_level = []
    for L in (2, 4, 8):
        ids = [b for b in range(len(spp)) if spp[b] >= L]
        per_level.append(_batches([nx * ny for nx, ny in (ad.own_size(p, g, b) for b in ids)]))
    print("batches per level", per_level)
    assert all(n >= 2 for n in per_level), per_level
    assert st.kernel_launches == sum(per_level)
    for name in IMAGES + ("bucket_spp", "bucket_error"):
        assert _bits_equal(out[name], ref[name]), name


# ---------------------------------------------------------------- 5. two ranks
def test_two_rank_rehearsal(gpu, glass_scene, glass_renderer):
    p = _params(glass_scene, 64, 48, 8)
    first = glass_renderer.render_adaptive(p, _ap(min_spp=2, growth=2, threshold=INF))["bucket_error"]
    ap = _ap(min_spp=2, growth=2, threshold=_median_gap(first.reshape(-1)))
    single = glass_renderer.render_adaptive(p, ap, albedo=True, normal=True, moment=True)
    assert len(np.unique(single["bucket_spp"])) >= 2
    m = nart_amd.HipRenderer(glass_scene, devices=[0, 0])
    assert m.devices() == (2, False)
    st = nart_amd.RenderStats()
    got = m.render_adaptive(p, ap, albedo=True, normal=True, moment=True, stats=st)
    for name in IMAGES + ("bucket_spp", "bucket_error"):
        assert _bits_equal(got[name], single[name]), (name, _report(got[name], single[name]))
    assert got["adaptive_ms"] > 0
    spp_map = nart_amd.spp_image(p, got["bucket_spp"])
    assert st.samples == sum(int((spp_map >= L).sum()) * L for L in (2, 4, 8))
    alone = m.render_adaptive(p, ap)
    assert _bits_equal(alone["beauty"], single["beauty"]) and set(alone) & set(IMAGES) == {"beauty"}
    assert _bits_equal(m.render(p), glass_renderer.render(p))
    m.close()


def test_widest_frame_two_ranks_in_batches(gpu, glass_scene, monkeypatch):
    """The widest request one frame carries -- adaptive, both first-hit AOVs and the moment image --
    on two ranks whose every level goes in several batches (NART_BATCH_BYTES=1 leaves 256 slots),
    against the same call on one device in one batch: test_moment_batches' frame (28 x 24 total, four
    buckets), threshold 0, so every bucket refines once and both levels run."""
    p = _params(glass_scene, 24, 20, 4, **CONFIGS["b16_fw2"])
    g = nart_amd.session_geometry(p)
    assert (g.total_width, g.total_height, g.n_buckets_x * g.n_buckets_y) == (28, 24, 4)
    ap = _ap(min_spp=2, growth=2, threshold=0.0)
    one = nart_amd.HipRenderer(glass_scene)
    st1 = nart_amd.RenderStats()
    ref = one.render_adaptive(p, ap, albedo=True, normal=True, moment=True, stats=st1)
    one.close()
    assert (ref["bucket_spp"] == 4).all()
    monkeypatch.setenv("NART_BATCH_BYTES", "1")
    m = nart_amd.HipRenderer(glass_scene, devices=[0, 0])
    st = nart_amd.RenderStats()
    got = m.render_adaptive(p, ap, albedo=True, normal=True, moment=True, stats=st)
    m.close()
    for name in IMAGES + ("bucket_spp",):
        assert _bits_equal(got[name], ref[name]), (name, _report(got[name], ref[name]))
    assert (st.samples, st.traced_samples) == (st1.samples, st1.traced_samples)


# ---------------------------------------------------------------- 6. volume integrator
def test_adaptive_volume_session(gpu, volume_scenes):
    vol = volume_scenes["c5"]
    p = _params(vol, 24, 20, 8, bucket_size=16)
    g = nart_amd.session_geometry(p)
    r = nart_amd.HipRenderer(vol)
    low = r.render_aovs(_at(p, 2), albedo=False, normal=False, moment=True)
    out = r.render_adaptive(p, _ap(min_spp=2, growth=2, threshold=INF), moment=True)
    assert _bits_equal(out["beauty"], low["beauty"]) and _bits_equal(out["moment"], low["moment"])
    assert _bits_equal(out["beauty"], r.render(_at(p, 2)))
    full = r.render_adaptive(p, _ap(min_spp=2, growth=2, threshold=0.0))
    assert (full["bucket_spp"][out["bucket_error"] > 0] == 8).all() and (out["bucket_error"] > 0).any()
    with pytest.raises(nart_amd.NartError) as e:
        r.render_adaptive(p, _ap(min_spp=2), albedo=True)
    assert e.value.code == -6  # NART_E_UNSUPPORTED: first-hit AOVs need surfaces
    img = np.zeros((g.total_height, g.total_width, 5), f32)
    rc = nart_amd.hip_lib().nart_hip_render_adaptive(r._ctx, ctypes.byref(p), None, nart_amd.api.AOV_NORMAL,
                                                     img.ctypes.data, None, img.ctypes.data, None, None, None, None, None)
    assert rc == -6
    assert _bits_equal(r.render(_at(p, 2)), low["beauty"])
    r.close()


# ---------------------------------------------------------------- 7. the denoiser on mixed sample counts
def test_denoiser_on_mixed_sample_counts(gpu, glass_scene, glass_renderer):
    r = glass_renderer
    p = _params(glass_scene, 48, 48, 16)
    g = nart_amd.session_geometry(p)
    first = r.render_adaptive(p, _ap(min_spp=2, growth=2, threshold=INF))["bucket_error"]
    out = r.render_adaptive(p, _ap(min_spp=2, growth=2, threshold=_median_gap(first.reshape(-1))), albedo=True,
                            normal=True, moment=True)
    assert len(np.unique(out["bucket_spp"])) >= 2
    got = r.denoise(p, out["beauty"], out["albedo"], out["normal"], moment=out["moment"])
    want = mp.denoise(48, 48, g.filter_bounds, out["beauty"], out["albedo"], out["normal"], out["moment"])
    assert _bits_equal(got, want), _report(got, want)
    assert np.isfinite(got).all()


# ---------------------------------------------------------------- 8. errors
def test_errors_leave_the_context_usable(gpu, glass_scene, glass_renderer):
    r = glass_renderer
    p = _params(glass_scene, 32, 24, 4)
    g = nart_amd.session_geometry(p)
    good, aov, dn = r.render(p), r.render_aovs(p), r.render_denoised(p)
    bad = [dict(min_spp=1), dict(min_spp=0), dict(growth=1), dict(growth=17), dict(threshold=-0.5),
           dict(threshold=float("nan")), dict(floor=0.0), dict(floor=-1.0), dict(floor=INF), dict(floor=float("nan"))]
    for kw in bad:
        with pytest.raises(nart_amd.NartError) as e:
            r.render_adaptive(p, _ap(**kw))
        assert e.value.code == -1, kw
        assert _bits_equal(r.render(p), good), kw
    with pytest.raises(nart_amd.NartError) as e:
        r.render_adaptive(_at(p, 1), _ap(min_spp=2))
    assert e.value.code == -1 and "spp" in str(e.value)
    lib = nart_amd.hip_lib()
    img = np.zeros((g.total_height, g.total_width, 5), f32)
    ptr = img.ctypes.data
    call = lambda ctx, pp, aovs, alb, nrm: lib.nart_hip_render_adaptive(ctx, pp, None, aovs, ptr, alb, nrm, None, None,
                                                                        None, None, None)
    assert call(None, ctypes.byref(p), 0, None, None) == -1
    assert call(r._ctx, None, 0, None, None) == -1
    assert call(r._ctx, ctypes.byref(p), 0x4, ptr, ptr) == -1       # an unknown bit
    assert call(r._ctx, ctypes.byref(p), 0x1, None, ptr) == -1      # a bit without its buffer
    assert _bits_equal(r.render(p), good)
    # everything optional left out: the per-bucket outputs alone
    spp = np.zeros(g.n_buckets_x * g.n_buckets_y, np.uint32)
    rc = lib.nart_hip_render_adaptive(r._ctx, ctypes.byref(p), None, 0, None, None, None, None, spp.ctypes.data, None,
                                      None, None)
    assert rc == 0 and set(spp.tolist()) <= {4}  # the defaults' first level is 16 >= 4: the one level 4
    # the other entry points after adaptive calls: the bits they had before
    r.render_adaptive(p, _ap(min_spp=2, growth=2, threshold=0.0), albedo=True, normal=True, moment=True)
    assert _bits_equal(r.render(p), good)
    again = r.render_aovs(p)
    for name in ("beauty", "albedo", "normal"):
        assert _bits_equal(again[name], aov[name]), name
    assert _bits_equal(r.render_denoised(p)["denoised"], dn["denoised"])


# ---------------------------------------------------------------- 9. CLI
def test_cli_adaptive(gpu, glass_scene, tmp_path):
    base = [NART, glass_scene.path]
    size = ["-w", "48", "-h", "32", "-s", "8"]
    p = nart_amd.parse_args(["nart", glass_scene.path, "out"] + size)
    p = nart_amd.load_sessions(glass_scene.path, p)[0]
    g = nart_amd.session_geometry(p)
    r = nart_amd.HipRenderer(glass_scene)
    first = r.render_adaptive(p, _ap(min_spp=2, threshold=INF))["bucket_error"]
    thr = _median_gap(first.reshape(-1))
    api = r.render_adaptive(p, _ap(min_spp=2, threshold=thr), albedo=True, normal=True, moment=True)
    api_dn = r.denoise(p, api["beauty"], api["albedo"], api["normal"], moment=api["moment"])
    r.close()
    assert len(np.unique(api["bucket_spp"])) >= 2

    def run(out, extra):
        res = subprocess.run(base + [out] + size + extra, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
        return res.stdout

    a_dir, d_dir, bad_dir = tmp_path / "a", tmp_path / "d", tmp_path / "bad"
    for d in (a_dir, d_dir, bad_dir):
        d.mkdir()
    flags = ["--adaptive", repr(thr), "--min-spp", "2"]
    stdout = run(str(a_dir / "out"), flags)
    assert sorted(os.listdir(a_dir)) == ["out.exr", "out.spp.exr"]
    line = [ln for ln in stdout.splitlines() if ln.startswith("Adaptive:")]
    spp_map = nart_amd.spp_image(p, api["bucket_spp"])
    taken = sum(int((spp_map >= L).sum()) * L for L in (2, 8))
    assert len(line) == 1 and "2 spp x %d buckets" % (g.n_buckets_x * g.n_buckets_y) in line[0]
    assert "8 spp x %d buckets" % int((api["bucket_spp"] == 8).sum()) in line[0]
    assert "%d of %d samples" % (taken, 48 * 32 * 8) in line[0], line
    run(str(d_dir / "out"), flags + ["--denoise", "--sample-variance"])
    assert sorted(os.listdir(d_dir)) == ["out.denoised.exr", "out.exr", "out.spp.exr"]
    assert (d_dir / "out.exr").read_bytes() == (a_dir / "out.exr").read_bytes()
    to_half = nart_amd.scene_lib().nart_float_to_half
    halves_of = lambda a: np.array([to_half(ctypes.c_float(v)) for v in a.reshape(-1)], np.uint16).reshape(a.shape)
    for path, img in ((a_dir / "out.exr", api["beauty"]), (d_dir / "out.denoised.exr", api_dn)):
        halves, _hdr = exr_py.read_rgba_halves(str(path))
        assert halves.shape == (32, 48, 4) and np.array_equal(halves, halves_of(nart_amd.finalize(p, img))), path
    # --aovs --denoise: the adaptive call's AOVs, and the spatial denoiser over the adaptive images
    s_dir = tmp_path / "s"
    s_dir.mkdir()
    run(str(s_dir / "out"), flags + ["--aovs", "--denoise"])
    assert sorted(os.listdir(s_dir)) == ["out.albedo.exr", "out.denoised.exr", "out.exr", "out.normal.exr", "out.spp.exr"]
    r = nart_amd.HipRenderer(glass_scene)
    api_sp = r.denoise(p, api["beauty"], api["albedo"], api["normal"])
    r.close()
    for name, img in (("out.exr", api["beauty"]), ("out.albedo.exr", api["albedo"]), ("out.normal.exr", api["normal"]),
                      ("out.denoised.exr", api_sp)):
        halves, _hdr = exr_py.read_rgba_halves(str(s_dir / name))
        assert np.array_equal(halves, halves_of(nart_amd.finalize(p, img))), name
    halves, _hdr = exr_py.read_rgba_halves(str(a_dir / "out.spp.exr"))
    spp_rgba = np.stack([spp_map.astype(f32)] * 3 + [np.ones_like(spp_map, f32)], axis=-1)
    assert np.array_equal(halves, halves_of(spp_rgba))
    # --min-spp alone: an error before anything is loaded or rendered
    res = subprocess.run(base + [str(bad_dir / "out")] + size + ["--min-spp", "2"], capture_output=True, text=True,
                         timeout=300)
    assert res.returncode != 0 and "--adaptive" in res.stderr and not res.stdout
    assert os.listdir(bad_dir) == []


# ---------------------------------------------------------------- 10. quality (measured, not tuned)
@pytest.mark.parametrize("name", ["cornell", "glass"])
def test_quality_adaptive(gpu, request, name):
    """128 x 128, levels 4 / 16 / 64 at the default threshold and floor, against 512 spp of the same
    renderer, with test_quality_sample_variance's relMSE = mean((x - ref)^2 / (ref^2 + 0.01)) over the
    pixels whose 512-spp coverage is >= 0.999.  Asserted: the adaptive frame beats the uniform 4-spp
    frame and takes fewer samples than 64 spp everywhere.  Printed: relMSE and samples of the
    adaptive frame, of uniform 64 spp and of the uniform render whose budget is nearest the adaptive
    one (the figures are in DESIGN.md, "Adaptive sampling")."""
    scene = request.getfixturevalue({"cornell": "cornell_scene", "glass": "glass_scene"}[name])
    r = nart_amd.HipRenderer(scene)
    p64, p512 = _params(scene, 128, 128, 64), _params(scene, 128, 128, 512)
    ref = r.render_aovs(p512, normal=False)
    st = nart_amd.RenderStats()
    out = r.render_adaptive(p64, _ap(min_spp=4, growth=4), stats=st)
    near = max(1, int(round(st.samples / (128.0 * 128.0))))
    uniform = {spp: r.render(_at(p64, spp)) for spp in sorted({4, near, 64})}
    r.close()
    mask = nart_amd.finalize(p512, ref["albedo"])[..., 3] >= 0.999
    x_ref = nart_amd.finalize(p512, ref["beauty"])[..., :3].astype(np.float64)

    def rel_mse(img):
        x = nart_amd.finalize(p64, img)[..., :3].astype(np.float64)
        return float((((x - x_ref) ** 2) / (x_ref ** 2 + 0.01))[mask].mean())

    e_ad, e = rel_mse(out["beauty"]), {spp: rel_mse(img) for spp, img in uniform.items()}
    counts = {int(L): int((out["bucket_spp"] == L).sum()) for L in out["levels"]}
    print("%s 128x128 max 64 spp: adaptive relMSE %.5f with %d samples (%.1f per pixel, buckets ending per level %s); "
          "uniform 4 spp %.5f, %d spp (nearest budget) %.5f, 64 spp %.5f with %d samples"
          % (name, e_ad, st.samples, st.samples / 16384.0, counts, e[4], near, e[near], e[64], 16384 * 64))
    assert mask.any() and e_ad < e[4], (e_ad, e[4])
    assert st.samples < 128 * 128 * 64
