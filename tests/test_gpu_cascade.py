"""The firefly cascade (nart_hip_render_cascade, nart_hip_cascade_reweight, `nart --robust`) on the
device against its numpy restatement (tests/cascade_py.py, validated on the CPU by
tests/test_cascade_restatement.py): bit for bit, tolerance 0, except the measured quality figures."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cascade_py as cp
import exr_py
import nart_amd
from test_aov_restatement import total_frame_uv
from test_cascade_restatement import BAD, SIZE, TEST

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NART = os.path.join(REPO, "nart_amd", "bin", "nart")
f32 = np.float32


def _params(scene, w, h, spp, **kw):
    p = nart_amd.load_sessions(scene.path)[0]
    p.image_width, p.image_height, p.spp = w, h, spp
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _cp(**kw):
    return nart_amd.CascadeParams.defaults(**kw)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bits_equal(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _report(a, b):
    ne = _bits(a) != _bits(b)
    idx = np.argwhere(ne)
    with np.errstate(all="ignore"):
        worst = float(np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64)))) if ne.any() else 0.0
    return "%d of %d floats differ, max abs diff %g, first at %s" % (int(ne.sum()), ne.size, worst,
                                                                     idx[0].tolist() if len(idx) else None)


def _restated_robust(p, out, c):
    """The reweighting restated over the device's own beauty and layers."""
    g = nart_amd.session_geometry(p)
    return cp.reweight(p.image_width, p.image_height, g.filter_bounds, out["beauty"], out["layers"], out["levels"], p.spp,
                       c.kappa)


# ---------------------------------------------------------------- 1. layers and robust image, bit for bit
CONFIGS = {"b16_fw2": dict(bucket_size=16, filter_width=2.0), "b12_fw1": dict(bucket_size=12, filter_width=1.0)}
_restated = {}


def _restated_layers(scene, key, cfg, spp, c, size=SIZE):
    """The layer images restated over the device's own per-sample Li_alpha of the whole total frame,
    computed once per configuration and shared read-only."""
    k = (key, cfg, spp, c.layers, c.start, c.base, size)
    if k not in _restated:
        p = _params(scene, size[0], size[1], spp, **CONFIGS[cfg])
        g = nart_amd.session_geometry(p)
        r = nart_amd.HipRenderer(scene)
        L = r.render_samples(p, 0, 0, g.total_width, g.total_height)
        r.close()
        levels = cp.levels_of(c.start, c.base, c.layers)
        _restated[k] = (p, cp.restate_layers(p, total_frame_uv(p), np.ascontiguousarray(L), levels, c.base))
    return _restated[k]


def _ran(st, splat_mode, cfg):
    """The splat kernel family the schedule bits report, against the one the mode selects: rows and
    skew need power-of-two buckets (bucket 12 runs the one-pixel-per-lane kernels in every mode)."""
    names = st.schedule_names()
    pow2 = cfg == "b16_fw2"
    return ("splat_rows" in names) == (pow2 and splat_mode == 5) and ("splat_skew" in names) == (pow2 and splat_mode == 4)


CASES = [("b16_fw2", spp, mode) for spp in (2, 3, 5) for mode in (5, 4, 3, 1, 0)] + \
        [("b12_fw1", 2, 5), ("b12_fw1", 2, 0)]


def _check_call(r, p, c, want, st=None):
    out = r.render_robust(p, c, with_beauty=True, with_layers=True, stats=st)
    assert out["layers"].shape == want.shape
    for k in range(c.layers):
        assert _bits_equal(out["layers"][k], want[k]), (k, _report(out["layers"][k], want[k]))
    robust = _restated_robust(p, out, c)
    assert _bits_equal(out["robust"], robust), _report(out["robust"], robust)
    plain = r.render(p)
    assert _bits_equal(out["beauty"], plain)
    for k in range(c.layers):
        assert _bits_equal(out["layers"][k][..., 4], plain[..., 4]), k
    assert out["cascade_ms"] > 0 and out["reweight_ms"] > 0
    return out


@pytest.mark.parametrize("cfg,spp,splat_mode", CASES, ids=["%s-%dspp-mode%d" % c for c in CASES])
def test_cascade_bit_for_bit(gpu, glass_scene, cfg, spp, splat_mode):
    """2, 3 and 5 spp reach the tails of the splat kernels' 4-sample unrolling; every splat family
    gives the restatement's layer bits; the robust image is the restated reweighting of those layers;
    the beauty of the same call is render()'s."""
    c = _cp(**TEST)
    p, want = _restated_layers(glass_scene, "glass", cfg, spp, c)
    assert want[0][..., :3].max() > 0 and want[c.layers - 1][..., :3].max() > 0  # the bulk and the fireflies
    r = nart_amd.HipRenderer(glass_scene, splat_mode=splat_mode)
    st = nart_amd.RenderStats()
    out = _check_call(r, p, c, want, st)
    assert _ran(st, splat_mode, cfg), (splat_mode, st.schedule_names())
    only = r.render_robust(p, c)
    assert set(only) == {"robust", "levels", "cascade_ms", "reweight_ms"} and _bits_equal(only["robust"], out["robust"])
    r.close()


def test_cascade_default_parameters(gpu, glass_scene):
    c = _cp()
    p, want = _restated_layers(glass_scene, "glass", "b16_fw2", 4, c)
    r = nart_amd.HipRenderer(glass_scene)
    out = _check_call(r, p, c, want)
    assert _bits_equal(r.render_robust(p)["robust"], out["robust"])  # params=None: the defaults
    r.close()


# ---------------------------------------------------------------- 2. the reweighting on synthetic inputs
@pytest.fixture(scope="module")
def glass_renderer(gpu, glass_scene):
    r = nart_amd.HipRenderer(glass_scene)
    yield r
    r.close()


SIZES = [(1, 1), (5, 3), (70, 3), (33, 9), (37, 29)]
OFF_DEFAULT = {2: dict(layers=2, start=0.75, base=3.0, kappa=3.5), 8: dict(layers=8, start=0.3, base=2.5, kappa=0.7)}


@pytest.mark.parametrize("K", [2, 8])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_cascade_reweight_synthetic_bit_for_bit(glass_renderer, glass_scene, size, K):
    """Tile edges and halo (32 x 8 tiles: 33, 70 and 37 wide, 9 and 29 high), one pixel, K = 2 (no
    layer above layer 1) and K = 8, a W = 0 pixel and a NaN layer pixel, every parameter off its default."""
    W, H = size
    spp = 3
    p = _params(glass_scene, W, H, spp)
    g = nart_amd.session_geometry(p)
    fb = g.filter_bounds
    c = _cp(**OFF_DEFAULT[K])
    levels = nart_amd.cascade_levels(c)
    assert _bits_equal(levels, cp.levels_of(c.start, c.base, c.layers))
    beauty, layers, spots = cp.synthetic(W, H, fb, levels, spp, seed=W * 131 + H)
    if W * H >= 15:
        assert None not in spots and not np.isfinite(layers).all()
    got = glass_renderer.cascade_reweight(p, beauty, layers, c)
    want = cp.reweight(W, H, fb, beauty, layers, levels, spp, c.kappa)
    assert got["robust"].shape == want.shape == (g.total_height, g.total_width, 5)
    assert _bits_equal(got["robust"], want), _report(got["robust"], want)
    assert got["reweight_ms"] > 0 and got["cascade_ms"] == 0
    if W * H >= 15:
        (zx, zy), (nx, ny) = spots
        assert not got["robust"][zy + fb, zx + fb].any() and np.isnan(got["robust"][ny + fb, nx + fb, 1])
        # kappa matters: another value gives another image
        other = glass_renderer.cascade_reweight(p, beauty, layers, _cp(**dict(OFF_DEFAULT[K], kappa=50.0)))
        assert not _bits_equal(other["robust"], got["robust"])


# ---------------------------------------------------------------- 3. batches, volume, two ranks
def test_cascade_batches(gpu, glass_scene, monkeypatch):
    """NART_BATCH_BYTES=1 leaves 256 slots (tests/test_gpu_moment.py test_moment_batches): the 28 x 24
    total frame's buckets of 256, 192, 128 and 96 traced pixels go in three batches, each splitting and
    splatting its own records into its own offset of the nine back-to-back tile slabs."""
    c = _cp(**TEST)
    p = _params(glass_scene, 24, 20, 2, **CONFIGS["b16_fw2"])
    one = nart_amd.HipRenderer(glass_scene)
    ref = one.render_robust(p, c, with_beauty=True, with_layers=True)
    one.close()
    monkeypatch.setenv("NART_BATCH_BYTES", "1")
    r = nart_amd.HipRenderer(glass_scene)
    st = nart_amd.RenderStats()
    out = r.render_robust(p, c, with_beauty=True, with_layers=True, stats=st)
    r.close()
    assert st.kernel_launches == 3
    for name in ("robust", "beauty", "layers"):
        assert _bits_equal(out[name], ref[name]), (name, _report(out[name], ref[name]))


def test_cascade_volume_session(gpu, volume_scenes):
    vol = volume_scenes["emissive"]
    c = _cp(**TEST)
    p, want = _restated_layers(vol, "vol", "b16_fw2", 2, c, size=(24, 20))
    assert want[..., :3].max() > 0
    r = nart_amd.HipRenderer(vol)
    _check_call(r, p, c, want)
    r.close()


def test_two_rank_rehearsal(gpu, glass_scene, glass_renderer):
    p = _params(glass_scene, 64, 48, 4)
    c = _cp(**TEST)
    single = glass_renderer.render_robust(p, c, with_beauty=True, with_layers=True)
    m = nart_amd.HipRenderer(glass_scene, devices=[0, 0])
    assert m.devices() == (2, False)
    got = m.render_robust(p, c, with_beauty=True, with_layers=True)
    for name in ("robust", "beauty", "layers"):
        assert _bits_equal(got[name], single[name]), (name, _report(got[name], single[name]))
    assert got["cascade_ms"] > 0 and got["reweight_ms"] > 0
    alone = m.render_robust(p, c)
    assert _bits_equal(alone["robust"], single["robust"])
    rew = m.cascade_reweight(p, got["beauty"], got["layers"], c)
    assert _bits_equal(rew["robust"], single["robust"])
    assert _bits_equal(m.render(p), glass_renderer.render(p))
    m.close()


# ---------------------------------------------------------------- 4. errors, and the other entry points' bits
def test_cascade_errors_leave_the_context_usable(gpu, glass_scene, glass_renderer):
    r = glass_renderer
    p = _params(glass_scene, 32, 24, 2)
    g = nart_amd.session_geometry(p)
    good = r.render(p)
    ok = r.render_robust(p, with_beauty=True, with_layers=True)
    lib = nart_amd.hip_lib()
    img = np.zeros((g.total_height, g.total_width, 5), f32)
    lay = np.zeros((9, g.total_height, g.total_width, 5), f32)
    P, ptr = ctypes.byref(p), lambda a: a.ctypes.data
    for kw in BAD:
        c = _cp(**kw)
        for call in (lambda: r.render_robust(p, c), lambda: r.cascade_reweight(p, ok["beauty"], ok["layers"], c)):
            with pytest.raises(nart_amd.NartError) as e:
                call()
            assert e.value.code == -1, kw
        # the entry points themselves, on a live context
        assert lib.nart_hip_render_cascade(r._ctx, P, ctypes.byref(c), ptr(img), None, None, None) == -1, kw
        assert lib.nart_hip_cascade_reweight(r._ctx, P, ctypes.byref(c), ptr(img), ptr(lay), ptr(img)) == -1, kw
        assert "cascade" in lib.nart_hip_last_error(r._ctx).decode()
    assert _bits_equal(r.render(p), good)
    assert lib.nart_hip_render_cascade(r._ctx, P, None, None, ptr(img), ptr(lay), None) == -1     # no image
    assert lib.nart_hip_render_cascade(r._ctx, None, None, ptr(img), None, None, None) == -1      # no params
    assert lib.nart_hip_cascade_reweight(r._ctx, P, None, None, ptr(lay), ptr(img)) == -1
    assert lib.nart_hip_cascade_reweight(r._ctx, P, None, ptr(img), None, ptr(img)) == -1
    assert lib.nart_hip_cascade_reweight(r._ctx, P, None, ptr(img), ptr(lay), None) == -1
    p0 = _params(glass_scene, 32, 24, 0)
    assert lib.nart_hip_render_cascade(r._ctx, ctypes.byref(p0), None, ptr(img), None, None, None) == -1  # spp < 1
    assert lib.nart_hip_cascade_reweight(r._ctx, ctypes.byref(p0), None, ptr(img), ptr(lay), ptr(img)) == -1
    assert _bits_equal(r.render(p), good)
    again = r.render_robust(p, with_beauty=True, with_layers=True)
    for name in ("robust", "beauty", "layers"):
        assert _bits_equal(again[name], ok[name]), name


def test_other_entry_points_keep_their_bits(gpu, glass_scene):
    """render, render_aovs(moment=True) and render_denoised give the same bits, launches and schedule
    before and after cascade calls on the same context."""
    p = _params(glass_scene, 48, 32, 4)
    r = nart_amd.HipRenderer(glass_scene)

    def snapshot():
        st = nart_amd.RenderStats()
        a = r.render(p, st)
        b = r.render_aovs(p, moment=True)
        d = r.render_denoised(p)
        return {"render": a, "albedo": b["albedo"], "normal": b["normal"], "moment": b["moment"], "beauty": b["beauty"],
                "denoised": d["denoised"]}, (st.kernel_launches, st.schedule)

    before, st_before = snapshot()
    r.render_robust(p, _cp(**TEST), with_beauty=True, with_layers=True)
    r.render_robust(p)
    after, st_after = snapshot()
    assert st_before == st_after
    for name in before:
        assert _bits_equal(before[name], after[name]), name
    r.close()


# ---------------------------------------------------------------- 5. CLI
def test_cli_robust(gpu, glass_scene, tmp_path):
    base = [NART, glass_scene.path]
    size = ["-w", "48", "-h", "32", "-s", "4"]

    def run(out, extra):
        res = subprocess.run(base + [out] + size + extra, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
        return res.stdout

    d_dir, k_dir, bad_dir = tmp_path / "d", tmp_path / "k", tmp_path / "bad"
    for d in (d_dir, k_dir, bad_dir):
        d.mkdir()
    run(str(d_dir / "out"), ["--robust"])
    # KAPPA after the flag; a following flag is not taken for it
    res = subprocess.run(base + [str(k_dir / "out"), "--robust", "0.5"] + size, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-2000:])
    assert sorted(os.listdir(d_dir)) == sorted(os.listdir(k_dir)) == ["out.exr", "out.robust.exr"]
    p = nart_amd.parse_args(["nart", glass_scene.path, "out"] + size)
    p = nart_amd.load_sessions(glass_scene.path, p)[0]
    g = nart_amd.session_geometry(p)
    r = nart_amd.HipRenderer(glass_scene)
    api = r.render_robust(p, with_beauty=True, with_layers=True)
    r.close()
    to_half = nart_amd.scene_lib().nart_float_to_half

    def halves_of(img):
        final = nart_amd.finalize(p, img)
        return np.array([to_half(ctypes.c_float(v)) for v in final.reshape(-1)], np.uint16).reshape(final.shape)

    restated = {kappa: cp.reweight(48, 32, g.filter_bounds, api["beauty"], api["layers"], api["levels"], p.spp, kappa)
                for kappa in (2.0, 0.5)}
    assert not _bits_equal(restated[2.0], restated[0.5])
    for d, kappa in ((d_dir, 2.0), (k_dir, 0.5)):
        for name, img in (("out.exr", api["beauty"]), ("out.robust.exr", restated[kappa])):
            halves, _hdr = exr_py.read_rgba_halves(str(d / name))
            assert halves.shape == (32, 48, 4) and np.array_equal(halves, halves_of(img)), (name, kappa)
    # not offered together with the denoiser, the AOVs or adaptive sampling; a bad kappa
    for extra in (["--robust", "--denoise"], ["--robust", "--aovs"], ["--robust", "--adaptive", "0.1"],
                  ["--robust", "0"]):
        res = subprocess.run(base + [str(bad_dir / "out")] + size + extra, capture_output=True, text=True, timeout=300)
        assert res.returncode != 0 and "--robust" in res.stderr and not res.stdout, extra
    assert os.listdir(bad_dir) == []


# ---------------------------------------------------------------- 6. quality (measured, not tuned)
@pytest.mark.parametrize("name", ["cornell", "glass"])
def test_quality_robust(gpu, request, name):
    """128 x 128, 16 spp with the default parameters against 512 spp of the same renderer, with
    test_quality_adaptive's relMSE = mean((x - ref)^2 / (ref^2 + 0.01)) over the pixels whose 512-spp
    coverage is >= 0.999.  Asserted: on glassSphere the robust image beats the noisy one; on both
    scenes the robust image's summed rgb does not exceed the beauty's by more than rounding (omega
    <= 1 and rounding is monotonic, so per pixel robust <= the float32 sum of the layer means, which
    differs from the beauty's mean by the split's and the splat sums' rounding: about 16 spp x 25
    footprint pixels x 2 layer terms additions of non-negative terms, each within 2^-23 relative, so
    1e-4 of the sum bounds it).  Printed: relMSE and the energy kept at kappa 1, 2 (the default) and
    4 (the figures are in DESIGN.md, "Firefly cascade")."""
    scene = request.getfixturevalue({"cornell": "cornell_scene", "glass": "glass_scene"}[name])
    r = nart_amd.HipRenderer(scene)
    p16, p512 = _params(scene, 128, 128, 16), _params(scene, 128, 128, 512)
    ref = r.render_aovs(p512, normal=False)
    out = {kappa: r.render_robust(p16, _cp(kappa=kappa), with_beauty=True) for kappa in (1.0, 2.0, 4.0)}
    r.close()
    assert nart_amd.CascadeParams.defaults().kappa == 2.0
    mask = nart_amd.finalize(p512, ref["albedo"])[..., 3] >= 0.999
    x_ref = nart_amd.finalize(p512, ref["beauty"])[..., :3].astype(np.float64)

    def rel_mse(img):
        x = nart_amd.finalize(p16, img)[..., :3].astype(np.float64)
        return float((((x - x_ref) ** 2) / (x_ref ** 2 + 0.01))[mask].mean())

    def energy(img):
        return float(np.nan_to_num(nart_amd.finalize(p16, img)[..., :3].astype(np.float64)).sum())

    noisy, e_noisy = rel_mse(out[2.0]["beauty"]), energy(out[2.0]["beauty"])
    fig = {kappa: (rel_mse(o["robust"]), energy(o["robust"]) / e_noisy) for kappa, o in out.items()}
    print("%s 128x128 16 spp: mask keeps %.3f, relMSE noisy %.5f; robust (relMSE, energy kept) %s; cascade_ms %.3f "
          "reweight_ms %.3f" % (name, mask.mean(), noisy, ", ".join("kappa %g: %.5f, %.4f" % ((k,) + fig[k]) for k in fig),
                                out[2.0]["cascade_ms"], out[2.0]["reweight_ms"]))
    assert mask.any()
    for kappa in fig:
        assert fig[kappa][1] <= 1 + 1e-4, (kappa, fig[kappa])
    if name == "glass":
        assert fig[2.0][0] < noisy, (fig[2.0][0], noisy)
