"""The parts denoise on the device (nart_hip_denoise_parts, nart_hip_render_denoised_light_groups,
nart_hip_render_denoised_depth_layers, `nart --denoise-parts`; include/nart_hip.h, "Denoised parts"):
every denoised part against the denoiser run on that part alone -- its numpy restatement
(tests/denoise_py.py) and the device's own denoise() -- bit for bit, tolerance 0, whatever K and whatever
the chunking; the sum against parts_sum (tests/denoise_parts_py.py).

Part k of the designed inputs is the same image for every K (tests/test_denoise_parts_restatement.py), so
the two references of a part are computed once per size, filter width and parameters and shared."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import denoise_parts_py as dnp
import denoise_py as dn
import exr_py
import nart_amd

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NART = os.path.join(REPO, "nart_amd", "bin", "nart")
E_INVALID, E_UNSUPPORTED = -1, -6
f32 = np.float32


def _params(scene, w, h, spp, **kw):
    p = nart_amd.load_sessions(scene.path)[0]
    p.image_width, p.image_height, p.spp = w, h, spp
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _report(a, b):
    ne = _bits(a) != _bits(b)
    idx = np.argwhere(ne)
    with np.errstate(all="ignore"):
        worst = float(np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64)))) if ne.any() else 0.0
    return "%d of %d floats differ, max abs diff %g, first at %s" % (int(ne.sum()), ne.size, worst,
                                                                     idx[0].tolist() if len(idx) else None)


@pytest.fixture(scope="module")
def glass_renderer(gpu, glass_scene):
    r = nart_amd.HipRenderer(glass_scene)
    yield r
    r.close()


# ---------------------------------------------------------------- 1. synthetic inputs, bit for bit
SIZES = [(1, 1), (5, 3), (70, 3), (37, 29), (129, 65)]
_REFS = {}


class Case:
    """The nine designed parts of one size, filter width and parameter set, and per part the two
    references: the restatement and the device's denoise() of that part alone (computed on first use)."""

    def __init__(self, r, scene, W, H, fw, dp_kw):
        self.r, self.W, self.H = r, W, H
        self.p = _params(scene, W, H, 1, filter_width=fw)
        self.fb = nart_amd.session_geometry(self.p).filter_bounds
        assert self.fb == int(fw)
        self.parts, self.albedo, self.normal = dnp.synthetic_parts(W, H, self.fb, dnp.PARTS_MAX, seed=W * 131 + H)
        self.dp = nart_amd.DenoiseParams.defaults(**dp_kw)
        self.want = {}

    def reference(self, k):
        if k not in self.want:
            restated = dn.denoise(self.W, self.H, self.fb, self.parts[k], self.albedo, self.normal, self.dp)
            device = self.r.denoise(self.p, self.parts[k], self.albedo, self.normal, self.dp)
            assert _same(device, restated), (k, _report(device, restated))
            self.want[k] = restated
        return self.want[k]

    def check(self, K):
        got, total = self.r.denoise_parts(self.p, self.parts[:K], self.albedo, self.normal, self.dp, with_sum=True)
        assert got.shape == (K,) + self.parts.shape[1:]
        for k in range(K):
            assert _same(got[k], self.reference(k)), (K, k, dnp.ROLES[k], _report(got[k], self.reference(k)))
        want_sum = dnp.parts_sum(got)
        assert _same(total, want_sum), (K, _report(total, want_sum))
        assert np.isfinite(got).all()
        plain = self.r.denoise_parts(self.p, self.parts[:K], self.albedo, self.normal, self.dp)  # (no sum asked for)
        assert _same(plain, got)
        return got


def _case(r, scene, W, H, fw, **dp_kw):
    key = (W, H, fw, tuple(sorted(dp_kw.items())))
    if key not in _REFS:
        _REFS[key] = Case(r, scene, W, H, fw, dp_kw)
    return _REFS[key]


@pytest.mark.parametrize("fw", [2.0, 1.0], ids=["fw2", "fw1"])
@pytest.mark.parametrize("iterations", [1, 5])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_synthetic_bit_for_bit(glass_renderer, glass_scene, monkeypatch, size, iterations, fw):
    """K = 1, 2, 4, 5, 9 on the automatic plan.  Tiles are 32 x 8 with up to 4 pixels of halo: 129 x 65
    crosses them raggedly on both axes, 70 x 3 is lower than every halo, 1 x 1 and 5 x 3 smaller than a
    window; 1 iteration stays in the LDS passes, 5 reach the global ones."""
    monkeypatch.delenv("NART_DN_PARTS_CHUNK", raising=False)
    c = _case(glass_renderer, glass_scene, size[0], size[1], fw, iterations=iterations)
    for K in (1, 2, 4, 5, 9):
        got = c.check(K)
        border = np.ones(got.shape[1:3], bool)
        border[c.fb:c.fb + c.H, c.fb:c.fb + c.W] = False
        assert not got[:, border].any() and (got[:, ~border][..., 4] == 1).all()
    t = glass_renderer.denoise_parts_timings()
    assert t["prepare"] > 0 and t["variance"] > 0 and t["finalize"] > 0 and t["sum"] == 0  # (the last call asked for none)
    assert all(x > 0 for x in t["passes"][:iterations]) and not any(t["passes"][iterations:])


@pytest.mark.parametrize("chunk", [1, 2, 3, 4])
def test_every_chunk_shape(glass_renderer, glass_scene, monkeypatch, chunk):
    """K = 5 and 9 with the chunk size forced: every chunk kernel, and a ragged last chunk (5 = 2+2+1 =
    3+2 = 4+1, 9 = 4+4+1), on a size with several tiles and one below a tile."""
    monkeypatch.setenv("NART_DN_PARTS_CHUNK", str(chunk))
    for W, H in ((129, 65), (37, 29)):
        c = _case(glass_renderer, glass_scene, W, H, 2.0, iterations=5)
        for K in (5, 9):
            c.check(K)


def test_other_parameters_bit_for_bit(glass_renderer, glass_scene, monkeypatch):
    """Every parameter away from its default, 8 iterations (step 128 on a 37 x 29 image)."""
    monkeypatch.delenv("NART_DN_PARTS_CHUNK", raising=False)
    c = _case(glass_renderer, glass_scene, 37, 29, 2.0, iterations=8, normal_squarings=2, sigma_color=1.5, sigma_depth=2.5,
              depth_eps=0.01, sigma_coverage=0.2, albedo_floor=0.05)
    c.check(5)
    # null params are the defaults
    a = glass_renderer.denoise_parts(c.p, c.parts[:2], c.albedo, c.normal)
    b = glass_renderer.denoise_parts(c.p, c.parts[:2], c.albedo, c.normal, nart_amd.DenoiseParams.defaults())
    assert _same(a, b)


# ---------------------------------------------------------------- 2-5. whole frames
def _check_groups(r, ref, p, groups):
    """render_denoised_light_groups on r against render_light_groups, render_aovs and denoise on ref."""
    out = r.render_denoised_light_groups(p, groups, with_groups=True, with_beauty=True)
    noisy = ref.render_light_groups(p, groups, with_beauty=True)
    aov = ref.render_aovs(p, beauty=False)
    assert _same(out["groups"], noisy["groups"]), _report(out["groups"], noisy["groups"])
    assert _same(out["beauty"], noisy["beauty"])
    for g in range(len(noisy["groups"])):
        want = ref.denoise(p, noisy["groups"][g], aov["albedo"], aov["normal"])
        assert _same(out["denoised"][g], want), (g, _report(out["denoised"][g], want))
    assert _same(out["sum"], dnp.parts_sum(out["denoised"]))
    assert out["denoise_ms"] > 0 and out["guides_ms"] > 0
    return out


def test_light_groups(gpu, materials_scene):
    """The two-light materials scene, one group per light."""
    r = nart_amd.HipRenderer(materials_scene)
    p = _params(materials_scene, 64, 48, 4)
    out = _check_groups(r, r, p, [0, 1])
    assert not _same(out["denoised"][0], out["groups"][0])  # the filter did something
    # relighting takes the denoised groups as it takes the noisy ones
    mixed = r.light_mix(p, out["denoised"], [1.0, 0.5])
    assert np.isfinite(mixed).all() and _same(mixed[..., 3:], out["denoised"][0][..., 3:])
    only = r.render_denoised_light_groups(p, [0, 1], with_sum=False)
    assert set(only) == {"denoised", "denoise_ms", "guides_ms"} and _same(only["denoised"], out["denoised"])
    r.close()


def _check_layers(r, ref, p, cuts, guides=None):
    out = r.render_denoised_depth_layers(p, cuts, guides=guides, with_layers=True, with_beauty=True)
    noisy = ref.render_depth_cuts(p, cuts, with_beauty=True)
    layers = ref.depth_layers(p, noisy["cuts"], noisy["beauty"])
    aov = ref.render_aovs(p, beauty=False) if guides is None else ref.render_guides(p, guides, beauty=False)
    assert _same(out["layers"], layers), _report(out["layers"], layers)
    assert _same(out["beauty"], noisy["beauty"])
    assert len(out["denoised"]) == len(cuts) + 1
    for k in range(len(layers)):
        want = ref.denoise(p, layers[k], aov["albedo"], aov["normal"])
        assert _same(out["denoised"][k], want), (k, _report(out["denoised"][k], want))
    assert _same(out["sum"], dnp.parts_sum(out["denoised"]))
    return out, aov


def test_depth_layers(glass_renderer, glass_scene):
    p = _params(glass_scene, 48, 48, 4)
    out, _aov = _check_layers(glass_renderer, glass_renderer, p, (1, 2))
    assert not _same(out["denoised"][1], out["layers"][1])
    t = glass_renderer.denoise_parts_timings()
    assert t["sum"] > 0 and t["guides_ms"] > 0 and all(x > 0 for x in t["passes"][:5])


def test_followed_guides(glass_renderer, glass_scene):
    """max_follow = 8: the guides are render_guides' images, which differ from the first-hit AOVs behind
    the glass."""
    p = _params(glass_scene, 48, 48, 4)
    gp = nart_amd.GuideParams.defaults(max_follow=8)
    out, guides = _check_layers(glass_renderer, glass_renderer, p, (1, 2), guides=gp)
    first = glass_renderer.render_aovs(p, beauty=False)
    assert not _same(guides["albedo"], first["albedo"])
    plain = glass_renderer.render_denoised_depth_layers(p, (1, 2))
    assert not _same(out["denoised"], plain["denoised"])


def test_multi_device_matches_single(gpu, materials_scene, glass_scene, glass_renderer):
    """Two ranks rehearsed on one device: gathered as before, denoised on the first device."""
    m = nart_amd.HipRenderer(materials_scene, devices=[0, 0])
    single = nart_amd.HipRenderer(materials_scene)
    assert m.devices() == (2, False)
    _check_groups(m, single, _params(materials_scene, 64, 48, 4), [0, 1])
    m.close()
    single.close()
    m = nart_amd.HipRenderer(glass_scene, devices=[0, 0])
    p = _params(glass_scene, 48, 48, 4)
    _check_layers(m, glass_renderer, p, (1, 2))
    c = _case(glass_renderer, glass_scene, 37, 29, 2.0, iterations=5)
    got = m.denoise_parts(c.p, c.parts[:5], c.albedo, c.normal, c.dp)
    for k in range(5):
        assert _same(got[k], c.reference(k)), k
    m.close()


# ---------------------------------------------------------------- 6. errors
def test_errors_leave_the_context_usable(gpu, glass_scene, glass_renderer, volume_scenes):
    vol = volume_scenes["c5"]
    pv = _params(vol, 32, 24, 2)
    rv = nart_amd.HipRenderer(vol)
    for call in (lambda: rv.render_denoised_depth_layers(pv, (1,)),
                 lambda: rv.render_denoised_light_groups(pv, [0] * vol.counts()["lights"])):
        with pytest.raises(nart_amd.NartError) as e:
            call()
        assert e.value.code == E_UNSUPPORTED and "volume" in str(e.value)
    rv.close()

    r = glass_renderer
    p = _params(glass_scene, 32, 24, 2)
    before = r.render_denoised(p)
    c = _case(r, glass_scene, 37, 29, 2.0, iterations=5)
    shape = c.parts.shape[1:]
    for K in (0, 10):
        with pytest.raises(nart_amd.NartError) as e:
            r.denoise_parts(c.p, np.zeros((K,) + shape, f32), c.albedo, c.normal)
        assert e.value.code == E_INVALID and "n_parts" in str(e.value)
    for kw in (dict(iterations=0), dict(iterations=9), dict(sigma_color=0.0), dict(albedo_floor=float("nan"))):
        bad = nart_amd.DenoiseParams.defaults(**kw)
        for call in (lambda: r.denoise_parts(c.p, c.parts[:2], c.albedo, c.normal, bad),
                     lambda: r.render_denoised_depth_layers(p, (1, 2), bad)):
            with pytest.raises(nart_amd.NartError) as e:
                call()
            assert e.value.code == E_INVALID, kw
    for call in (lambda: r.render_denoised_depth_layers(p, (2, 1)), lambda: r.render_denoised_depth_layers(p, ()),
                 lambda: r.render_denoised_depth_layers(p, (1, p.bounces + 1)),
                 lambda: r.render_denoised_light_groups(p, [0, 0, 0, 0, 0, 0, 0]),  # (not the scene's light count)
                 lambda: r.render_denoised_depth_layers(p, (1,), guides=nart_amd.GuideParams.defaults(max_follow=11))):
        with pytest.raises(nart_amd.NartError) as e:
            call()
        assert e.value.code == E_INVALID
    lib = nart_amd.hip_lib()
    out = np.zeros((2,) + shape, f32)
    ptr = lambda a: a.ctypes.data
    good = (ptr(c.parts), ptr(c.albedo), ptr(c.normal), ptr(out))
    for i in range(4):
        args = list(good)
        args[i] = None
        assert lib.nart_hip_denoise_parts(r._ctx, ctypes.byref(c.p), None, 2, *args, None, None) == E_INVALID, i
    assert lib.nart_hip_denoise_parts(r._ctx, None, None, 2, *good, None, None) == E_INVALID
    cuts = np.array([1, 2], np.uint32)
    assert lib.nart_hip_render_denoised_depth_layers(r._ctx, ctypes.byref(p), None, None, ptr(cuts), 2, None, None, None, None,
                                                     None, None) == E_INVALID
    assert lib.nart_hip_render_denoised_depth_layers(r._ctx, ctypes.byref(p), None, None, None, 2, ptr(out), None, None, None,
                                                     None, None) == E_INVALID
    one = np.zeros(1, np.uint32)
    assert lib.nart_hip_render_denoised_light_groups(r._ctx, ctypes.byref(p), None, None, ptr(one), 1, 1, None, None, None,
                                                     None, None, None) == E_INVALID
    assert not out.any()
    # the context renders and denoises as it did before the failed calls, and after good ones
    c.check(2)
    after = r.render_denoised(p)
    for name in ("denoised", "beauty"):
        assert _same(after[name], before[name]), name


# ---------------------------------------------------------------- 7. CLI
def _halves(p, image):
    final = nart_amd.finalize(p, image)
    to_half = nart_amd.scene_lib().nart_float_to_half
    return np.array([to_half(ctypes.c_float(v)) for v in final.reshape(-1)], np.uint16).reshape(final.shape)


def _run(args, ok=True):
    run = subprocess.run([NART] + args, capture_output=True, text=True, timeout=300)
    if ok:
        assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    return run


def test_cli(gpu, materials_scene, glass_scene, glass_renderer, tmp_path):
    flags = ["-w", "48", "-h", "32", "-s", "4"]
    # light groups, with gains
    d = tmp_path / "lg"
    d.mkdir()
    path = materials_scene.path
    log = _run([path, str(d / "out")] + flags + ["--light-groups", "each", "--light-gains", "1,0.5", "--denoise-parts"]).stdout
    assert sorted(os.listdir(d)) == ["out.denoised.exr", "out.exr", "out.light.00.denoised.exr", "out.light.00.exr",
                                     "out.light.01.denoised.exr", "out.light.01.exr", "out.mix.denoised.exr", "out.mix.exr"]
    assert ("Writing to %s..." % (d / "out.light.01.denoised.exr")) in log
    p = nart_amd.load_sessions(path, nart_amd.parse_args(["nart", path, "out"] + flags))[0]
    r = nart_amd.HipRenderer(materials_scene)
    api = r.render_denoised_light_groups(p, [0, 1], with_groups=True, with_beauty=True)
    want = {"out.exr": api["beauty"], "out.denoised.exr": api["sum"], "out.light.00.exr": api["groups"][0],
            "out.light.01.exr": api["groups"][1], "out.light.00.denoised.exr": api["denoised"][0],
            "out.light.01.denoised.exr": api["denoised"][1], "out.mix.exr": r.light_mix(p, api["groups"], [1.0, 0.5]),
            "out.mix.denoised.exr": r.light_mix(p, api["denoised"], [1.0, 0.5])}
    r.close()
    for name, img in want.items():
        halves, _hdr = exr_py.read_rgba_halves(str(d / name))
        assert halves.shape == (32, 48, 4) and np.array_equal(halves, _halves(p, img)), name
    # depth cuts; the noisy layers only with --depth-layers; the followed guides next to it
    path = glass_scene.path
    p = nart_amd.load_sessions(path, nart_amd.parse_args(["nart", path, "out"] + flags))[0]
    for sub, extra, guides in (("dc", [], None), ("dcl", ["--depth-layers"], None),
                               ("dcf", ["--follow-specular", "8"], nart_amd.GuideParams.defaults(max_follow=8))):
        d = tmp_path / sub
        d.mkdir()
        _run([path, str(d / "out")] + flags + ["--depth-cuts", "1,2", "--denoise-parts"] + extra)
        names = ["out.denoised.exr", "out.depth.01.exr", "out.depth.02.exr", "out.exr"]
        names += ["out.layer.%02d.denoised.exr" % k for k in range(3)]
        if "--depth-layers" in extra:
            names += ["out.layer.%02d.exr" % k for k in range(3)]
        assert sorted(os.listdir(d)) == sorted(names), sub
        api = glass_renderer.render_denoised_depth_layers(p, (1, 2), guides=guides, with_layers=True, with_beauty=True)
        want = {"out.exr": api["beauty"], "out.denoised.exr": api["sum"]}
        for k in range(3):
            want["out.layer.%02d.denoised.exr" % k] = api["denoised"][k]
            if "--depth-layers" in extra:
                want["out.layer.%02d.exr" % k] = api["layers"][k]
        for name, img in want.items():
            halves, _hdr = exr_py.read_rgba_halves(str(d / name))
            assert np.array_equal(halves, _halves(p, img)), (sub, name)
    # refused: the flag alone, and what was refused before it existed, with the messages it had
    out = str(tmp_path / "x")
    for extra, message in ((["--denoise-parts"], "--denoise-parts denoises the light groups or the depth layers"),
                           (["--light-groups", "each", "--denoise"], "--light-groups is not offered together with"),
                           (["--depth-cuts", "1,2", "--denoise"], "--depth-cuts is not offered together with"),
                           (["--light-groups", "each", "--denoise", "--denoise-parts"], "--light-groups is not offered"),
                           (["--depth-cuts", "1,2", "--aovs", "--denoise-parts"], "--depth-cuts is not offered together with"),
                           (["--depth-cuts", "1,2", "--follow-specular"], "--follow-specular selects the guides")):
        bad = _run([glass_scene.path, out] + flags + extra, ok=False)
        assert bad.returncode != 0 and bad.stderr.startswith("Error: ") and message in bad.stderr, (extra, bad.stderr)
        assert "Rendering" not in bad.stdout and not os.path.exists(out + ".exr")


# ---------------------------------------------------------------- 8. quality
def test_quality_cornell(gpu, cornell_scene):
    """Cornell 128 x 128: 4 spp noisy, denoised, and the sum of the separately denoised direct and indirect
    layers (cuts {1}) against the same renderer at 512 spp; relMSE and coverage mask as
    tests/test_gpu_denoise.py test_quality_cornell.  The values are recorded in DESIGN.md ("Denoised parts",
    D); the one assertion is that the parts' sum beats the noisy image."""
    r = nart_amd.HipRenderer(cornell_scene)
    p4, p512 = _params(cornell_scene, 128, 128, 4), _params(cornell_scene, 128, 128, 512)
    ref = r.render_aovs(p512, normal=False)
    whole = r.render_denoised(p4)
    parts = r.render_denoised_depth_layers(p4, (1,))
    r.close()
    mask = nart_amd.finalize(p512, ref["albedo"])[..., 3] >= 0.999
    x_ref = nart_amd.finalize(p512, ref["beauty"])[..., :3].astype(np.float64)

    def rel_mse(img):
        x = nart_amd.finalize(p4, img)[..., :3].astype(np.float64)
        return float((((x - x_ref) ** 2) / (x_ref ** 2 + 0.01))[mask].mean())

    noisy, den, summed = rel_mse(whole["beauty"]), rel_mse(whole["denoised"]), rel_mse(parts["sum"])
    print("cornell 128x128 4 spp: mask keeps %.3f, relMSE noisy %.5f denoised %.5f direct+indirect %.5f (ratios %.3f %.3f)" % (
        mask.mean(), noisy, den, summed, den / noisy, summed / noisy))
    assert mask.mean() >= 0.90, mask.mean()
    assert summed < noisy, (summed, noisy)
