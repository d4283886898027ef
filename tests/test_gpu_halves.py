"""Half buffers (nart_hip_render_halves, `nart --halves`) on the device against their numpy restatement
(tests/halves_py.py, validated on the CPU by tests/test_halves_restatement.py) fed with the device's own
per-sample Li_alpha: bit for bit, tolerance 0, in both sample orders the splat kernels consume."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import exr_py
import halves_py as hp
import nart_amd
from test_aov_restatement import total_frame_uv

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


# ---------------------------------------------------------------- 1. the halves, bit for bit
_restated = {}


def _restated_halves(scene, key, size, spp, bucket):
    """The half images restated over the device's own per-sample Li_alpha of the whole total frame,
    computed once per configuration (the splat mode does not enter) and shared read-only."""
    k = (key, size, spp, bucket)
    if k not in _restated:
        p = _params(scene, size[0], size[1], spp, bucket_size=bucket)
        g = nart_amd.session_geometry(p)
        r = nart_amd.HipRenderer(scene)
        L = np.ascontiguousarray(r.render_samples(p, 0, 0, g.total_width, g.total_height))
        r.close()
        want = hp.restate_halves(p, total_frame_uv(p), L)
        want.setflags(write=False)
        _restated[k] = (p, want)
    return _restated[k]


# mode 4: the skew kernels, which stream one pixel's samples (pixel-major records); mode 5: the rows
# kernels on sample-major records.  Both need power-of-two buckets, which 16 and 32 are
CASES = [(size, spp, bucket, mode) for size in ((37, 29), (70, 3)) for spp in (2, 5, 16) for bucket in (16, 32)
         for mode in (4, 5)]


def _check_call(r, p, want, st=None, **kw):
    out = r.render_halves(p, stats=st, **kw)
    assert out["halves"].shape == want.shape
    for h in (0, 1):
        assert _bits_equal(out["halves"][h], want[h]), (h, _report(out["halves"][h], want[h]))
    plain = r.render(p)
    assert _bits_equal(out["beauty"], plain)
    for h in (0, 1):
        assert _bits_equal(out["halves"][h][..., 4], plain[..., 4]), h
    assert out["halves_ms"] > 0
    return out


@pytest.mark.parametrize("size,spp,bucket,splat_mode", CASES, ids=["%dx%d-%dspp-b%d-mode%d" % (c[0] + c[1:]) for c in CASES])
def test_halves_bit_for_bit(gpu, glass_scene, size, spp, bucket, splat_mode):
    """Odd sizes over several buckets and one row of buckets; 2, 5 and 16 spp: one sample per half, an
    odd count (three samples against two) and the splat kernels' 4-sample unrolling; both sample orders."""
    p, want = _restated_halves(glass_scene, "glass", size, spp, bucket)
    assert want[0][..., :3].max() > 0 and want[1][..., :3].max() > 0
    r = nart_amd.HipRenderer(glass_scene, splat_mode=splat_mode)
    st = nart_amd.RenderStats()
    _check_call(r, p, want, st)
    names = st.schedule_names()
    assert ("splat_skew" in names) == (splat_mode == 4) and ("splat_rows" in names) == (splat_mode == 5), names
    r.close()


def test_halves_default_splat_and_one_sample(gpu, glass_scene):
    """The default splat choice; and spp 1, where half 0 holds the beauty's rgb and half 1 nothing."""
    p, want = _restated_halves(glass_scene, "glass", (37, 29), 5, 16)
    r = nart_amd.HipRenderer(glass_scene)
    _check_call(r, p, want)
    p1 = _params(glass_scene, 37, 29, 1, bucket_size=16)
    out = r.render_halves(p1)
    assert _bits_equal(out["halves"][0][..., :3], out["beauty"][..., :3])
    assert _bits_equal(out["halves"][0][..., 3], out["beauty"][..., 4])
    assert not _bits(out["halves"][1][..., :4]).any() and _bits_equal(out["halves"][1][..., 4], out["beauty"][..., 4])
    r.close()


# ---------------------------------------------------------------- 2. AOVs, guides, batches, volume, two ranks
@pytest.fixture(scope="module")
def glass_renderer(gpu, glass_scene):
    r = nart_amd.HipRenderer(glass_scene)
    yield r
    r.close()


def test_halves_with_aovs_and_guides(glass_scene, glass_renderer):
    """The AOVs and the followed guides of the same call have the bits their own entry points give, one
    image or both (both guides: the normal records take the halves' record buffer after the halves'
    pass), and the halves do not change."""
    r = glass_renderer
    p, want = _restated_halves(glass_scene, "glass", (37, 29), 5, 16)
    aovs = r.render_aovs(p)
    out = _check_call(r, p, want, albedo=True, normal=True)
    assert _bits_equal(out["albedo"], aovs["albedo"]) and _bits_equal(out["normal"], aovs["normal"])
    gp = nart_amd.GuideParams.defaults()
    guides = r.render_guides(p, gp)
    assert not _bits_equal(guides["albedo"], aovs["albedo"])  # the glass sphere is followed
    out = _check_call(r, p, want, albedo=True, normal=True, guides=gp)
    assert _bits_equal(out["albedo"], guides["albedo"]) and _bits_equal(out["normal"], guides["normal"])
    out = _check_call(r, p, want, normal=True, guides=gp)
    assert set(out) == {"beauty", "halves", "normal", "halves_ms"} and _bits_equal(out["normal"], guides["normal"])


def test_halves_batches(gpu, glass_scene, monkeypatch):
    """NART_BATCH_BYTES=1 leaves 256 slots (tests/test_gpu_moment.py test_moment_batches): several
    batches, each with bucket bases of its own for the sample index, in both sample orders."""
    p, want = _restated_halves(glass_scene, "glass", (37, 29), 5, 16)
    monkeypatch.setenv("NART_BATCH_BYTES", "1")
    for mode in (4, 5):
        r = nart_amd.HipRenderer(glass_scene, splat_mode=mode)
        st = nart_amd.RenderStats()
        _check_call(r, p, want, st)
        r.close()
        assert st.kernel_launches > 1


def test_halves_volume_session(gpu, volume_scenes):
    vol = volume_scenes["emissive"]
    p, want = _restated_halves(vol, "vol", (24, 20), 5, 16)
    assert want[..., :3].max() > 0
    r = nart_amd.HipRenderer(vol)
    _check_call(r, p, want)
    for kw in (dict(albedo=True), dict(normal=True, guides=nart_amd.GuideParams.defaults())):
        with pytest.raises(nart_amd.NartError) as e:
            r.render_halves(p, **kw)
        assert e.value.code == -6 and "volume" in str(e.value)
    _check_call(r, p, want)
    r.close()


def test_two_rank_rehearsal(gpu, glass_scene, glass_renderer):
    p = _params(glass_scene, 64, 48, 4)
    gp = nart_amd.GuideParams.defaults()
    single = glass_renderer.render_halves(p, albedo=True, normal=True, guides=gp)
    m = nart_amd.HipRenderer(glass_scene, devices=[0, 0])
    assert m.devices() == (2, False)
    got = m.render_halves(p, albedo=True, normal=True, guides=gp)
    for name in ("beauty", "halves", "albedo", "normal"):
        assert _bits_equal(got[name], single[name]), (name, _report(got[name], single[name]))
    assert got["halves_ms"] > 0
    assert _bits_equal(m.render(p), glass_renderer.render(p))
    m.close()


# ---------------------------------------------------------------- 3. errors, and the other entry points' bits
def test_halves_errors_leave_the_context_usable(gpu, glass_scene, glass_renderer):
    """What the entry point can be asked and refuses; the combinations it cannot express (the moment
    image, adaptive sampling, the cascade, the mattes, light groups, depth cuts, the cost image) are
    plan_frame's rules, which tests/test_frame_plan_halves.py covers with their messages."""
    r = glass_renderer
    p = _params(glass_scene, 32, 24, 2)
    g = nart_amd.session_geometry(p)
    good = r.render(p)
    ok = r.render_halves(p)
    lib = nart_amd.hip_lib()
    img = [np.zeros((g.total_height, g.total_width, 5), f32) for _ in range(5)]
    P, d = ctypes.byref(p), [a.ctypes.data for a in img]
    call = lambda *a: lib.nart_hip_render_halves(r._ctx, *a)
    assert call(P, 0, None, None, None, None, d[3], d[4], None, None) == -1   # no beauty
    assert "half" in lib.nart_hip_last_error(r._ctx).decode()
    assert call(P, 0, None, d[0], None, None, None, d[4], None, None) == -1   # no half 0
    assert call(P, 0, None, d[0], None, None, d[3], None, None, None) == -1   # no half 1
    assert call(None, 0, None, d[0], None, None, d[3], d[4], None, None) == -1  # no params
    assert call(P, 4, None, d[0], d[1], d[2], d[3], d[4], None, None) == -1   # an unknown AOV bit
    assert call(P, 1, None, d[0], None, d[2], d[3], d[4], None, None) == -1   # a bit without its buffer
    bad = nart_amd.GuideParams.defaults()
    bad.max_follow = 11
    assert call(P, 3, ctypes.byref(bad), d[0], d[1], d[2], d[3], d[4], None, None) == -1
    assert not any(a.any() for a in img)
    assert _bits_equal(r.render(p), good)
    again = r.render_halves(p)
    assert _bits_equal(again["halves"], ok["halves"]) and _bits_equal(again["beauty"], good)


def test_other_entry_points_keep_their_bits(gpu, glass_scene):
    """render, render_aovs(moment=True), render_guides and render_denoised give the same bits, launches
    and schedule before and after half-buffer calls on the same context."""
    p = _params(glass_scene, 48, 32, 4)
    r = nart_amd.HipRenderer(glass_scene)

    def snapshot():
        st = nart_amd.RenderStats()
        a = r.render(p, st)
        b = r.render_aovs(p, moment=True)
        c = r.render_guides(p)
        d = r.render_denoised(p)
        return {"render": a, "albedo": b["albedo"], "normal": b["normal"], "moment": b["moment"], "beauty": b["beauty"],
                "guide_albedo": c["albedo"], "guide_normal": c["normal"], "denoised": d["denoised"]}, \
            (st.kernel_launches, st.schedule)

    before, st_before = snapshot()
    r.render_halves(p)
    r.render_halves(p, albedo=True, normal=True, guides=nart_amd.GuideParams.defaults())
    after, st_after = snapshot()
    assert st_before == st_after
    for name in before:
        assert _bits_equal(before[name], after[name]), name
    r.close()


# ---------------------------------------------------------------- 4. CLI
def test_cli_halves(gpu, glass_scene, tmp_path):
    base = [NART, glass_scene.path]
    size = ["-w", "48", "-h", "32", "-s", "5"]
    h_dir, a_dir, bad_dir = tmp_path / "h", tmp_path / "a", tmp_path / "bad"
    for d in (h_dir, a_dir, bad_dir):
        d.mkdir()
    for d, extra in ((h_dir, ["--halves"]), (a_dir, ["--halves", "--aovs", "--follow-specular", "4"])):
        res = subprocess.run(base + [str(d / "out")] + size + extra, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    assert sorted(os.listdir(h_dir)) == ["out.exr", "out.half.0.exr", "out.half.1.exr"]
    assert sorted(os.listdir(a_dir)) == ["out.albedo.exr", "out.exr", "out.half.0.exr", "out.half.1.exr", "out.normal.exr"]
    p = nart_amd.parse_args(["nart", glass_scene.path, "out"] + size)
    p = nart_amd.load_sessions(glass_scene.path, p)[0]
    r = nart_amd.HipRenderer(glass_scene)
    gp = nart_amd.GuideParams.defaults()
    gp.max_follow = 4
    api = r.render_halves(p, albedo=True, normal=True, guides=gp)
    r.close()
    to_half = nart_amd.scene_lib().nart_float_to_half

    def halves_of(img):
        final = nart_amd.finalize(p, img)
        return np.array([to_half(ctypes.c_float(v)) for v in final.reshape(-1)], np.uint16).reshape(final.shape)

    files = {"out.exr": api["beauty"], "out.half.0.exr": api["halves"][0], "out.half.1.exr": api["halves"][1]}
    for d, names in ((h_dir, files), (a_dir, dict(files, **{"out.albedo.exr": api["albedo"], "out.normal.exr": api["normal"]}))):
        for name, img in names.items():
            halves, _hdr = exr_py.read_rgba_halves(str(d / name))
            assert halves.shape == (32, 48, 4) and np.array_equal(halves, halves_of(img)), (str(d), name)
    # not offered together with the stages that the halves' frame refuses
    for extra in (["--denoise"], ["--adaptive", "0.1"], ["--robust"], ["--mattes"], ["--light-groups", "each"],
                  ["--depth-cuts", "1"], ["--cost"], ["--light-groups", "each", "--denoise-parts"]):
        res = subprocess.run(base + [str(bad_dir / "out")] + size + ["--halves"] + extra, capture_output=True, text=True,
                             timeout=300)
        assert res.returncode != 0 and "--halves" in res.stderr and not res.stdout, extra
    assert os.listdir(bad_dir) == []
