"""Depth cuts on the device (nart_hip_render_depth_cuts, nart_hip_depth_layers,
nart_hip_render_depth_cut_samples, `nart --depth-cuts`; include/nart_hip.h, "Depth cuts") against the
unchanged oracle at `bounces = d`, which agrees with cut d where the RNG start states agree: the whole
frame at 1 spp, the first sample of every pixel at any spp (tests/test_depth_cuts_definition.py checks the
yardstick frames on the CPU).  Tolerance 0 throughout.  Every render also returns the beauty, which must
have render()'s bits, and every cut image carries the beauty's alpha and filter weight sum.  Oracle
frames are rendered once per session and shared (lightgroup_py.Frames, keyed on p.bounces)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import depthcut_py as dc
import exr_py
import nart_amd
import oracle

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NART = os.path.join(REPO, "nart_amd", "bin", "nart")
E_INVALID, E_UNSUPPORTED = -1, -6
PLAIN = {"priority", "spec_pairs", "half_waves", "lean", "specialized"}  # what a depth-cut frame never runs


@pytest.fixture(scope="module")
def frames(gpu, tmp_path_factory):
    return dc.lg.shared_frames(tmp_path_factory)


def _check(r, frames, name, p, cuts, st=None):
    """render_depth_cuts(p, cuts) on r at 1 spp: the beauty has render()'s bits, cut j the bits of the
    oracle's frame with bounces = cuts[j], alpha and filter weight sum the beauty's."""
    assert p.spp == 1
    out = r.render_depth_cuts(p, cuts, with_beauty=True, stats=st)
    assert out["cuts"].shape[0] == len(cuts)
    plain = r.render(p)
    assert dc.bits_equal(out["beauty"], plain), dc.report(out["beauty"], plain)
    assert dc.bits_equal(plain, frames.oracle(name, p))
    for j, d in enumerate(cuts):
        want = frames.oracle(name, dc.with_bounces(p, d))
        assert dc.bits_equal(out["cuts"][j], want), (name, d, dc.report(out["cuts"][j], want))
        assert dc.bits_equal(out["cuts"][j][..., 3:], plain[..., 3:]), d  # alpha, filter weight sum: the beauty's
    assert out["splat_ms"] > 0
    return out, plain


def test_materials_direct(frames):
    """50x37, bucket 16, filter width 1.5: ragged buckets, one lane per pixel."""
    name, p, cuts = dc.frame_params(frames, "materials_direct")
    r = nart_amd.HipRenderer(frames.scene(name))
    st = nart_amd.RenderStats()
    _check(r, frames, name, p, cuts, st)
    names = set(st.schedule_names())
    assert not names & (PLAIN | {"probe_queue", "wave_groups"}), names
    assert r.scene_features()[1] == nart_amd.api.FT_ALL  # the generic build


def test_materials_pixel_queue(frames):
    """432x300 (1.0 rounds of resident waves; the schedule is chosen from the pixel count, so 1 spp runs
    what the light groups' 4 spp frame of this size runs): the probe-ordered pixel queue, without
    priority lanes or speculative pairs."""
    name, p, cuts = dc.frame_params(frames, "materials_queue")
    r = nart_amd.HipRenderer(frames.scene(name))
    st = nart_amd.RenderStats()
    _check(r, frames, name, p, cuts, st)
    names = set(st.schedule_names())
    assert "probe_queue" in names and not names & PLAIN, names
    assert r.scene_features()[1] == nart_amd.api.FT_ALL


def test_materials_wave_groups(frames):
    """1056x750 (6.1 rounds): the persistent grid's waves take 64-slot groups, a lane several pixels in turn."""
    name, p, cuts = dc.frame_params(frames, "materials_groups")
    r = nart_amd.HipRenderer(frames.scene(name))
    st = nart_amd.RenderStats()
    _check(r, frames, name, p, cuts, st)
    names = set(st.schedule_names())
    assert "wave_groups" in names and not names & PLAIN, names
    assert r.scene_features()[1] == nart_amd.api.FT_ALL


@pytest.mark.parametrize("key", ["veach", "ring"])
def test_reference_scenes(frames, key):
    name, p, cuts = dc.frame_params(frames, key)
    r = nart_amd.HipRenderer(frames.scene(name))
    _check(r, frames, name, p, cuts)
    assert r.scene_features()[1] == nart_amd.api.FT_ALL


@pytest.mark.parametrize("key", ["env", "envc"])
def test_environment(frames, key):
    """The ENV build, and the camera ray that escapes to a light at bounce 0: a sky pixel holds Le in
    every cut."""
    name, p, cuts = dc.frame_params(frames, key)
    r = nart_amd.HipRenderer(frames.scene(name))
    out, plain = _check(r, frames, name, p, cuts)
    assert r.scene_features()[1] == nart_amd.api.FT_ALL
    coverage = r.render_aovs(p, albedo=True, normal=False, beauty=False)["albedo"][..., 3]
    g = nart_amd.session_geometry(p)
    fb = g.filter_bounds
    crop = (slice(fb, fb + p.image_height), slice(fb, fb + p.image_width))
    sky = (coverage[crop] == 0) & (plain[crop][..., :3].sum(-1) > 0)
    assert sky.any()
    for j in range(len(cuts)):
        assert dc.bits_equal(out["cuts"][j][crop][sky], plain[crop][sky]), cuts[j]


def test_nested_glass_deep_lists(frames):
    """bounces 16: the EXT build (dielectric lists beyond the registers) and stepped-through interfaces,
    bounces without a term."""
    name, p, cuts = dc.frame_params(frames, "nested")
    r = nart_amd.HipRenderer(frames.scene(name))
    assert p.bounces == 16 and cuts[-1] == 16
    out, _plain = _check(r, frames, name, p, cuts)
    assert dc.bits_equal(out["cuts"][-1], out["beauty"])
    assert r.scene_features()[1] == nart_amd.api.FT_ALL


def _materials8(frames):
    return frames.params("materials", 50, 37, 8, **dc.MATERIALS_DIRECT)


def test_eight_spp_the_deepest_cut_is_the_beauty(frames):
    r = nart_amd.HipRenderer(frames.scene("materials"))
    p = _materials8(frames)
    assert p.bounces == 12
    plain = r.render(p)
    assert dc.bits_equal(plain, frames.oracle("materials", p))
    out = r.render_depth_cuts(p, [12], with_beauty=True)
    assert dc.bits_equal(out["beauty"], plain)
    assert dc.bits_equal(out["cuts"][0], plain), dc.report(out["cuts"][0], plain)
    eight = r.render_depth_cuts(p, list(range(1, 9)), with_beauty=True)
    assert eight["cuts"].shape[0] == 8 and dc.bits_equal(eight["beauty"], plain)
    for j in range(8):
        assert dc.bits_equal(eight["cuts"][j][..., 3:], plain[..., 3:]), j
        assert np.isfinite(eight["cuts"][j]).all()
    assert not dc.bits_equal(eight["cuts"][0], eight["cuts"][1])
    two = r.render_depth_cuts(p, [2], with_beauty=True)
    assert dc.bits_equal(two["beauty"], plain)
    assert dc.bits_equal(two["cuts"][0], eight["cuts"][1]), dc.report(two["cuts"][0], eight["cuts"][1])


def test_per_sample_records(frames):
    """An 8x8 block of materials at 8 spp: sample 0 of every pixel starts from the RNG state a render with
    bounces = d starts from; the deepest cut is the beauty sample for sample; the records never
    decrease with the depth (the terms are non-negative, float addition is monotone)."""
    r = nart_amd.HipRenderer(frames.scene("materials"))
    p = _materials8(frames)
    x0, y0, cuts = 20, 14, [1, 2, 12]
    rec = r.render_depth_cut_samples(p, cuts, x0, y0, 8, 8)
    assert rec.shape == (3, 8, 8, 8, 4)
    orc = oracle.Oracle(frames.scene("materials"))
    beauty = orc.render_samples(p, x0, y0, 8, 8)
    assert dc.bits_equal(r.render_samples(p, x0, y0, 8, 8), beauty)
    for j, d in enumerate(cuts):
        want = orc.render_samples(dc.with_bounces(p, d), x0, y0, 8, 8)
        assert dc.bits_equal(rec[j][..., 0, :], want[..., 0, :]), (d, dc.report(rec[j][..., 0, :], want[..., 0, :]))
        assert dc.bits_equal(rec[j][..., 3], beauty[..., 3]), d  # alpha of every record: the beauty sample's
    assert dc.bits_equal(rec[2], beauty), dc.report(rec[2], beauty)
    assert np.isfinite(rec).all()
    for j in range(2):
        assert (rec[j + 1][..., :3] >= rec[j][..., :3]).all(), j
    assert rec[0][..., :3].any()  # the direct records are not all zero
    assert not dc.bits_equal(rec[0], rec[1]) and not dc.bits_equal(rec[1], rec[2])


def test_several_batches(frames, monkeypatch):
    """NART_BATCH_BYTES so small that the 50x37 frame takes several batches: the record arrays are sized
    and strided per batch."""
    name, p, cuts = dc.frame_params(frames, "materials_direct")
    r = nart_amd.HipRenderer(frames.scene(name))
    whole = r.render_depth_cuts(p, cuts)["cuts"]
    p8 = _materials8(frames)
    whole8 = r.render_depth_cuts(p8, cuts, with_beauty=True)
    monkeypatch.setenv("NART_BATCH_BYTES", str(300000))
    st = nart_amd.RenderStats()
    out, _plain = _check(r, frames, name, p, cuts, st)
    assert dc.bits_equal(out["cuts"], whole)
    st = nart_amd.RenderStats()
    out8 = r.render_depth_cuts(p8, cuts, with_beauty=True, stats=st)
    assert st.kernel_launches >= 3
    assert dc.bits_equal(out8["cuts"], whole8["cuts"]) and dc.bits_equal(out8["beauty"], whole8["beauty"])


def test_two_devices(frames):
    name, p, cuts = dc.frame_params(frames, "materials_direct")
    r = nart_amd.HipRenderer(frames.scene(name), devices=[0, 0])
    _check(r, frames, name, p, cuts)
    p8 = _materials8(frames)
    rec = r.render_depth_cut_samples(p8, cuts, 20, 14, 2, 2)  # (runs on the first device)
    one = nart_amd.HipRenderer(frames.scene(name)).render_depth_cut_samples(p8, cuts, 20, 14, 2, 2)
    assert dc.bits_equal(rec, one)


def _raises(code, call):
    with pytest.raises(nart_amd.NartError) as e:
        call()
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


def test_errors_leave_the_context_usable(frames, volume_scenes):
    r = nart_amd.HipRenderer(frames.scene("materials"))
    p = _materials8(frames)
    want = frames.oracle("materials", p)

    def usable():
        assert dc.bits_equal(r.render(p), want)

    # K outside 1..8, not strictly ascending, a cut of 0, a cut above p.bounces, null cuts
    for cuts, kw in (([], {}), (list(range(1, 10)), {}), ([1, 2], {"n_cuts": 0}), ([2, 2], {}), ([3, 1], {}), ([0, 1], {}),
                     ([0], {}), ([1, 13], {}), ([13], {}), (None, {"n_cuts": 2})):
        _raises(E_INVALID, lambda: r.render_depth_cuts(p, cuts, **kw))
        _raises(E_INVALID, lambda: r.render_depth_cut_samples(p, cuts, 0, 0, 2, 2, **kw))
        usable()
    # null images
    c = (ctypes.c_uint32 * 2)(1, 2)
    assert r._lib.nart_hip_render_depth_cuts(r._ctx, ctypes.byref(p), c, 2, None, None, None) == E_INVALID
    assert r._lib.nart_hip_render_depth_cut_samples(r._ctx, ctypes.byref(p), c, 2, 0, 0, 2, 2, None) == E_INVALID
    g = nart_amd.session_geometry(p)
    img = np.zeros((3, g.total_height, g.total_width, 5), np.float32)
    a = img.ctypes.data
    assert r._lib.nart_hip_depth_layers(r._ctx, ctypes.byref(p), 2, None, a, a) == E_INVALID
    assert r._lib.nart_hip_depth_layers(r._ctx, ctypes.byref(p), 2, a, None, a) == E_INVALID
    assert r._lib.nart_hip_depth_layers(r._ctx, ctypes.byref(p), 2, a, a, None) == E_INVALID
    assert r._lib.nart_hip_depth_layers(r._ctx, ctypes.byref(p), 0, a, a, a) == E_INVALID
    assert r._lib.nart_hip_depth_layers(r._ctx, ctypes.byref(p), 9, a, a, a) == E_INVALID
    # a bad rect
    _raises(E_INVALID, lambda: r.render_depth_cut_samples(p, [1, 2], 0, 0, 0, 2))
    _raises(E_INVALID, lambda: r.render_depth_cut_samples(p, [1, 2], g.total_width - 1, 0, 2, 2))
    usable()
    # variant 3 runs k_render, which has no depth-cut build
    r.set_variant(3)
    assert "depth cuts" in _raises(E_UNSUPPORTED, lambda: r.render_depth_cuts(p, [1, 2]))
    assert "depth cuts" in _raises(E_UNSUPPORTED, lambda: r.render_depth_cut_samples(p, [1, 2], 0, 0, 2, 2))
    usable()
    r.set_variant(0)
    out = r.render_depth_cuts(p, [12])
    assert dc.bits_equal(out["cuts"][0], want)
    # the volume integrator has no depth-cut build
    vs = volume_scenes["c5"]
    rv = nart_amd.HipRenderer(vs)
    pv = nart_amd.load_sessions(vs.path)[0]
    pv.image_width, pv.image_height, pv.spp = 32, 24, 2
    assert pv.integrator == 1 and pv.bounces >= 1
    before = rv.render(pv)
    assert "depth cuts" in _raises(E_UNSUPPORTED, lambda: rv.render_depth_cuts(pv, [1]))
    assert "depth cuts" in _raises(E_UNSUPPORTED, lambda: rv.render_depth_cut_samples(pv, [1], 0, 0, 2, 2))
    assert dc.bits_equal(rv.render(pv), before)


def _same_values(a, b):
    """Bit for bit where neither is NaN, NaN in the same places (a NaN's payload and sign are the
    processor's: x86 makes inf - inf a negative quiet NaN, the device a positive one)."""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(dc.bits(a)[~na], dc.bits(b)[~nb])


def test_depth_layers_on_the_device(frames):
    r = nart_amd.HipRenderer(frames.scene("materials"))
    p = _materials8(frames)
    g = nart_amd.session_geometry(p)
    rng = np.random.RandomState(7)
    for K in (1, 3, 8):
        I = rng.standard_normal((K + 1, g.total_height, g.total_width, 5)).astype(np.float32)
        special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, 1e-45, -3e-45, 3e38], np.float32)
        where = rng.rand(*I.shape) < 0.08
        I[where] = special[rng.randint(0, len(special), int(where.sum()))]
        got, want = r.depth_layers(p, I[:K], I[K]), dc.layers(I[:K], I[K])
        assert got.shape == (K + 1, g.total_height, g.total_width, 5)
        assert _same_values(got, want), (K, dc.report(got, want))
        assert np.isnan(got).any() and np.isinf(got).any()
        finite = np.nan_to_num(I, nan=0.5, posinf=2.0, neginf=-2.0)  # without NaN: every bit
        assert dc.bits_equal(r.depth_layers(p, finite[:K], finite[K]), dc.layers(finite[:K], finite[K]))
        assert r.depth_cut_timings()["layers_ms"] > 0
    # rendered cuts: every bit; layer_0 is the first cut, the layers meet the beauty within layers' bound
    out = r.render_depth_cuts(p, [1, 2, 5], with_beauty=True)
    L = r.depth_layers(p, out["cuts"], out["beauty"])
    assert dc.bits_equal(L, dc.layers(out["cuts"], out["beauty"]))
    assert dc.bits_equal(L[0][..., :3], out["cuts"][0][..., :3])
    for j in range(4):
        assert dc.bits_equal(L[j][..., 3:], out["beauty"][..., 3:])
    err = np.abs(dc.layers_sum(L).astype(np.float64) - out["beauty"][..., :3])
    assert (err <= dc.layers_bound(out["cuts"], out["beauty"])).all()
    # direct and indirect
    two = r.depth_layers(p, out["cuts"][:1], out["beauty"])
    assert two.shape[0] == 2 and dc.bits_equal(two, dc.layers(out["cuts"][:1], out["beauty"]))


def _halves(p, image):
    with np.errstate(over="ignore"):
        return nart_amd.finalize(p, image).astype(np.float16).view(np.uint16)


def test_cli(frames, tmp_path):
    path = frames.base["materials"]
    out = str(tmp_path / "out")
    flags = ["-w", "50", "-h", "37", "-s", "1"]
    run = subprocess.run([NART, path, out] + flags + ["--depth-cuts", "1,2,12", "--depth-layers"],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    p = nart_amd.load_sessions(path, nart_amd.parse_args(["nart", path, out] + flags))[0]
    assert p.spp == 1 and p.bounces == 12
    beauty = frames.oracle("materials", p)
    images = [frames.oracle("materials", dc.with_bounces(p, d)) for d in (1, 2, 12)]
    layers = dc.layers(np.stack(images), beauty)
    wanted = [("", beauty), (".depth.01", images[0]), (".depth.02", images[1]), (".depth.12", images[2])]
    wanted += [(".layer.%02d" % j, layers[j]) for j in range(4)]
    for name, image in wanted:
        assert ("Writing to %s%s.exr..." % (out, name)) in run.stdout
        halves, _hdr = exr_py.read_rgba_halves(out + name + ".exr")
        assert np.array_equal(halves, _halves(p, image)), name
    # without --depth-layers: the cuts only
    run = subprocess.run([NART, path, out + "b"] + flags + ["--depth-cuts", "4"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and os.path.exists(out + "b.depth.04.exr") and not os.path.exists(out + "b.layer.00.exr")
    halves, _hdr = exr_py.read_rgba_halves(out + "b.depth.04.exr")
    assert np.array_equal(halves, _halves(p, frames.oracle("materials", dc.with_bounces(p, 4))))
    # refused combinations and malformed, unsorted or out-of-range lists: a message, a non-zero exit, nothing rendered
    cut = ["--depth-cuts", "1,2"]
    for extra in (cut + ["--light-groups", "each"], cut + ["--adaptive", "0.1"], cut + ["--robust"], cut + ["--mattes"],
                  cut + ["--aovs"], cut + ["--denoise"], cut + ["--aovs", "--follow-specular"], ["--depth-layers"],
                  ["--depth-cuts"], ["--depth-cuts", "1,x"], ["--depth-cuts", ""], ["--depth-cuts", "1,,2"],
                  ["--depth-cuts", "2,1"], ["--depth-cuts", "2,2"], ["--depth-cuts", "0,1"], ["--depth-cuts", "-1"],
                  ["--depth-cuts", "1,13"], ["--depth-cuts", "1,2,3,4,5,6,7,8,9"]):
        bad = subprocess.run([NART, path, out + "x"] + flags + extra, capture_output=True, text=True, timeout=300)
        assert bad.returncode != 0 and bad.stderr.startswith("Error: "), (extra, bad.stdout, bad.stderr)
        assert "Rendering" not in bad.stdout and not os.path.exists(out + "x.exr")
