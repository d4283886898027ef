"""Light groups on the device (nart_hip_render_light_groups, nart_hip_light_mix,
nart_hip_render_light_group_samples, `nart --light-groups`; include/nart_hip.h, "Light groups") against
the unchanged oracle on scene files whose other lights have intensity 0
(tests/test_light_groups_definition.py checks on the CPU that those frames form no 0 * inf): tolerance 0,
except the one sanity bound that says otherwise.  Every render also returns the beauty, which must have
render()'s bits.  Oracle frames are rendered once per session and shared (lightgroup_py.Frames)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import exr_py
import lightgroup_py as lg
import nart_amd
import oracle

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NART = os.path.join(REPO, "nart_amd", "bin", "nart")
E_INVALID, E_UNSUPPORTED = -1, -6
PLAIN = {"priority", "spec_pairs", "half_waves", "lean", "specialized"}  # what a group frame never runs


@pytest.fixture(scope="module")
def frames(gpu, tmp_path_factory):
    return lg.shared_frames(tmp_path_factory)


def _check(r, frames, name, p, groups, lit, st=None):
    """render_light_groups(p, groups) on r: the beauty has render()'s bits, group g the bits of the
    oracle's frame with only the lights lit[g] on."""
    out = r.render_light_groups(p, groups, with_beauty=True, stats=st)
    assert out["groups"].shape[0] == len(lit)
    plain = r.render(p)
    assert lg.bits_equal(out["beauty"], plain), lg.report(out["beauty"], plain)
    for g, on in enumerate(lit):
        want = frames.oracle(name, p, lit=on)
        assert lg.bits_equal(out["groups"][g], want), (name, g, lg.report(out["groups"][g], want))
        assert lg.bits_equal(out["groups"][g][..., 3:], plain[..., 3:]), g  # alpha, filter weight sum: the beauty's
    assert out["splat_ms"] > 0
    return out, plain


def test_materials_direct(frames):
    """50x37 at 8 spp, bucket 16, filter width 1.5: ragged buckets, one lane per pixel."""
    r = nart_amd.HipRenderer(frames.scene("materials"))
    p = frames.params("materials", 50, 37, 8, bucket_size=16, filter_width=1.5)
    st = nart_amd.RenderStats()
    _check(r, frames, "materials", p, [0, 1], [[0], [1]], st)
    names = set(st.schedule_names())
    assert not names & (PLAIN | {"probe_queue", "wave_groups"}), names
    assert r.scene_features()[1] == nart_amd.api.FT_ALL  # the generic build


def test_materials_pixel_queue(frames):
    """432x300 at 4 spp (1.0 rounds of resident waves): the probe-ordered pixel queue, without priority
    lanes or speculative pairs."""
    r = nart_amd.HipRenderer(frames.scene("materials"))
    p = frames.params("materials", 432, 300, 4)
    st = nart_amd.RenderStats()
    _check(r, frames, "materials", p, [0, 1], [[0], [1]], st)
    names = set(st.schedule_names())
    assert "probe_queue" in names and not names & PLAIN, names


def test_materials_wave_groups(frames):
    """1056x750 at 1 spp (6.1 rounds): the persistent grid's waves take 64-slot groups."""
    r = nart_amd.HipRenderer(frames.scene("materials"))
    p = frames.params("materials", 1056, 750, 1)
    st = nart_amd.RenderStats()
    _check(r, frames, "materials", p, [0, 1], [[0], [1]], st)
    names = set(st.schedule_names())
    assert "wave_groups" in names and not names & PLAIN, names


def test_veach_merged_lights(frames):
    """Four lights, three groups: lights 1 and 2 share group 1."""
    r = nart_amd.HipRenderer(frames.scene("veach"))
    p = frames.params("veach", 48, 32, 8)
    _check(r, frames, "veach", p, [0, 1, 1, 2], [[0], [1, 2], [3]])


def test_ring_two_lights(frames):
    r = nart_amd.HipRenderer(frames.scene("ring"))
    _check(r, frames, "ring", frames.params("ring", 48, 32, 8), [1, 0], [[1], [0]])  # groups need not follow scene order


def test_one_group_holding_every_light_is_the_beauty(frames):
    r = nart_amd.HipRenderer(frames.scene("materials"))
    p = frames.params("materials", 50, 37, 8, bucket_size=16, filter_width=1.5)
    out = r.render_light_groups(p, [0, 0], with_beauty=True)
    assert lg.bits_equal(out["beauty"], r.render(p))
    assert lg.bits_equal(out["groups"][0], out["beauty"]), lg.report(out["groups"][0], out["beauty"])
    assert lg.bits_equal(out["beauty"], frames.oracle("materials", p))
    # a group without a light is black, with the beauty's alpha and weights
    three = r.render_light_groups(p, [2, 0], n_groups=3)["groups"]
    assert not three[1][..., :3].any() and lg.bits_equal(three[1][..., 3:], out["beauty"][..., 3:])


@pytest.mark.parametrize("name", ["env", "envc"])
def test_environment_and_disk(frames, name):
    """The ENV build, and the camera ray that escapes to a light: the environment's group has pixels
    where no surface was hit first."""
    r = nart_amd.HipRenderer(frames.scene(name))
    p = frames.params(name, 48, 32, 8)
    out, _plain = _check(r, frames, name, p, [0, 1], [[0], [1]])
    coverage = r.render_aovs(p, albedo=True, normal=False, beauty=False)["albedo"][..., 3]
    g = nart_amd.session_geometry(p)
    fb = g.filter_bounds
    crop = (slice(fb, fb + p.image_height), slice(fb, fb + p.image_width))
    sky = (coverage[crop] == 0) & (out["groups"][0][crop][..., :3].sum(-1) > 0)
    assert sky.any()
    assert not out["groups"][1][crop][sky].any(0)[:3].any()  # the disk's group sees nothing there


def test_nested_glass_deep_lists(frames):
    """bounces 16: the EXT build (dielectric lists beyond the registers)."""
    r = nart_amd.HipRenderer(frames.scene("nested"))
    p = frames.params("nested", 48, 36, 4)
    assert p.bounces == 16
    oracle.max_list_length(reset=True)
    _check(r, frames, "nested", p, [0, 1], [[0], [1]])
    if oracle.max_list_length() <= 10:  # (the frames were rendered by an earlier test: once more, for the count)
        oracle.Oracle(frames.scene("nested")).render(p)
    assert oracle.max_list_length() > 10


def test_per_sample_records(frames):
    """An 8x8 block of materials: every group's records against Oracle.render_samples of its
    zero-intensity scene, sample for sample (each group by itself: nothing is summed)."""
    r = nart_amd.HipRenderer(frames.scene("materials"))
    p = frames.params("materials", 50, 37, 8, bucket_size=16, filter_width=1.5)
    x0, y0 = 20, 14
    rec = r.render_light_group_samples(p, [0, 1], x0, y0, 8, 8)
    assert rec.shape == (2, 8, 8, 8, 4)
    beauty = r.render_samples(p, x0, y0, 8, 8)
    for g in (0, 1):
        want = oracle.Oracle(frames.scene("materials", [g])).render_samples(p, x0, y0, 8, 8)
        assert lg.bits_equal(rec[g], want), (g, lg.report(rec[g], want))
        assert lg.bits_equal(rec[g][..., 3], beauty[..., 3])
        assert rec[g][..., :3].any()
    assert lg.bits_equal(beauty, oracle.Oracle(frames.scene("materials")).render_samples(p, x0, y0, 8, 8))


def test_several_batches(frames, monkeypatch):
    """NART_BATCH_BYTES so small that the 50x37 frame (2,214 slots of 8 + 8 (28 + 32) bytes) takes several
    batches: the record arrays are sized and strided per batch."""
    r = nart_amd.HipRenderer(frames.scene("materials"))
    p = frames.params("materials", 50, 37, 8, bucket_size=16, filter_width=1.5)
    monkeypatch.setenv("NART_BATCH_BYTES", str(300000))
    st = nart_amd.RenderStats()
    _check(r, frames, "materials", p, [0, 1], [[0], [1]], st)
    assert st.kernel_launches >= 3


def test_two_devices(frames):
    r = nart_amd.HipRenderer(frames.scene("materials"), devices=[0, 0])
    p = frames.params("materials", 50, 37, 8, bucket_size=16, filter_width=1.5)
    _check(r, frames, "materials", p, [0, 1], [[0], [1]])
    rec = r.render_light_group_samples(p, [0, 1], 20, 14, 2, 2)  # (runs on the first device)
    one = nart_amd.HipRenderer(frames.scene("materials")).render_light_group_samples(p, [0, 1], 20, 14, 2, 2)
    assert lg.bits_equal(rec, one)


def _raises(code, call):
    with pytest.raises(nart_amd.NartError) as e:
        call()
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


def test_errors_leave_the_context_usable(frames, volume_scenes):
    r = nart_amd.HipRenderer(frames.scene("materials"))
    p = frames.params("materials", 50, 37, 8, bucket_size=16, filter_width=1.5)
    want = frames.oracle("materials", p)

    def usable():
        assert lg.bits_equal(r.render(p), want)

    for groups, kw in (([0], {}), ([0, 1, 1], {}), ([0, 2], {"n_groups": 2}), ([0, 0], {"n_groups": 0}),
                       ([0, 8], {}), ([0, 1], {"n_groups": 9}), (None, {"n_groups": 2})):
        _raises(E_INVALID, lambda: r.render_light_groups(p, groups, **kw))
        _raises(E_INVALID, lambda: r.render_light_group_samples(p, groups, 0, 0, 2, 2, **kw))
        usable()
    # a null image for the groups, a null gain table
    m = (ctypes.c_uint32 * 2)(0, 1)
    assert r._lib.nart_hip_render_light_groups(r._ctx, ctypes.byref(p), m, 2, 2, None, None, None) == E_INVALID
    g = nart_amd.session_geometry(p)
    img = np.zeros((2, g.total_height, g.total_width, 5), np.float32)
    assert r._lib.nart_hip_light_mix(r._ctx, ctypes.byref(p), 2, None, img.ctypes.data, img.ctypes.data) == E_INVALID
    _raises(E_INVALID, lambda: r.light_mix(p, img, [1.0, float("inf")]))
    _raises(E_INVALID, lambda: r.light_mix(p, img, [[1.0, 1.0, float("nan")], [1, 1, 1]]))
    _raises(E_INVALID, lambda: r.render_light_group_samples(p, [0, 1], 0, 0, 0, 2))
    _raises(E_INVALID, lambda: r.render_light_group_samples(p, [0, 1], g.total_width - 1, 0, 2, 2))
    usable()
    # variant 3 runs k_render, which has no light-group build
    r.set_variant(3)
    assert "light groups" in _raises(E_UNSUPPORTED, lambda: r.render_light_groups(p, [0, 1]))
    assert "light groups" in _raises(E_UNSUPPORTED, lambda: r.render_light_group_samples(p, [0, 1], 0, 0, 2, 2))
    usable()
    r.set_variant(0)
    out = r.render_light_groups(p, [0, 1])
    assert lg.bits_equal(out["groups"][0], frames.oracle("materials", p, lit=[0]))
    # the volume integrator has no light-group build
    vs = volume_scenes["c5"]
    rv = nart_amd.HipRenderer(vs)
    pv = nart_amd.load_sessions(vs.path)[0]
    pv.image_width, pv.image_height, pv.spp = 32, 24, 2
    assert pv.integrator == 1
    n = lg.n_lights(vs.path)
    before = rv.render(pv)
    assert "light groups" in _raises(E_UNSUPPORTED, lambda: rv.render_light_groups(pv, [0] * n))
    assert "light groups" in _raises(E_UNSUPPORTED, lambda: rv.render_light_group_samples(pv, [0] * n, 0, 0, 2, 2))
    assert lg.bits_equal(rv.render(pv), before)


def _same_values(a, b):
    """Bit for bit where neither is NaN, NaN in the same places (a NaN's payload and sign are the
    processor's: x86 makes 0 * inf a negative quiet NaN, the device a positive one)."""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(lg.bits(a)[~na], lg.bits(b)[~nb])


def test_light_mix_on_the_device(frames):
    r = nart_amd.HipRenderer(frames.scene("materials"))
    p = frames.params("materials", 50, 37, 8, bucket_size=16, filter_width=1.5)
    g = nart_amd.session_geometry(p)
    rng = np.random.RandomState(5)
    for G in (1, 3, 8):
        I = rng.standard_normal((G, g.total_height, g.total_width, 5)).astype(np.float32)
        special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, 1e-45, 3e38], np.float32)
        where = rng.rand(*I.shape) < 0.05
        I[where] = special[rng.randint(0, len(special), int(where.sum()))]
        gains = rng.uniform(-2, 2, (G, 3)).astype(np.float32)
        gains[0] = (0.0, 1.0, -0.0)
        got, want = r.light_mix(p, I, gains), lg.mix(I, gains)
        assert _same_values(got, want), (G, lg.report(got, want))
        assert np.isnan(got).any() and np.isinf(got).any()
        finite = np.nan_to_num(I, nan=0.5, posinf=2.0, neginf=-2.0)  # without NaN: every bit
        assert lg.bits_equal(r.light_mix(p, finite, gains), lg.mix(finite, gains))
        assert r.light_group_timings()["mix_ms"] > 0
    # the rendered groups with gains 1: the beauty within the bound of summing the same terms in two orders
    out = r.render_light_groups(p, [0, 1], with_beauty=True)
    mixed = r.light_mix(p, out["groups"], [1.0, 1.0])
    assert lg.bits_equal(mixed, lg.mix(out["groups"], [1.0, 1.0]))
    assert lg.bits_equal(mixed[..., 3:], out["beauty"][..., 3:])
    total = out["groups"][..., :3].astype(np.float64).sum(0)
    bound = lg.sum_bound(p.spp, p.filter_width, p.bounces, 2)
    assert (np.abs(mixed[..., :3] - out["beauty"][..., :3].astype(np.float64)) <= bound * total).all()
    # gains 1 and 0: a group switched off leaves the other one, bit for bit
    assert lg.bits_equal(r.light_mix(p, out["groups"], [0.0, 1.0])[..., :3], out["groups"][1][..., :3])


def _halves(p, image):
    with np.errstate(over="ignore"):
        return nart_amd.finalize(p, image).astype(np.float16).view(np.uint16)


def test_cli(frames, tmp_path):
    path = frames.base["materials"]
    out = str(tmp_path / "out")
    flags = ["-w", "50", "-h", "37", "-s", "4"]
    run = subprocess.run([NART, path, out] + flags + ["--light-groups", "each", "--light-gains", "1,0.5"],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    p = nart_amd.load_sessions(path, nart_amd.parse_args(["nart", path, out] + flags))[0]
    images = [frames.oracle("materials", p, lit=[l]) for l in (0, 1)]
    for name, image in (("", frames.oracle("materials", p)), (".light.00", images[0]), (".light.01", images[1]),
                        (".mix", lg.mix(np.stack(images), [1.0, 0.5]))):
        assert ("Writing to %s%s.exr..." % (out, name)) in run.stdout
        halves, _hdr = exr_py.read_rgba_halves(out + name + ".exr")
        assert np.array_equal(halves, _halves(p, image)), name
    # a list: both lights in one group gives the beauty
    run = subprocess.run([NART, path, out + "b"] + flags + ["--light-groups", "0,0"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and not os.path.exists(out + "b.mix.exr") and not os.path.exists(out + "b.light.01.exr")
    halves, _hdr = exr_py.read_rgba_halves(out + "b.light.00.exr")
    assert np.array_equal(halves, _halves(p, frames.oracle("materials", p)))
    # refused combinations and malformed values: a message, a non-zero exit, nothing rendered
    for extra in (["--light-groups", "each", "--adaptive", "0.1"], ["--light-groups", "each", "--robust"],
                  ["--light-groups", "each", "--mattes"], ["--light-groups", "each", "--aovs"],
                  ["--light-groups", "each", "--denoise"], ["--light-groups", "each", "--aovs", "--follow-specular"],
                  ["--light-gains", "1,1"], ["--light-groups", "0,8"], ["--light-groups", "0,x"], ["--light-groups"],
                  ["--light-groups", "0,1,1"], ["--light-groups", "each", "--light-gains", "1"],
                  ["--light-groups", "each", "--light-gains", "1,inf"]):
        bad = subprocess.run([NART, path, out + "x"] + flags + extra, capture_output=True, text=True, timeout=300)
        assert bad.returncode != 0 and bad.stderr.startswith("Error: "), (extra, bad.stdout, bad.stderr)
        assert "Rendering" not in bad.stdout and not os.path.exists(out + "x.exr")
    # `each` is refused above 8 lights
    many = lg.scene_with(path, str(tmp_path / "many.json"), extra_lights=[lg.DISK] * 7)
    bad = subprocess.run([NART, many, out + "m"] + flags + ["--light-groups", "each"], capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "9 lights" in bad.stderr
