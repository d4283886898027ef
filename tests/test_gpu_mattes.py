"""The first-hit ID mattes (nart_hip_render_mattes, nart_hip_matte_rank, nart_hip_matte_extract,
`nart --mattes`) on the device against their numpy restatement (tests/matte_py.py, validated on the
CPU by tests/test_matte_restatement.py): bit for bit, tolerance 0, except the one sanity bound that
says otherwise."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import exr_py
import matte_py as mp
import nart_amd
from nart_amd import scenes
from nart_amd.api import MATTE_MATERIAL, MATTE_MESH
from test_aov_restatement import total_frame_uv
from test_matte_restatement import BAD, MATERIALS_SIZE, MATERIALS_SPP

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NART = os.path.join(REPO, "nart_amd", "bin", "nart")
f32 = np.float32
SIZE = (24, 40)
CONFIGS = {"b16_fw2": dict(bucket_size=16, filter_width=2.0), "b12_fw1": dict(bucket_size=12, filter_width=1.0)}


def _params(scene, w, h, spp, **kw):
    p = nart_amd.load_sessions(scene.path)[0]
    p.image_width, p.image_height, p.spp = w, h, spp
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _mp(**kw):
    return nart_amd.MatteParams.defaults(**kw)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bits_equal(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(_bits(a), _bits(b))


def _report(a, b):
    ne = _bits(a) != _bits(b)
    idx = np.argwhere(ne)
    with np.errstate(all="ignore"):
        worst = float(np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64)))) if ne.any() else 0.0
    return "%d of %d floats differ, max abs diff %g, first at %s" % (int(ne.sum()), ne.size, worst,
                                                                     idx[0].tolist() if len(idx) else None)


_restated = {}


def _restated_planes(scene, key, p, kind):
    """(ids, planes, terms, ranks by R) restated over the device's own per-sample first hits of the whole
    total frame, computed once per frame and id kind and shared read-only."""
    k = (key, p.image_width, p.image_height, p.spp, p.bucket_size, p.filter_width, kind)
    if k not in _restated:
        g = nart_amd.session_geometry(p)
        r = nart_amd.HipRenderer(scene)
        _rec, tri = r.render_aov_samples(p, 0, 0, g.total_width, g.total_height)
        r.close()
        ids = mp.ids_of(scene, np.where(tri == mp.NO_HIT, -1, tri.astype(np.int64)), kind)
        n = nart_amd.matte_ids(scene, kind)
        planes, terms = mp.restate_planes(p, total_frame_uv(p), ids, n, with_terms=True)
        _restated[k] = {"ids": ids, "n": n, "planes": planes, "terms": terms, "ranks": {}}
    return _restated[k]


def _restated_ranks(entry, p, R):
    if R not in entry["ranks"]:
        g = nart_amd.session_geometry(p)
        entry["ranks"][R] = mp.rank(p.image_width, p.image_height, g.filter_bounds, entry["planes"], entry["n"], R)
    return entry["ranks"][R]


def _ran(st, splat_mode, cfg):
    """The splat kernel family the schedule bits report, against the one the mode selects: rows and
    skew need power-of-two buckets (bucket 12 runs the one-pixel-per-lane kernels in every mode)."""
    names = st.schedule_names()
    pow2 = cfg == "b16_fw2"
    return ("splat_rows" in names) == (pow2 and splat_mode == 5) and ("splat_skew" in names) == (pow2 and splat_mode == 4)


def _check_call(r, p, m, entry, st=None):
    """A call with the beauty and the planes against the restatement and render(); then the
    matte-only call."""
    out = r.render_mattes(p, m, with_beauty=True, with_planes=True, stats=st)
    want = entry["planes"]
    assert out["n_ids"] == entry["n"] and out["planes"].shape == want.shape
    for q in range(len(want)):
        assert _bits_equal(out["planes"][q], want[q]), (q, _report(out["planes"][q], want[q]))
    ranks = _restated_ranks(entry, p, m.ranks)
    assert out["ranks"].shape == ranks.shape == (m.ranks // 2,) + want.shape[1:]
    assert _bits_equal(out["ranks"], ranks), _report(out["ranks"], ranks)
    plain = r.render(p)
    assert _bits_equal(out["beauty"], plain)
    for q in range(len(want)):
        assert _bits_equal(out["planes"][q][..., 4], plain[..., 4]), q
    assert out["matte_ms"] > 0 and out["rank_ms"] > 0
    st_only = nart_amd.RenderStats()
    only = r.render_mattes(p, m, stats=st_only)
    assert set(only) == {"ranks", "n_ids", "matte_ms", "rank_ms"} and _bits_equal(only["ranks"], out["ranks"])
    assert st_only.kernel_launches == 0
    return out


# ---------------------------------------------------------------- 1. planes and ranks, bit for bit
CASES = [(cfg, spp, mode) for cfg in CONFIGS for spp in (2, 3, 5) for mode in (5, 4, 3, 1, 0)]


@pytest.mark.parametrize("cfg,spp,splat_mode", CASES, ids=["%s-%dspp-mode%d" % c for c in CASES])
def test_mattes_bit_for_bit(gpu, glass_scene, cfg, spp, splat_mode):
    """2, 3 and 5 spp reach the tails of the splat kernels' 4-sample unrolling; every splat family gives
    the restatement's plane bits over the device's own first hits; the ranks are the restated ranking
    of those planes; the beauty of the same call is render()'s; the matte-only call launches no path
    kernel."""
    p = _params(glass_scene, SIZE[0], SIZE[1], spp, **CONFIGS[cfg])
    entry = _restated_planes(glass_scene, "glass", p, MATTE_MESH)
    assert (entry["ids"] >= 0).any() and (entry["ids"] < 0).any()  # hits and misses
    assert entry["planes"][0][..., :4].max() > 0
    r = nart_amd.HipRenderer(glass_scene, splat_mode=splat_mode)
    st = nart_amd.RenderStats()
    _check_call(r, p, _mp(ranks=2 if spp == 3 else 6), entry, st)
    assert _ran(st, splat_mode, cfg), (splat_mode, st.schedule_names())
    r.close()


def test_mattes_default_parameters(gpu, glass_scene):
    p = _params(glass_scene, SIZE[0], SIZE[1], 2, **CONFIGS["b16_fw2"])
    entry = _restated_planes(glass_scene, "glass", p, MATTE_MESH)
    r = nart_amd.HipRenderer(glass_scene)
    out = r.render_mattes(p)  # params=None: mesh ids, six ranks
    assert out["ranks"].shape[0] == 3 and _bits_equal(out["ranks"], _restated_ranks(entry, p, 6))
    r.close()


# ---------------------------------------------------------------- 2. the materials scene: two planes
def _glass_mask(scene, kind):
    """The id set of the glass: the glass materials, or the meshes that wear them."""
    glass = [i for i, m in enumerate(scene.materials()) if m.type == nart_amd.api.MAT_GLASS]
    if kind == MATTE_MATERIAL:
        return sum(1 << i for i in glass)
    return sum(1 << i for i, mesh in enumerate(scene.meshes()) if int(mesh[2]) in glass)


@pytest.mark.parametrize("R", [2, 6])
@pytest.mark.parametrize("kind", [MATTE_MESH, MATTE_MATERIAL], ids=["mesh", "material"])
def test_materials_scene(gpu, materials_scene, kind, R):
    """Seven ids in two planes at the frame fixed on the CPU (test_first_hits_on_materials_scene): a
    pixel that three ids cover loses one at ranks = 2; the extraction of the glass equals the
    restatement; and, as a sanity bound (not bitwise), the sum of all ids' coverages agrees with the
    albedo AOV's coverage within (terms + N) * 2^-24 relative, terms the additions the pixel's sums
    received (matte_py.count_terms)."""
    p = _params(materials_scene, MATERIALS_SIZE[0], MATERIALS_SIZE[1], MATERIALS_SPP)
    g = nart_amd.session_geometry(p)
    fb, W, H = g.filter_bounds, p.image_width, p.image_height
    entry = _restated_planes(materials_scene, "materials", p, kind)
    assert entry["n"] == 7 and entry["planes"].shape[0] == 2
    crop = entry["planes"][:, fb:fb + H, fb:fb + W]
    positive = sum((crop[q][..., c] > 0).astype(int) for q in range(2) for c in range(4))
    assert positive.max() >= 3 and crop[1][..., :3].max() > 0
    r = nart_amd.HipRenderer(materials_scene)
    m = _mp(kind=kind, ranks=R)
    out = _check_call(r, p, m, entry)
    rk = out["ranks"][:, fb:fb + H, fb:fb + W]
    if R == 2:  # a truncated pixel: both ranks taken, a third id left out
        assert (rk[0][..., 2][positive >= 3] >= 0).all()
    else:
        assert (rk[1][..., 0][positive >= 3] >= 0).all() and (rk[2][..., 2] == -1).all()
    mask = _glass_mask(materials_scene, kind)
    assert mask == (1 << 5) | (1 << 6)
    got = r.matte_extract(p, out["ranks"], mask, m)
    want = mp.extract(W, H, fb, out["ranks"], mask)
    assert _bits_equal(got, want), _report(got, want)
    assert got[..., 0].max() > 0
    assert _bits_equal(r.matte_extract(p, out["ranks"], [5, 6], m), got)
    # the sanity bound, over the planes (every id, whatever R keeps)
    alb = r.render_aovs(p, normal=False, beauty=False)["albedo"][fb:fb + H, fb:fb + W]
    dev = out["planes"][:, fb:fb + H, fb:fb + W]
    with np.errstate(all="ignore"):
        c = (dev[..., :4] / dev[0][..., 4:5]).astype(f32)
        total = c.astype(np.float64).sum(axis=(0, -1))
        cover = (alb[..., 3] / alb[..., 4]).astype(f32).astype(np.float64)
    tol = (entry["terms"][fb:fb + H, fb:fb + W] + entry["n"]) * 2.0 ** -24
    err = np.abs(total - cover)
    print("coverage sum against the albedo coverage: max err / bound %.3f" % float((err / (tol * cover + 1e-300)).max()))
    assert (alb[..., 4] > 0).all() and (err <= tol * cover).all()
    r.close()


# ---------------------------------------------------------------- 3. several planes
def test_nested_glass_four_planes(gpu, tmp_path):
    """15 meshes: four planes, of which the concentric shells leave the two middle ones empty (only
    the outermost shell is ever hit first; the backdrop is id 14)."""
    scene = nart_amd.Scene(scenes.nested_glass(str(tmp_path), n=14))
    p = _params(scene, 24, 20, 2)
    entry = _restated_planes(scene, "nested14", p, MATTE_MESH)
    assert entry["n"] == 15 and entry["planes"].shape[0] == 4
    assert entry["planes"][0][..., 0].max() > 0 and entry["planes"][3][..., 2].max() > 0
    assert not entry["planes"][1][..., :4].any() and not entry["planes"][2][..., :4].any()
    r = nart_amd.HipRenderer(scene)
    out = _check_call(r, p, _mp(ranks=4), entry)
    assert set(np.unique(out["ranks"][:, :, :, (0, 2)]).tolist()) <= {-1.0, 0.0, 14.0}
    r.close()


# ---------------------------------------------------------------- 4. ranking and extraction on synthetic planes
@pytest.fixture(scope="module")
def glass_renderer(gpu, glass_scene):
    r = nart_amd.HipRenderer(glass_scene)
    yield r
    r.close()


SIZES = [(1, 1), (33, 9), (70, 20)]


@pytest.mark.parametrize("R", [2, 8])
@pytest.mark.parametrize("n", [1, 5, 32])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_rank_and_extract_synthetic(glass_renderer, glass_scene, size, n, R):
    """Partial 32 x 8 tiles (33 and 70 wide, 9 and 20 high), one pixel; one id, ids in a second plane
    whose padding channels hold values, all 32; ties, NaN and W <= 0."""
    W, H = size
    p = _params(glass_scene, W, H, 1)
    g = nart_amd.session_geometry(p)
    fb = g.filter_bounds
    planes, spots = mp.synthetic(W, H, fb, n, seed=W * 131 + H + n)
    m = _mp(ranks=R)
    got = glass_renderer.matte_rank(p, planes, n, m)
    want = mp.rank(W, H, fb, planes, n, R)
    assert got["ranks"].shape == want.shape == (R // 2, g.total_height, g.total_width, 5)
    assert _bits_equal(got["ranks"], want), _report(got["ranks"], want)
    assert got["rank_ms"] > 0 and got["matte_ms"] == 0
    if W * H > 1:
        assert len(spots) == 8 and not np.isfinite(planes).all()
        for name in ("w_zero", "w_negative", "w_nan", "all_zero"):
            x, y = spots[name]
            assert got["ranks"][:, y + fb, x + fb].tolist() == [[-1, 0, -1, 0, 1]] * (R // 2), name
        x, y = spots["all_equal"]
        assert got["ranks"][0, y + fb, x + fb].tolist() == ([0, 0.5, 1, 0.5, 1] if n > 1 else [0, 0.5, -1, 0, 1])
        first = want[0][fb:fb + H, fb:fb + W]
        ties = (first[..., 1] == first[..., 3]) & (first[..., 0] >= 0) & (first[..., 2] >= 0)
        assert n == 1 or (ties.any() and (first[..., 0][ties] < first[..., 2][ties]).all())
    for mask in (0, 1, 0b10110, (1 << 64) - 1, 1 << 31, 1 << 40):
        ext = glass_renderer.matte_extract(p, got["ranks"], mask, m)
        ref = mp.extract(W, H, fb, want, mask)
        assert _bits_equal(ext, ref), (mask, _report(ext, ref))


def test_rank_without_ids(glass_renderer, glass_scene):
    """No ids, no planes: every cropped pixel is {-1, 0, -1, 0, 1}, the border zero."""
    p = _params(glass_scene, 33, 9, 1)
    g = nart_amd.session_geometry(p)
    fb = g.filter_bounds
    got = glass_renderer.matte_rank(p, np.zeros((0, g.total_height, g.total_width, 5), f32), 0, _mp(ranks=4))["ranks"]
    want = mp.rank(33, 9, fb, np.zeros((0, g.total_height, g.total_width, 5), f32), 0, 4)
    assert _bits_equal(got, want) and got[:, fb, fb].tolist() == [[-1, 0, -1, 0, 1]] * 2 and not got[:, 0].any()


# ---------------------------------------------------------------- 5. batches and devices
def test_mattes_batches(gpu, glass_scene, monkeypatch):
    """NART_BATCH_BYTES=1 leaves 256 slots (tests/test_gpu_moment.py test_moment_batches): the 28 x 24
    total frame's buckets go in three batches, each writing its own records and splatting them into its
    own offset of the back-to-back tile slabs."""
    p = _params(glass_scene, 24, 20, 2, **CONFIGS["b16_fw2"])
    m = _mp(ranks=4)
    one = nart_amd.HipRenderer(glass_scene)
    ref = one.render_mattes(p, m, with_beauty=True, with_planes=True)
    one.close()
    monkeypatch.setenv("NART_BATCH_BYTES", "1")
    r = nart_amd.HipRenderer(glass_scene)
    st, st_only = nart_amd.RenderStats(), nart_amd.RenderStats()
    out = r.render_mattes(p, m, with_beauty=True, with_planes=True, stats=st)
    only = r.render_mattes(p, m, with_planes=True, stats=st_only)
    r.close()
    assert st.kernel_launches == 3 and st_only.kernel_launches == 0
    for name in ("ranks", "beauty", "planes"):
        assert _bits_equal(out[name], ref[name]), (name, _report(out[name], ref[name]))
    assert _bits_equal(only["ranks"], ref["ranks"]) and _bits_equal(only["planes"], ref["planes"])


def test_two_rank_rehearsal(gpu, materials_scene):
    p = _params(materials_scene, 64, 48, 2)
    m = _mp(kind=MATTE_MATERIAL, ranks=4)
    one = nart_amd.HipRenderer(materials_scene)
    single = one.render_mattes(p, m, with_beauty=True, with_planes=True)
    plain = one.render(p)
    one.close()
    assert single["planes"].shape[0] == 2 and single["planes"][1][..., :3].max() > 0
    r = nart_amd.HipRenderer(materials_scene, devices=[0, 0])
    assert r.devices() == (2, False)
    got = r.render_mattes(p, m, with_beauty=True, with_planes=True)
    for name in ("ranks", "beauty", "planes"):
        assert _bits_equal(got[name], single[name]), (name, _report(got[name], single[name]))
    assert got["matte_ms"] > 0 and got["rank_ms"] > 0
    st = nart_amd.RenderStats()
    alone = r.render_mattes(p, m, stats=st)
    assert _bits_equal(alone["ranks"], single["ranks"]) and st.kernel_launches == 0
    assert _bits_equal(r.matte_rank(p, got["planes"], got["n_ids"], m)["ranks"], single["ranks"])
    g = nart_amd.session_geometry(p)
    want = mp.extract(p.image_width, p.image_height, g.filter_bounds, single["ranks"], 1 << 5)
    assert _bits_equal(r.matte_extract(p, got["ranks"], [5], m), want) and want[..., 0].max() > 0
    assert _bits_equal(r.render(p), plain)
    r.close()


# ---------------------------------------------------------------- 6. errors, and the other entry points' bits
def test_matte_errors_leave_the_context_usable(gpu, glass_scene, glass_renderer, volume_scenes, tmp_path):
    r = glass_renderer
    p = _params(glass_scene, 32, 24, 2)
    g = nart_amd.session_geometry(p)
    good = r.render(p)
    ok = r.render_mattes(p, with_beauty=True, with_planes=True)
    lib = nart_amd.hip_lib()
    img = np.zeros((4, g.total_height, g.total_width, 5), f32)
    P, ptr = ctypes.byref(p), lambda a: a.ctypes.data
    for kw in BAD:
        c = _mp(**kw)
        for call in (lambda: r.render_mattes(p, c), lambda: r.matte_rank(p, ok["planes"], ok["n_ids"], c),
                     lambda: r.matte_extract(p, np.zeros((c.ranks // 2,) + good.shape, f32), 1, c)):
            with pytest.raises(nart_amd.NartError) as e:
                call()
            assert e.value.code == -1, kw
        assert lib.nart_hip_render_mattes(r._ctx, P, ctypes.byref(c), ptr(img), None, None, None) == -1, kw
        assert "matte" in lib.nart_hip_last_error(r._ctx).decode()
        assert lib.nart_hip_matte_rank(r._ctx, P, ctypes.byref(c), 4, ptr(img), ptr(img)) == -1, kw
        assert lib.nart_hip_matte_extract(r._ctx, P, ctypes.byref(c), ptr(img), 1, ptr(img)) == -1, kw
    assert _bits_equal(r.render(p), good)
    assert lib.nart_hip_render_mattes(r._ctx, P, None, None, ptr(img), None, None) == -1      # no rank images
    assert lib.nart_hip_render_mattes(r._ctx, None, None, ptr(img), None, None, None) == -1   # no params
    assert lib.nart_hip_matte_rank(r._ctx, P, None, 4, None, ptr(img)) == -1
    assert lib.nart_hip_matte_rank(r._ctx, P, None, 4, ptr(img), None) == -1
    assert lib.nart_hip_matte_rank(r._ctx, P, None, 33, ptr(img), ptr(img)) == -1
    assert lib.nart_hip_matte_extract(r._ctx, P, None, None, 1, ptr(img)) == -1
    assert lib.nart_hip_matte_extract(r._ctx, P, None, ptr(img), 1, None) == -1
    again = r.render_mattes(p, with_beauty=True, with_planes=True)
    for name in ("ranks", "beauty", "planes"):
        assert _bits_equal(again[name], ok[name]), name
    assert _bits_equal(again["beauty"], good)
    # the volume integrator has no surfaces
    vol = volume_scenes["emissive"]
    pv = _params(vol, 24, 20, 2)
    rv = nart_amd.HipRenderer(vol)
    before = rv.render(pv)
    for kw in (dict(), dict(with_beauty=True)):
        with pytest.raises(nart_amd.NartError) as e:
            rv.render_mattes(pv, **kw)
        assert e.value.code == -6
    assert _bits_equal(rv.render(pv), before)
    # the same scene has no meshes: under the path integrator (NART_INTEGRATOR_PATH = 0) a matte-only
    # call has no ids, renders no plane and returns empty ranks
    pp = _params(vol, 24, 20, 2)
    pp.integrator = 0
    gv = nart_amd.session_geometry(pp)
    none = rv.render_mattes(pp, _mp(ranks=4), with_planes=True)
    assert none["n_ids"] == 0 and none["planes"].shape[0] == 0 and none["matte_ms"] == 0
    empty = np.zeros((0, gv.total_height, gv.total_width, 5), f32)
    assert _bits_equal(none["ranks"], mp.rank(24, 20, gv.filter_bounds, empty, 0, 4))
    assert _bits_equal(rv.render(pv), before)
    rv.close()
    # 34 meshes: refused at render for mesh ids; the materials are as many
    big = nart_amd.Scene(scenes.nested_glass(str(tmp_path), n=33))
    pb = _params(big, 24, 20, 1)
    rb = nart_amd.HipRenderer(big)
    before = rb.render(pb)
    for kind in (MATTE_MESH, MATTE_MATERIAL):
        with pytest.raises(nart_amd.NartError) as e:
            rb.render_mattes(pb, _mp(kind=kind), with_beauty=True)
        assert e.value.code == -6
    assert _bits_equal(rb.render(pb), before)
    rb.close()


def test_other_entry_points_keep_their_bits(gpu, glass_scene):
    """render, render_aovs(moment=True), render_robust and render_denoised give the same bits, launches
    and schedule before and after matte calls on the same context."""
    p = _params(glass_scene, 48, 32, 4)
    r = nart_amd.HipRenderer(glass_scene)

    def snapshot():
        st, st_a, st_r, st_d = (nart_amd.RenderStats() for _ in range(4))
        a = r.render(p, st)
        b = r.render_aovs(p, moment=True, stats=st_a)
        c = r.render_robust(p, with_beauty=True, with_layers=True, stats=st_r)
        d = r.render_denoised(p, stats=st_d)
        return ({"render": a, "albedo": b["albedo"], "normal": b["normal"], "moment": b["moment"], "beauty": b["beauty"],
                 "robust": c["robust"], "layers": c["layers"], "denoised": d["denoised"]},
                [(s.kernel_launches, s.schedule) for s in (st, st_a, st_r, st_d)])

    before, st_before = snapshot()
    r.render_mattes(p, _mp(kind=MATTE_MATERIAL, ranks=8), with_beauty=True, with_planes=True)
    r.render_mattes(p)
    after, st_after = snapshot()
    assert st_before == st_after
    for name in before:
        assert _bits_equal(before[name], after[name]), name
    r.close()


# ---------------------------------------------------------------- 7. CLI
def test_cli_mattes(gpu, materials_scene, tmp_path):
    base = [NART, materials_scene.path]
    size = ["-w", "40", "-h", "24", "-s", "2"]

    def run(out, extra, ok=True):
        res = subprocess.run(base + [str(out)] + size + extra, capture_output=True, text=True, timeout=300)
        assert (res.returncode == 0) == ok, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
        return res

    dirs = {k: tmp_path / k for k in ("mesh", "mat", "aov", "bad")}
    for d in dirs.values():
        d.mkdir()
    run(dirs["mesh"] / "out", ["--mattes"])
    run(dirs["mat"] / "out", ["--mattes", "material", "--matte-ranks", "4", "--matte-ids", "5,6"])
    run(dirs["aov"] / "out", ["--aovs", "--mattes", "mesh", "--matte-ranks", "2"])
    assert sorted(os.listdir(dirs["mesh"])) == ["out.exr", "out.matte.00.exr", "out.matte.01.exr", "out.matte.02.exr"]
    assert sorted(os.listdir(dirs["mat"])) == ["out.exr", "out.matte.00.exr", "out.matte.01.exr", "out.matte.exr"]
    assert sorted(os.listdir(dirs["aov"])) == ["out.albedo.exr", "out.exr", "out.matte.00.exr", "out.normal.exr"]
    p = nart_amd.parse_args(["nart", materials_scene.path, "out"] + size)
    p = nart_amd.load_sessions(materials_scene.path, p)[0]
    r = nart_amd.HipRenderer(materials_scene)
    to_half = nart_amd.scene_lib().nart_float_to_half

    def halves_of(img):
        final = nart_amd.finalize(p, img)
        return np.array([to_half(ctypes.c_float(v)) for v in final.reshape(-1)], np.uint16).reshape(final.shape)

    def same(path, img):
        halves, _hdr = exr_py.read_rgba_halves(str(path))
        return halves.shape == (24, 40, 4) and np.array_equal(halves, halves_of(img))

    api = r.render_mattes(p, with_beauty=True)
    assert same(dirs["mesh"] / "out.exr", api["beauty"])
    for k in range(3):
        assert same(dirs["mesh"] / ("out.matte.0%d.exr" % k), api["ranks"][k]), k
    m = _mp(kind=MATTE_MATERIAL, ranks=4)
    api = r.render_mattes(p, m)
    for k in range(2):
        assert same(dirs["mat"] / ("out.matte.0%d.exr" % k), api["ranks"][k]), k
    assert same(dirs["mat"] / "out.matte.exr", r.matte_extract(p, api["ranks"], [5, 6], m))
    api = r.render_mattes(p, _mp(ranks=2))
    assert same(dirs["aov"] / "out.matte.00.exr", api["ranks"][0])
    assert same(dirs["aov"] / "out.exr", r.render(p))
    r.close()
    # refused combinations and bad values: a message, no output
    for extra in (["--mattes", "--adaptive", "0.1"], ["--mattes", "--robust"], ["--mattes", "--matte-ranks", "3"],
                  ["--mattes", "--matte-ranks", "10"], ["--mattes", "--matte-ranks", "x"], ["--mattes", "--matte-ids", "1,,2"],
                  ["--mattes", "--matte-ids", "32"], ["--mattes", "--matte-ids", "-1"], ["--matte-ranks", "4"],
                  ["--matte-ids", "1"], ["--mattes", "--matte-ranks"]):
        res = run(dirs["bad"] / "out", extra, ok=False)
        assert "matte" in res.stderr and not res.stdout, extra
    assert os.listdir(dirs["bad"]) == []
