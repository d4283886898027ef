"""Followed guides (nart_hip_render_guides, nart_hip_render_denoised_guides,
nart_hip_render_guide_samples, `nart --follow-specular`) on the device: every traced segment against
the oracle's octree answer for the device's own reported ray, every chain step against the float64
restatement (tests/guide_py.py) from the device's own previous segment, the records against the
reported segments, the images bit for bit against the numpy restatement of the splat and the tile
combine over the device's own records, and the invariants that tie the feature to what was there
before: max_follow = 0 and scenes without delta surfaces give the first-hit AOVs bit for bit, and
nothing else changes its bits."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import aov_py
import exr_py
import guide_py
import nart_amd
import oracle
from guide_py import FOLLOWED, GUIDE_HIT, STEPPED
from nart_amd import GuideParams, scenes
from test_aov_restatement import restate_render, total_frame_uv

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NART = os.path.join(REPO, "nart_amd", "bin", "nart")
NO_HIT = aov_py.NO_HIT
MF = 8


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
    return "%d of %d floats differ, max abs diff %g" % (int(ne.sum()), ne.size, float(np.nanmax(np.abs(a - b))))


# ---------------------------------------------------------------- scenes and blocks
def _lit_two_spheres(directory):
    """guide_py.two_sphere_scene with two disk lights back to back between the farther sphere and
    the wall (whichever way a disk faces, one of them bounds a ray that travels towards the wall)."""
    path = guide_py.two_sphere_scene(directory)
    with open(path) as f:
        scene = json.load(f)
    for rot in ([1, 0, 0, 0, 0, -1, 0, 1, 0], [1, 0, 0, 0, 0, 1, 0, -1, 0]):
        scene["lights"].append({"type": "disk", "radius": 0.5, "Le": [1, 1, 1], "intensity": 5.0,
                                "transform": rot[0:3] + [0.0] + rot[3:6] + [1.5] + rot[6:9] + [1.0] + [0, 0, 0, 1]})
    lit = os.path.join(directory, "two_spheres_lit.json")
    with open(lit, "w") as f:
        json.dump(scene, f, indent=1)
    return lit


# Per scene: frame (w, h, spp), max_follow and 8x8 blocks in total-image coordinates.
#   glass      the sphere's centre, its silhouette, backdrop only, the frame's last corner (extra rows)
#   materials  the mirror sphere, its silhouette against the wall, the plastic sphere, the last corner
#   two        the overlap of the two spheres (step-through); lit: the same with a light behind them
#   nested*    the middle of the 14 shells at three limits
BLOCKS = {
    "glass": ((48, 48, 4), MF, [(16, 20, 8, 8), (22, 16, 8, 8), (36, 36, 8, 8), (44, 44, 8, 8)]),
    "materials": ((64, 48, 4), MF, [(28, 16, 8, 8), (33, 14, 8, 8), (40, 17, 8, 8), (60, 44, 8, 8)]),
    "two": ((48, 36, 2), MF, [(20, 16, 8, 8)]),
    "lit": ((48, 36, 2), MF, [(20, 16, 8, 8)]),
    "nested3": ((48, 36, 2), 3, [(22, 16, 8, 8)]),
    "nested8": ((48, 36, 2), 8, [(22, 16, 8, 8)]),
    "nested10": ((48, 36, 2), 10, [(22, 16, 8, 8)]),
}
_cache = {}
_scenes = {}


def _scene_of(name, request):
    if name in ("glass", "materials", "cornell"):
        return request.getfixturevalue({"glass": "glass_scene", "materials": "materials_scene",
                                        "cornell": "cornell_scene"}[name])
    key = "nested" if name.startswith("nested") else name
    if key not in _scenes:
        d = str(request.getfixturevalue("tmp_path_factory").mktemp("guides_" + key))
        path = {"two": guide_py.two_sphere_scene, "lit": _lit_two_spheres, "nested": scenes.nested_glass}[key](d)
        _scenes[key] = nart_amd.Scene(path)
    return _scenes[key]


def _replay(gs, dev, idx, mf):
    """One sample's chain through the restatement, each step from the device's own reported segment:
    per followed or stepped-through segment the float64 next ray, the float32 one and the device's."""
    n = max(int(dev["n_seg"][idx]), 1)
    l32, l64 = guide_py.NestedList(), guide_py.NestedList()
    steps = []
    for j in range(n):
        seg, tri = dev["seg"][idx][j], int(dev["tri"][idx][j])
        if tri == NO_HIT:
            steps.append({"decision": guide_py.MISS})
            break
        o, d = seg[0:3], seg[4:7]
        l64.e = list(l32.e)  # the float32 chain is the device's: its list carries on
        s32 = guide_py.step(gs, tri, o, d, l32, j, mf, np.float32)
        s64 = guide_py.step(gs, tri, o, d, l64, j, mf, np.float64)
        s32["next64"] = None if s64["o"] is None else np.concatenate([s64["o"], s64["d"]])
        s32["decision64"] = s64["decision"]
        steps.append(s32)
        if s32["decision"] == GUIDE_HIT:
            break
    return steps


def _blocks(name, request):
    """The device's chains of a scene's blocks and their replay through the restatement, computed
    once and shared (read-only) by the tests."""
    if name not in _cache:
        sc = _scene_of(name, request)
        (w, h, spp), mf, rects = BLOCKS[name]
        p = _params(sc, w, h, spp)
        gs, orc = guide_py.GuideScene(sc), oracle.Oracle(sc)
        r = nart_amd.HipRenderer(sc)
        out = []
        for rect in rects:
            dev = r.render_guide_samples(p, *rect, GuideParams(max_follow=mf))
            replay = {idx: _replay(gs, dev, idx, mf) for idx in np.ndindex(dev["n_seg"].shape)}
            out.append({"rect": rect, "dev": dev, "replay": replay})
        r.close()
        _cache[name] = (sc, p, gs, orc, mf, out)
    return _cache[name]


# ---------------------------------------------------------------- 1. traversal
@pytest.mark.parametrize("name", ["glass", "materials", "lit"])
def test_every_segment_is_the_octrees_answer(gpu, request, name):
    """For every sample and every segment the device reports, nothing excluded: oracle.trace of the
    device's own ray within its own bound returns the reported triangle and t bit for bit, and a
    segment reported as a miss is the oracle's miss."""
    _sc, _p, gs, orc, mf, blocks = _blocks(name, request)
    n_hit = n_miss = n_deep = 0
    per_block = []
    for b in blocks:
        dev = b["dev"]
        hits0 = 0
        for idx in np.ndindex(dev["n_seg"].shape):
            n = int(dev["n_seg"][idx])
            assert 0 <= n <= mf + 1
            for j in range(max(n, 1)):
                seg, tri = dev["seg"][idx][j], int(dev["tri"][idx][j])
                got = oracle.trace(orc, seg[0:3], seg[4:7], float(seg[3]))
                if tri == NO_HIT:
                    assert got[0] < 0, (name, idx, j, got)
                    assert j == max(n, 1) - 1 and (n == 0) == (j == 0)  # a miss ends the chain
                    n_miss += 1
                else:
                    assert got[0] == tri, (name, idx, j, got, tri)
                    assert np.float32(got[1]).view(np.uint32) == seg[7:8].view(np.uint32)[0], (name, idx, j, got[1], seg[7])
                    n_hit += 1
                    n_deep += j > 0
                    hits0 += j == 0
            for j in range(max(n, 1), mf + 1):  # never traced
                assert dev["tri"][idx][j] == NO_HIT and not dev["seg"][idx][j].any()
        per_block.append(hits0 / dev["n_seg"].size)
    assert n_hit > 200 and n_deep > 100 and (n_miss > 0 or name == "glass"), (n_hit, n_deep, n_miss)
    if name == "glass":  # first hits: centre all glass, silhouette mixed, backdrop and corner all backdrop
        def first_mesh(b):
            t = b["dev"]["tri"][..., 0]
            return np.where(t == NO_HIT, -1, gs.tri_mesh[np.minimum(t, len(gs.tri_mesh) - 1).astype(np.int64)])
        assert per_block[0] == 1.0 and np.all(first_mesh(blocks[0]) == 0)
        assert 0.05 < (first_mesh(blocks[1]) == 0).mean() < 0.95
        assert np.all(first_mesh(blocks[2]) == 2) and np.all(first_mesh(blocks[3]) == 2)
        assert blocks[3]["rect"][0] + 8 == 52 and blocks[3]["rect"][1] + 8 == 52  # the extra rows and columns


# ---------------------------------------------------------------- 2. the chain step
@pytest.mark.parametrize("name", ["glass", "materials", "two", "lit", "nested3", "nested8", "nested10"])
def test_chain_steps_match_the_restatement(gpu, request, name):
    """The decision at every hit (followed / stepped through / guide hit / miss) and n_seg match the
    restatement exactly; the device's next ray is within tolerance of the float64 restatement from
    the device's own previous segment, so no sample is excluded.  Tolerance: 4x the largest gap, over
    these same samples, between the float32 restatement (the device's operation order) and the
    float64 one, as tests/test_gpu_aovs.py test_normal_matches_float64_restatement finds its own."""
    _sc, _p, _gs, _orc, mf, blocks = _blocks(name, request)
    gap = worst = 0.0
    counts = {FOLLOWED: 0, STEPPED: 0, GUIDE_HIT: 0, guide_py.MISS: 0}
    for b in blocks:
        dev = b["dev"]
        for idx, steps in b["replay"].items():
            n = int(dev["n_seg"][idx])
            assert len(steps) == max(n, 1), (name, idx, len(steps), n)  # n_seg
            for j, s in enumerate(steps):
                counts[s["decision"]] += 1
                last = j == len(steps) - 1
                if s["decision"] in (GUIDE_HIT, guide_py.MISS):
                    assert last, (name, idx, j)
                    continue
                assert not last and s["decision64"] == s["decision"], (name, idx, j, s["decision"])
                nxt = np.concatenate([dev["seg"][idx][j + 1][0:3], dev["seg"][idx][j + 1][4:7]]).astype(np.float64)
                n32 = np.concatenate([s["o"], s["d"]]).astype(np.float64)
                gap = max(gap, float(np.abs(n32 - s["next64"]).max()))
                worst = max(worst, float(np.abs(nxt - s["next64"]).max()))
    tol = 4.0 * gap
    print("chain step on %s: float32 vs float64 gap %.3g, tolerance %.3g, device vs float64 %.3g, decisions %s"
          % (name, gap, tol, worst, counts))
    assert counts[FOLLOWED] + counts[STEPPED] > 100 and worst <= tol, (worst, tol)
    if name in ("two", "lit"):
        assert counts[STEPPED] > 50  # the lower-priority interface inside the nearer sphere
    if name.startswith("nested"):
        deepest = max(int(b["dev"]["n_seg"].max()) for b in blocks)
        assert deepest == mf + 1  # the limit, and nothing beyond it


def test_step_through_on_the_device(gpu, request):
    """The two-sphere scene's middle: the reported triangles' meshes are near, far (stepped through,
    same direction), near, far, wall, and the sample ends on the wall's albedo."""
    sc, _p, gs, _orc, _mf, blocks = _blocks("two", request)
    dev = blocks[0]["dev"]
    full = 0
    for idx in np.ndindex(dev["n_seg"].shape):
        if dev["n_seg"][idx] != 5:
            continue
        meshes = [int(gs.tri_mesh[t]) for t in dev["tri"][idx][:5]]
        if meshes != [0, 1, 0, 1, 2]:
            continue
        full += 1
        assert _bits_equal(dev["seg"][idx][2][4:7], dev["seg"][idx][1][4:7])  # stepped through: the direction stays
        assert _bits_equal(dev["rec"][idx][:4], np.float32([0.5, 0.4, 0.3, 1.0]))
    assert full > 50, full


def test_light_between_segments_bounds_the_chain(gpu, request):
    """A disk light behind the spheres: the segment that leaves them towards the wall has a finite
    bound, misses within it (the unbounded oracle query hits the wall) and the sample is a miss."""
    _sc, _p, _gs, orc, _mf, blocks = _blocks("lit", request)
    dev = blocks[0]["dev"]
    cut = 0
    for idx in np.ndindex(dev["n_seg"].shape):
        n = int(dev["n_seg"][idx])
        if n < 2 or dev["tri"][idx][n - 1] != NO_HIT:
            continue
        seg = dev["seg"][idx][n - 1]
        assert np.isfinite(seg[3]) and seg[7] == seg[3]
        assert oracle.trace(orc, seg[0:3], seg[4:7])[0] >= 0
        assert not dev["rec"][idx].any()
        cut += 1
    assert cut > 50, cut


# ---------------------------------------------------------------- 3. records
@pytest.mark.parametrize("name", ["glass", "materials", "nested3"])
def test_records(gpu, request, name):
    """D is the float32 sum of the reported t in order, bit for bit; the albedo is the guide
    triangle's pattern value (constant patterns; on `materials` the textured ground and wall seen in
    the mirror, texel-boundary samples left out: at most 2 %); the normal is within the first-hit
    normal test's tolerance method of the float64 restatement at the last segment's ray (surfaces
    without a normal map); a miss is all zeros."""
    _sc, _p, gs, _orc, mf, blocks = _blocks(name, request)
    n_guide = n_miss = n_tex = n_tex_deep = n_left_out = 0
    gap = 0.0
    normals = []
    for b in blocks:
        dev = b["dev"]
        for idx in np.ndindex(dev["n_seg"].shape):
            n, rec = int(dev["n_seg"][idx]), dev["rec"][idx]
            if n == 0 or dev["tri"][idx][n - 1] == NO_HIT:
                assert not rec.any(), (name, idx)
                n_miss += 1
                continue
            n_guide += 1
            D = np.float32(0)
            for j in range(n):
                D = np.float32(D + dev["seg"][idx][j][7])
            assert D.view(np.uint32) == rec[7:8].view(np.uint32)[0], (name, idx, D, rec[7])
            assert rec[3] == 1.0
            tri, seg = int(dev["tri"][idx][n - 1]), dev["seg"][idx][n - 1]
            want, near = guide_py.albedo_value(gs, tri, seg[0:3], seg[4:7])
            textured = aov_py.albedo_pattern(gs.mats[gs.tri_mat[tri]]).type == nart_amd.api.PTN_TEXTURE
            n_tex += textured
            n_tex_deep += textured and n > 1
            if near:
                n_left_out += 1
            else:
                assert _bits_equal(rec[:3], want), (name, idx, n, rec[:3], want)
            if not gs.has_normal_map(tri):
                T = gs.tris[tri]
                n64 = aov_py.shading_normal(T, seg[0:3], seg[4:7], np.float64)
                n32 = aov_py.shading_normal(T, seg[0:3], seg[4:7], np.float32)
                gap = max(gap, float(np.abs(n32.astype(np.float64) - n64).max()))
                normals.append(float(np.abs(rec[4:7].astype(np.float64) - n64).max()))
    worst = max(normals)
    tol = 4.0 * gap
    print("records on %s: %d guide hits, %d misses, normal gap %.3g, tolerance %.3g, device vs float64 %.3g"
          % (name, n_guide, n_miss, gap, tol, worst))
    assert n_guide > 100 and len(normals) > 100 and worst <= tol, (worst, tol)
    assert n_left_out <= 0.02 * max(n_tex, 1), (n_tex, n_left_out)
    if name == "materials":
        assert n_tex_deep > 50, n_tex_deep  # textured albedo through the mirror


# ---------------------------------------------------------------- 4. invariants
SMALL = dict(bucket_size=16, filter_width=2.0)


@pytest.mark.parametrize("name,max_follow", [("glass", 0), ("cornell", 8)])
def test_first_hit_records_bit_for_bit(gpu, request, name, max_follow):
    """max_follow = 0 on glassSphere, and the Cornell box (no delta surface) at max_follow = 8: the
    per-sample records and both images are the first-hit AOVs' bit for bit."""
    sc = _scene_of(name, request)
    p = _params(sc, 24, 20, 2, **SMALL)
    g = nart_amd.session_geometry(p)
    gp = GuideParams(max_follow=max_follow)
    r = nart_amd.HipRenderer(sc)
    rec, tri = r.render_aov_samples(p, 0, 0, g.total_width, g.total_height)
    dev = r.render_guide_samples(p, 0, 0, g.total_width, g.total_height, gp)
    assert (rec[..., 3] == 1.0).any() and (tri == NO_HIT).any() == (rec[..., 3] == 0.0).any()
    assert _bits_equal(dev["rec"], rec), _report(dev["rec"], rec)
    assert np.array_equal(dev["tri"][..., 0], tri) and dev["n_seg"].max() == 1
    first, followed = r.render_aovs(p), r.render_guides(p, gp)
    for k in ("beauty", "albedo", "normal"):
        assert _bits_equal(followed[k], first[k]), (k, _report(followed[k], first[k]))
    assert followed["guide_ms"] > 0.0


@pytest.mark.parametrize("variant", [0, 3], ids=["rayqueue", "megakernel"])
def test_beauty_and_later_renders_unchanged(gpu, glass_scene, variant):
    p = _params(glass_scene, 40, 32, 4)
    r = nart_amd.HipRenderer(glass_scene, variant=variant)
    st0, st1 = nart_amd.RenderStats(), nart_amd.RenderStats()
    before = r.render(p, st0)
    out = r.render_guides(p, moment=True, stats=st1)
    after = r.render(p)
    ref = oracle.Oracle(glass_scene).render(p)
    assert _bits_equal(before, ref) and _bits_equal(out["beauty"], ref), _report(out["beauty"], ref)
    assert _bits_equal(after, ref)
    assert st1.schedule == st0.schedule and st1.kernel_launches == st0.kernel_launches
    assert _bits_equal(out["moment"], r.render_aovs(p, albedo=False, normal=False, moment=True)["moment"])
    # the guides see through the glass: they differ from the first-hit AOVs
    first = r.render_aovs(p)
    assert not _bits_equal(out["normal"], first["normal"])


# ---------------------------------------------------------------- 5. images
_restated = {}


def _restated_guides(glass_scene, spp):
    """The restatement's guide images of glassSphere 24x20 over the device's own per-sample records
    of the whole total frame (the records do not depend on the splat mode)."""
    if spp not in _restated:
        p = _params(glass_scene, 24, 20, spp, **SMALL)
        g = nart_amd.session_geometry(p)
        r = nart_amd.HipRenderer(glass_scene)
        rec = r.render_guide_samples(p, 0, 0, g.total_width, g.total_height, GuideParams(max_follow=MF))["rec"]
        r.close()
        uv = total_frame_uv(p)
        _restated[spp] = (p, restate_render(p, uv, np.ascontiguousarray(rec[..., :4])),
                          restate_render(p, uv, np.ascontiguousarray(rec[..., 4:])))
    return _restated[spp]


@pytest.mark.parametrize("spp", [8, 3], ids=["rows_of_eight", "one_by_one"])
@pytest.mark.parametrize("splat_mode", [5, 4, 3, 0], ids=["rows", "skew", "col4", "direct"])
def test_guide_images_equal_restated_splat(gpu, glass_scene, spp, splat_mode):
    """8 spp: the kernel's eight-samples-per-read path on pixel-major rows; 3 spp: the other."""
    p, albedo, normal = _restated_guides(glass_scene, spp)
    assert albedo[..., 3].max() > 0 and np.abs(normal[..., :3]).max() > 0
    out = nart_amd.HipRenderer(glass_scene, splat_mode=splat_mode).render_guides(p, GuideParams(max_follow=MF))
    assert _bits_equal(out["albedo"], albedo), _report(out["albedo"], albedo)
    assert _bits_equal(out["normal"], normal), _report(out["normal"], normal)


def test_guide_images_in_three_batches(gpu, glass_scene, monkeypatch):
    """NART_BATCH_BYTES=1 leaves 256 slots: the 28 x 24 total frame's buckets go in three batches,
    each tracing its own chains, holding its own second record buffer and splatting into its own
    offset of the tile slabs.  One guide alone (no second buffer) gives the same image."""
    p, albedo, normal = _restated_guides(glass_scene, 3)
    monkeypatch.setenv("NART_BATCH_BYTES", "1")
    r = nart_amd.HipRenderer(glass_scene)
    st = nart_amd.RenderStats()
    out = r.render_guides(p, GuideParams(max_follow=MF), stats=st)
    only = r.render_guides(p, GuideParams(max_follow=MF), albedo=False, beauty=False)
    r.close()
    assert st.kernel_launches == 3
    assert _bits_equal(out["albedo"], albedo) and _bits_equal(out["normal"], normal)
    assert set(only) == {"normal", "guide_ms"} and _bits_equal(only["normal"], normal)


# ---------------------------------------------------------------- 6. denoiser
@pytest.mark.parametrize("sample_variance", [False, True], ids=["spatial", "sample_variance"])
def test_denoised_with_guides(gpu, glass_scene, sample_variance):
    p = _params(glass_scene, 40, 32, 4)
    gp = GuideParams(max_follow=MF)
    r = nart_amd.HipRenderer(glass_scene)
    old = r.render_denoised(p, sample_variance=sample_variance)
    imgs = r.render_guides(p, gp, moment=sample_variance)
    want = r.denoise(p, imgs["beauty"], imgs["albedo"], imgs["normal"], moment=imgs["moment"] if sample_variance else None)
    got = r.render_denoised(p, sample_variance=sample_variance, guides=gp)
    assert _bits_equal(got["denoised"], want), _report(got["denoised"], want)
    assert _bits_equal(got["beauty"], imgs["beauty"]) and got["denoise_ms"] > 0.0
    assert not _bits_equal(got["denoised"], old["denoised"])  # other guides, another image
    again = r.render_denoised(p, sample_variance=sample_variance)
    assert _bits_equal(again["denoised"], old["denoised"]) and _bits_equal(again["beauty"], old["beauty"])


# ---------------------------------------------------------------- 7. multi-device and CLI
def test_two_rank_rehearsal_matches_single(gpu, glass_scene):
    p = _params(glass_scene, 48, 36, 4)
    gp = GuideParams(max_follow=MF)
    single = nart_amd.HipRenderer(glass_scene).render_guides(p, gp, moment=True)
    m = nart_amd.HipRenderer(glass_scene, devices=[0, 0])
    assert m.devices() == (2, False)
    got = m.render_guides(p, gp, moment=True)
    for name in ("beauty", "albedo", "normal", "moment"):
        assert _bits_equal(got[name], single[name]), (name, _report(got[name], single[name]))
    one = nart_amd.HipRenderer(glass_scene)
    want = one.render_denoised(p, guides=gp)["denoised"]
    assert _bits_equal(m.render_denoised(p, guides=gp)["denoised"], want)
    dev = m.render_guide_samples(p, 20, 16, 4, 4, gp)
    assert _bits_equal(dev["rec"], one.render_guide_samples(p, 20, 16, 4, 4, gp)["rec"])


def test_cli_follow_specular(gpu, glass_scene, tmp_path):
    def run(out, extra):
        return subprocess.run([NART, glass_scene.path, out, "-w", "48", "-h", "32", "-s", "4"] + extra,
                              capture_output=True, text=True, timeout=300)

    first_dir, out_dir = tmp_path / "first", tmp_path / "followed"
    first_dir.mkdir()
    out_dir.mkdir()
    assert run(str(first_dir / "out"), ["--aovs", "--denoise"]).returncode == 0
    r = run(str(out_dir / "out"), ["--aovs", "--denoise", "--follow-specular"])
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    names = ["out.albedo.exr", "out.denoised.exr", "out.exr", "out.normal.exr"]
    assert sorted(os.listdir(out_dir)) == names
    assert (first_dir / "out.exr").read_bytes() == (out_dir / "out.exr").read_bytes()
    assert (first_dir / "out.normal.exr").read_bytes() != (out_dir / "out.normal.exr").read_bytes()
    p = nart_amd.parse_args(["nart", glass_scene.path, "out", "-w", "48", "-h", "32", "-s", "4"])
    p = nart_amd.load_sessions(glass_scene.path, p)[0]
    rr = nart_amd.HipRenderer(glass_scene)
    api = rr.render_guides(p)  # the defaults: max_follow 8
    api["denoised"] = rr.denoise(p, api["beauty"], api["albedo"], api["normal"])
    to_half = nart_amd.scene_lib().nart_float_to_half
    for name in ("albedo", "normal", "denoised"):
        halves, _hdr = exr_py.read_rgba_halves(str(out_dir / ("out.%s.exr" % name)))
        final = nart_amd.finalize(p, api[name])
        want = np.array([to_half(ctypes.c_float(v)) for v in final.reshape(-1)], np.uint16).reshape(final.shape)
        assert halves.shape == (32, 48, 4) and np.array_equal(halves, want), name
    # --denoise alone goes through the on-device call: the same image; N selects the limit
    only_dir = tmp_path / "only"
    only_dir.mkdir()
    assert run(str(only_dir / "out"), ["--denoise", "--follow-specular", "8"]).returncode == 0
    assert sorted(os.listdir(only_dir)) == ["out.denoised.exr", "out.exr"]
    assert (only_dir / "out.denoised.exr").read_bytes() == (out_dir / "out.denoised.exr").read_bytes()
    zero_dir = tmp_path / "zero"
    zero_dir.mkdir()
    assert run(str(zero_dir / "out"), ["--aovs", "--follow-specular", "0"]).returncode == 0
    assert (zero_dir / "out.normal.exr").read_bytes() == (first_dir / "out.normal.exr").read_bytes()
    # refused combinations: before any rendering, with a message
    for extra in (["--follow-specular"], ["--aovs", "--follow-specular", "--adaptive", "0.1"],
                  ["--follow-specular", "--robust"], ["--aovs", "--follow-specular", "--mattes"],
                  ["--aovs", "--follow-specular", "11"], ["--aovs", "--follow-specular", "2.5"]):
        bad = run(str(tmp_path / "bad"), extra)
        assert bad.returncode != 0 and "--follow-specular" in bad.stderr, (extra, bad.stderr)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("bad")]


# ---------------------------------------------------------------- 8. errors
def test_guide_errors_leave_contexts_usable(gpu, glass_scene, volume_scenes):
    vol = volume_scenes["c5"]
    pv = _params(vol, 32, 24, 2)
    rv = nart_amd.HipRenderer(vol)
    for call in (lambda: rv.render_guides(pv), lambda: rv.render_guide_samples(pv, 0, 0, 4, 4),
                 lambda: rv.render_denoised(pv, guides=GuideParams.defaults()),
                 lambda: rv.render_guides(pv, albedo=False, beauty=False)):
        with pytest.raises(nart_amd.NartError) as e:
            call()
        assert e.value.code == -6 and "followed guides need surfaces" in str(e.value)  # NART_E_UNSUPPORTED
    assert _bits_equal(rv.render(pv), oracle.Oracle(vol).render(pv))

    p = _params(glass_scene, 32, 24, 2)
    g = nart_amd.session_geometry(p)
    r = nart_amd.HipRenderer(glass_scene)
    assert GuideParams.defaults().max_follow == 8
    deep = GuideParams(max_follow=11)
    for call in (lambda: r.render_guides(p, deep), lambda: r.render_guide_samples(p, 0, 0, 4, 4, deep),
                 lambda: r.render_denoised(p, guides=deep)):
        with pytest.raises(nart_amd.NartError) as e:
            call()
        assert e.value.code == -1 and "max_follow" in str(e.value)  # NART_E_INVALID
    lib = nart_amd.hip_lib()
    img = np.zeros((g.total_height, g.total_width, 5), np.float32)
    A = nart_amd.api
    d = img.ctypes.data
    bad = [(A.AOV_ALBEDO | A.AOV_NORMAL, d, d, None, None),  # normal bit, no buffer
           (A.AOV_ALBEDO, d, None, d, None),                 # albedo bit, no buffer
           (0x4, d, d, d, None),                             # a bit outside the mask
           (0, None, None, None, None)]                      # nothing requested
    for mask, beauty, albedo, normal, moment in bad:
        rc = lib.nart_hip_render_guides(r._ctx, ctypes.byref(p), None, mask, beauty, albedo, normal, moment, None, None)
        assert rc == -1, (mask, rc)
    assert lib.nart_hip_render_guides(None, ctypes.byref(p), None, 1, d, d, None, None, None, None) == -1
    assert lib.nart_hip_render_denoised_guides(r._ctx, ctypes.byref(p), None, None, 0, None, None, None, None) == -1
    assert lib.nart_hip_render_guide_samples(r._ctx, ctypes.byref(p), None, 0, 0, 4, 4, None, None, None, None) == -1
    out8 = np.zeros((4, 4, 2, 8), np.float32)
    for rect in ((0, 0, 0, 4), (g.total_width - 2, 0, 4, 4)):  # empty, out of range
        assert lib.nart_hip_render_guide_samples(r._ctx, ctypes.byref(p), None, *rect, out8.ctypes.data, None, None,
                                                 None) == -1
    # the sample-variance mode's own error, and the denoiser's
    p1 = _params(glass_scene, 32, 24, 1)
    with pytest.raises(nart_amd.NartError) as e:
        r.render_denoised(p1, sample_variance=True, guides=GuideParams.defaults())
    assert e.value.code == -1
    with pytest.raises(nart_amd.NartError) as e:
        r.render_denoised(p, nart_amd.DenoiseParams.defaults(iterations=9), guides=GuideParams.defaults())
    assert e.value.code == -1
    # the existing entry points reject what they rejected
    assert lib.nart_hip_render_aovs(r._ctx, ctypes.byref(p), 0x4, d, d, d, None, None) == -1
    # seg8, tri and n_seg are optional
    assert lib.nart_hip_render_guide_samples(r._ctx, ctypes.byref(p), None, 8, 8, 4, 4, out8.ctypes.data, None, None,
                                             None) == 0
    assert _bits_equal(out8, r.render_guide_samples(p, 8, 8, 4, 4)["rec"])
    assert _bits_equal(r.render(p), oracle.Oracle(glass_scene).render(p))
