"""First-hit AOVs (nart_hip_render_aovs, nart_hip_render_aov_samples, `nart --aovs`) against the
oracle: hit, depth and triangle bit for bit against the reference octree's answer; the AOV images
bit for bit against the numpy restatement of AddSample and the tile combine
(tests/test_aov_restatement.py) over the device's own per-sample records; coverage bit for bit
against the reference's alpha; albedo against the blob's pattern values and texels; the shading
normal against a float64 restatement within a tolerance measured from float32 arithmetic."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import aov_py
import exr_py
import nart_amd
import oracle
from nart_amd import scenes
from test_aov_restatement import restate_render, total_frame_uv

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NART = os.path.join(REPO, "nart_amd", "bin", "nart")
NO_HIT = aov_py.NO_HIT


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


@pytest.fixture(scope="module")
def c4_scene(built, tmp_path_factory):
    return nart_amd.Scene(scenes.c4_teapot(str(tmp_path_factory.mktemp("c4aov")), env_size=(64, 32)))


# Per scene: frame (w, h, spp) and 8x8 blocks in total-image coordinates -- the first on geometry
# (every centre ray hits), the others across silhouettes or material borders.
BLOCKS = {
    "env": ((64, 48, 4), [(22, 16, 8, 8), (16, 10, 8, 8)]),
    "c4": ((64, 48, 4), [(24, 22, 8, 8), (40, 16, 8, 8)]),
    "glass": ((64, 48, 4), [(24, 20, 8, 8), (18, 16, 8, 8)]),
    "cornell": ((64, 36, 4), [(30, 16, 8, 8), (8, 2, 8, 8)]),
    "materials": ((64, 48, 4), [(16, 17, 8, 8), (29, 17, 8, 8), (40, 17, 8, 8), (30, 22, 8, 8)]),
}
_cache = {}


def _scene_of(name, request):
    fixture = {"env": "env_scene", "c4": "c4_scene", "glass": "glass_scene", "cornell": "cornell_scene",
               "materials": "materials_scene"}[name]
    return request.getfixturevalue(fixture)


def _blocks(name, request):
    """The device's per-sample AOV records and the oracle's rays and hits of a scene's blocks,
    computed once and shared (read-only) by the tests."""
    if name not in _cache:
        sc = _scene_of(name, request)
        (w, h, spp), rects = BLOCKS[name]
        p = _params(sc, w, h, spp)
        orc = oracle.Oracle(sc)
        gpu_r = nart_amd.HipRenderer(sc)
        out = []
        for rect in rects:
            rec, tri = gpu_r.render_aov_samples(p, *rect)
            out.append({"rect": rect, "rec": rec, "tri": tri, "ref": aov_py.trace_block(orc, p, *rect)})
        gpu_r.close()
        _cache[name] = (sc, p, orc, out)
    return _cache[name]


# ---------------------------------------------------------------- 1. beauty unchanged
@pytest.mark.parametrize("variant", [0, 3], ids=["rayqueue", "megakernel"])
def test_beauty_unchanged(gpu, glass_scene, variant):
    p = _params(glass_scene, 64, 64, 4)
    r = nart_amd.HipRenderer(glass_scene, variant=variant)
    st0, st1 = nart_amd.RenderStats(), nart_amd.RenderStats()
    plain = r.render(p, st0)
    feat0 = r.scene_features()
    out = r.render_aovs(p, stats=st1)
    ref = oracle.Oracle(glass_scene).render(p)
    assert _bits_equal(out["beauty"], ref), _report(out["beauty"], ref)
    assert _bits_equal(plain, ref)
    assert r.scene_features() == feat0
    assert st1.schedule == st0.schedule and st1.kernel_launches == st0.kernel_launches
    assert out["aov_ms"] > 0.0


# ---------------------------------------------------------------- 2. depth and triangle, exact
@pytest.mark.parametrize("name", ["env", "c4"])
def test_depth_and_triangle_exact(gpu, request, name):
    """Environment-lit scenes (the light's bound never cuts a hit): hit, depth and triangle of
    every sample equal the reference octree's answer."""
    _sc, _p, _orc, blocks = _blocks(name, request)
    centre_hits = []
    for b in blocks:
        rec, tri, ref = b["rec"], b["tri"], b["ref"]
        hit = ref["tri"] >= 0
        centre_hits.append(hit.mean())
        assert np.array_equal(rec[..., 3] == 1.0, hit) and np.all((rec[..., 3] == 1.0) | (rec[..., 3] == 0.0))
        assert np.array_equal(_bits(rec[..., 7])[hit], _bits(ref["t"])[hit])
        assert not rec[~hit].any()  # a miss is all zeros
        assert np.array_equal(tri == NO_HIT, ~hit)
        agree = hit & (ref["tri"] == ref["tri_bf"])
        assert agree.sum() > 0.9 * hit.sum()
        assert np.array_equal(tri[agree].astype(np.int64), ref["tri"][agree])
    # the first block lies on geometry, the second straddles a silhouette
    assert centre_hits[0] == 1.0 and 0.05 < centre_hits[1] < 0.95, centre_hits


def test_depth_with_disk_light(gpu, request):
    """glassSphere (a disk light bounds the camera rays): a device hit has the octree's t; a device
    miss where the unbounded octree query hits is accepted only where the reference's alpha at one
    bounce is 1 (a light was met first)."""
    sc, p, orc, blocks = _blocks("glass", request)
    p1 = _params(sc, p.image_width, p.image_height, p.spp, bounces=1)
    n_hits = 0
    for b in blocks:
        rec, ref = b["rec"], b["ref"]
        dev_hit = rec[..., 3] == 1.0
        n_hits += int(dev_hit.sum())
        assert np.all(ref["tri"][dev_hit] >= 0)
        assert np.array_equal(_bits(rec[..., 7])[dev_hit], _bits(ref["t"])[dev_hit])
        cut = ~dev_hit & (ref["tri"] >= 0)
        if cut.any():
            alpha = orc.render_samples(p1, *b["rect"])[..., 3]
            assert np.all(alpha[cut] == 1.0)
    assert n_hits > 0


# ---------------------------------------------------------------- 3. octree-missed hit
def test_octree_missed_hit_is_a_miss(gpu, cornell_scene):
    """C2 pixel (331, 235), sample 30: the reference octree misses the triangle a brute-force pass
    finds (tests/test_gpu_parity.py test_octree_missed_camera_hit_samples); the AOVs report the
    miss the beauty renders."""
    p = _params(cornell_scene, 1920, 1080, 64, bounces=1)
    rec, tri = nart_amd.HipRenderer(cornell_scene).render_aov_samples(p, 328, 232, 8, 8)
    assert not rec[3, 3, 30].any() and tri[3, 3, 30] == NO_HIT
    assert (rec[..., 3] == 1.0).any()  # the block is not all sky
    orc = oracle.Oracle(cornell_scene)
    g = nart_amd.session_geometry(p)
    uv = oracle.latin_square(235 * g.total_width + 331, p.spp)[0][30]
    o, d = oracle.camera_ray(orc, p.image_width, p.image_height, 331, 235, uv[0], uv[1])
    tr = oracle.trace(orc, o, d)
    assert tr[0] < 0 and tr[2] >= 0  # octree miss, brute-force hit: the case stays meaningful


# ---------------------------------------------------------------- 4. coverage = reference alpha
def _closed_scene(directory):
    """A Lambert sphere over a Lambert floor patch (sky around them: misses) whose one disk light
    lies behind the camera, so that no camera ray meets it: at one bounce the reference's alpha is
    exactly the first-hit mask."""
    os.makedirs(directory, exist_ok=True)
    scenes.write_geo(os.path.join(directory, "ball.geo"), *scenes._uv_sphere((0.0, 0.0, 1.0), 0.7, 16, 32))
    scenes.write_geo(os.path.join(directory, "floor.geo"),
                     *scenes._uv_grid((-1.0, -1.5, 0.2), (2.0, 0, 0), (0, 3.0, 0), (0, 0, 1), 8))
    scene = {
        "renderSessions": [{"imageWidth": 40, "imageHeight": 28, "bucketSize": 16, "spp": 4, "bounces": 1,
                            "filterWidth": 2, "rougheningFactor": 0}],
        "camera": {"fov": 16.5, "transform": [1, 0, 0, 0, 0, 0, -1, -3.9, 0, 1, 0, 1, 0, 0, 0, 1]},
        "meshes": [{"filePath": os.path.join(directory, "ball.geo"),
                    "material": {"type": "lambert", "rho_d": [0.6, 0.3, 0.2]}},
                   {"filePath": os.path.join(directory, "floor.geo"),
                    "material": {"type": "lambert", "rho_d": [0.5, 0.5, 0.5]}}],
        "lights": [{"type": "disk", "radius": 0.5, "Le": [1, 1, 1], "intensity": 20.0,
                    "transform": [1, 0, 0, 0, 0, 1, 0, -6.0, 0, 0, 1, 1.0, 0, 0, 0, 1]}],
    }
    path = os.path.join(directory, "closed.json")
    with open(path, "w") as f:
        json.dump(scene, f, indent=1)
    return path


def test_coverage_equals_reference_alpha(gpu, tmp_path):
    sc = nart_amd.Scene(_closed_scene(str(tmp_path)))
    p = _params(sc, 40, 28, 4, bucket_size=16, bounces=1)
    g = nart_amd.session_geometry(p)
    orc = oracle.Oracle(sc)
    # CPU precondition: alpha at one bounce is the octree's hit mask for every sample of the frame
    ref = aov_py.trace_block(orc, p, 0, 0, g.total_width, g.total_height)
    alpha = orc.render_samples(p, 0, 0, g.total_width, g.total_height)[..., 3]
    mask = ref["tri"] >= 0
    assert np.array_equal(alpha == 1.0, mask) and np.all((alpha == 1.0) | (alpha == 0.0))
    assert 0.1 < mask.mean() < 0.9
    out = nart_amd.HipRenderer(sc).render_aovs(p, normal=False, beauty=False)
    want = orc.render(p)
    assert _bits_equal(out["albedo"][..., 3], want[..., 3]), _report(out["albedo"][..., 3], want[..., 3])
    assert _bits_equal(out["albedo"][..., 4], want[..., 4])


# ---------------------------------------------------------------- 5. splat of AOV records
SPLAT_CONFIGS = {"b16_fw2": dict(bucket_size=16, filter_width=2.0), "b12_fw1": dict(bucket_size=12, filter_width=1.0)}
_restated = {}


def _restated_aovs(glass_scene, cfg):
    """The restatement's albedo and normal images of glassSphere 24x20x2 over the device's
    per-sample records of the whole total frame (the records do not depend on the splat mode)."""
    if cfg not in _restated:
        p = _params(glass_scene, 24, 20, 2, **SPLAT_CONFIGS[cfg])
        g = nart_amd.session_geometry(p)
        rec, _tri = nart_amd.HipRenderer(glass_scene).render_aov_samples(p, 0, 0, g.total_width, g.total_height)
        uv = total_frame_uv(p)
        _restated[cfg] = (p, restate_render(p, uv, np.ascontiguousarray(rec[..., :4])),
                          restate_render(p, uv, np.ascontiguousarray(rec[..., 4:])))
    return _restated[cfg]


@pytest.mark.parametrize("cfg", list(SPLAT_CONFIGS))
@pytest.mark.parametrize("splat_mode", [5, 4, 3, 0], ids=["rows", "skew", "col4", "direct"])
def test_aov_images_equal_restated_splat(gpu, glass_scene, cfg, splat_mode):
    p, albedo, normal = _restated_aovs(glass_scene, cfg)
    assert albedo[..., 3].max() > 0 and np.abs(normal[..., :3]).max() > 0
    out = nart_amd.HipRenderer(glass_scene, splat_mode=splat_mode).render_aovs(p)
    assert _bits_equal(out["albedo"], albedo), _report(out["albedo"], albedo)
    assert _bits_equal(out["normal"], normal), _report(out["normal"], normal)


def test_aov_images_eight_samples_per_pixel(gpu, glass_scene):
    """8 spp: k_aov's eight-samples-per-step path (the other frames of this file have 2 or 4 spp).
    The per-sample entry point and the pixel-major frame (splat mode 5) take it, the sample-major
    frame (splat mode 3) takes the one-sample path; all must agree through the restatement, and the
    records' depth must be the octree's t."""
    p = _params(glass_scene, 24, 20, 8, bucket_size=16)
    g = nart_amd.session_geometry(p)
    rec, _tri = nart_amd.HipRenderer(glass_scene).render_aov_samples(p, 0, 0, g.total_width, g.total_height)
    ref = aov_py.trace_block(oracle.Oracle(glass_scene), p, 10, 8, 8, 8)
    blk = rec[8:16, 10:18]
    hit = blk[..., 3] == 1.0
    assert hit.any() and np.all(ref["tri"][hit] >= 0)
    assert np.array_equal(_bits(blk[..., 7])[hit], _bits(ref["t"])[hit])
    uv = total_frame_uv(p)
    want = {name: restate_render(p, uv, np.ascontiguousarray(rec[..., lo:lo + 4]))
            for name, lo in (("albedo", 0), ("normal", 4))}
    for mode in (5, 3):
        st = nart_amd.RenderStats()
        out = nart_amd.HipRenderer(glass_scene, splat_mode=mode).render_aovs(p, stats=st)
        assert ("splat_rows" in st.schedule_names()) == (mode == 5)  # the pixel-major layout
        for name in want:
            assert _bits_equal(out[name], want[name]), (mode, name, _report(out[name], want[name]))


# ---------------------------------------------------------------- 6. albedo
@pytest.mark.parametrize("name", ["cornell", "materials"])
def test_albedo_constant_patterns(gpu, request, name):
    """Every hit sample on a material whose colour pattern is constant carries that pattern's value,
    by the kind table: triangle -> mesh -> material."""
    sc, _p, _orc, blocks = _blocks(name, request)
    mats, tri_mat = sc.materials(), aov_py.tri_material(sc)
    kinds, checked = set(), 0
    for b in blocks:
        rec, tri = b["rec"], b["tri"]
        for idx in zip(*np.nonzero(tri != NO_HIT)):
            m = mats[tri_mat[tri[idx]]]
            ptn = aov_py.albedo_pattern(m)
            if ptn.type != nart_amd.api.PTN_CONSTANT:
                continue
            assert _bits_equal(rec[idx][:3], np.float32(list(ptn.value))), (idx, m.type)
            kinds.add(m.type)
            checked += 1
    assert checked > 100
    if name == "materials":
        A = nart_amd.api
        assert kinds >= {A.MAT_SPECULAR, A.MAT_GLOSSY, A.MAT_GLASS, A.MAT_PLASTIC}, kinds


def test_albedo_textured(gpu, request):
    """C4 teapot (plastic, rho_d = uv.exr): st recomputed in float64 from the oracle's triangle and
    ray; the albedo is the texel at TexturePattern's index.  Samples whose scaled u or v lies within
    1e-3 of a texel boundary are left out (float32 st may round across it): at most 2 %."""
    sc, _p, _orc, blocks = _blocks("c4", request)
    mats, tri_mat, tris, texs = sc.materials(), aov_py.tri_material(sc), sc.triangles(), sc.textures()
    n_tex = n_left_out = 0
    for b in blocks:
        rec, ref = b["rec"], b["ref"]
        for idx in zip(*np.nonzero(ref["tri"] >= 0)):
            ptn = aov_py.albedo_pattern(mats[tri_mat[ref["tri"][idx]]])
            if ptn.type != nart_amd.api.PTN_TEXTURE:
                continue
            n_tex += 1
            tex = texs[ptn.texture]
            th, tw = tex.shape[:2]
            st = aov_py.surface_st(tris[ref["tri"][idx]], ref["o"][idx], ref["d"][idx], np.float64)
            su = tw * min(max(st[0], 0.0001), 0.9999)       # texturepattern.cpp:172-187
            sv = th * min(max(1.0 - st[1], 0.0001), 0.9999)
            if min(abs(su - round(su)), abs(sv - round(sv))) < 1e-3:
                n_left_out += 1
                continue
            want = tex[int(sv), int(su), :3].view(np.float16).astype(np.float32)
            assert _bits_equal(rec[idx][:3], want), (idx, st)
    assert n_tex > 100 and n_left_out <= 0.02 * n_tex, (n_tex, n_left_out)


# ---------------------------------------------------------------- 7. normal
def _normal_gaps(blocks, tris, select=None):
    """Per hit sample (of the oracle's triangle): the float64 normal, and the largest component gap
    of the float32 restatement (the reference's operation order) from it."""
    out = []
    for b in blocks:
        ref = b["ref"]
        for idx in zip(*np.nonzero(ref["tri"] >= 0)):
            if select is not None and not select(ref["tri"][idx]):
                continue
            T, o, d = tris[ref["tri"][idx]], ref["o"][idx], ref["d"][idx]
            n64 = aov_py.shading_normal(T, o, d, np.float64)
            n32 = aov_py.shading_normal(T, o, d, np.float32)
            assert n32.dtype == np.float32
            out.append((b, idx, n64, float(np.abs(n32.astype(np.float64) - n64).max())))
    return out


@pytest.mark.parametrize("name", ["glass", "cornell"])
def test_normal_matches_float64_restatement(gpu, request, name):
    """Scenes without a normal map: the record's normal against normalize(n0 u + n1 v + n2 w) in
    float64 for the oracle's triangle.  Tolerance: 4x the largest gap, over these same samples, of a
    float32 numpy restatement in fill_isect's operation order from the float64 one (the factor
    covers the device's normalise sequence, which differs from numpy's by the rounding of 1/sqrt).
    Measured on the CPU over these blocks: glassSphere gap 2.19e-06 (tolerance 8.74e-06; the
    backdrop's interpolated normals are far from unit length before the normalise), Cornell gap
    8.86e-08 (tolerance 3.55e-07).  The test computes the gap itself, so the figures follow the
    blocks."""
    sc, _p, _orc, blocks = _blocks(name, request)
    gaps = _normal_gaps(blocks, sc.triangles())
    gap = max(g for *_x, g in gaps)
    tol = 4.0 * gap
    print("normal gap float32 vs float64 on %s: %.3g, tolerance %.3g, %d samples" % (name, gap, tol, len(gaps)))
    worst = 0.0
    for b, idx, n64, _g in gaps:
        if b["rec"][idx][3] != 1.0:
            continue  # cut by the disk light (test_depth_with_disk_light)
        worst = max(worst, float(np.abs(b["rec"][idx][4:7].astype(np.float64) - n64).max()))
    print("device normal vs float64: %.3g" % worst)
    assert len(gaps) > 100 and worst <= tol, (worst, tol)


def test_normal_with_normal_map(gpu, request):
    """C4 teapot (normal-mapped plastic): unit length within the tolerance above, measured on these
    samples (float32-to-float64 gap of the unmapped normal 1.28e-07, tolerance 5.12e-07), and
    different from the unmapped normal somewhere."""
    sc, _p, _orc, blocks = _blocks("c4", request)
    mats, tri_mat = sc.materials(), aov_py.tri_material(sc)
    gaps = _normal_gaps(blocks, sc.triangles(), select=lambda t: mats[tri_mat[t]].has_normal)
    tol = 4.0 * max(g for *_x, g in gaps)
    differs = 0.0
    for b, idx, n64, _g in gaps:
        n = b["rec"][idx][4:7].astype(np.float64)
        assert abs(np.sqrt((n * n).sum()) - 1.0) <= tol, (idx, n)
        differs = max(differs, float(np.abs(n - n64).max()))
    assert len(gaps) > 100 and differs > 1e-2, differs


# ---------------------------------------------------------------- 8. multi-device
@pytest.mark.parametrize("mode", ["copy-rehearsal", "rccl-one-device"])
def test_multi_device_aovs_match_single(gpu, glass_scene, monkeypatch, mode):
    p = _params(glass_scene, 64, 48, 4)
    single = nart_amd.HipRenderer(glass_scene).render_aovs(p)
    if mode == "rccl-one-device":
        monkeypatch.setenv("NART_GATHER", "rccl")
        m = nart_amd.HipRenderer(glass_scene, devices=[0])
        assert m.devices() == (1, True)
    else:
        m = nart_amd.HipRenderer(glass_scene, devices=[0, 0])
        assert m.devices() == (2, False)
    got = m.render_aovs(p)
    for name in ("beauty", "albedo", "normal"):
        assert _bits_equal(got[name], single[name]), (name, _report(got[name], single[name]))
    only = m.render_aovs(p, beauty=False)
    assert "beauty" not in only and _bits_equal(only["normal"], single["normal"])
    assert _bits_equal(m.render(p), single["beauty"])


# ---------------------------------------------------------------- 9. errors
def test_aov_errors_leave_contexts_usable(gpu, glass_scene, volume_scenes):
    vol = volume_scenes["c5"]
    pv = _params(vol, 32, 24, 2)
    rv = nart_amd.HipRenderer(vol)
    with pytest.raises(nart_amd.NartError) as e:
        rv.render_aovs(pv)
    assert e.value.code == -6 and "volume" in str(e.value)  # NART_E_UNSUPPORTED
    with pytest.raises(nart_amd.NartError) as e:
        rv.render_aov_samples(pv, 0, 0, 4, 4)
    assert e.value.code == -6
    assert _bits_equal(rv.render(pv), oracle.Oracle(vol).render(pv))

    p = _params(glass_scene, 32, 24, 2)
    g = nart_amd.session_geometry(p)
    r = nart_amd.HipRenderer(glass_scene)
    lib = nart_amd.hip_lib()
    img = np.zeros((g.total_height, g.total_width, 5), np.float32)
    A = nart_amd.api
    bad = [(A.AOV_ALBEDO | A.AOV_NORMAL, img.ctypes.data, img.ctypes.data, None),  # normal bit, no buffer
           (A.AOV_ALBEDO, img.ctypes.data, None, img.ctypes.data),                 # albedo bit, no buffer
           (0x4, img.ctypes.data, img.ctypes.data, img.ctypes.data),               # bit outside the mask
           (0, None, None, None)]                                                  # nothing requested
    for mask, beauty, albedo, normal in bad:
        rc = lib.nart_hip_render_aovs(r._ctx, ctypes.byref(p), mask, beauty, albedo, normal, None, None)
        assert rc == -1, (mask, rc)  # NART_E_INVALID
    assert _bits_equal(r.render(p), oracle.Oracle(glass_scene).render(p))


# ---------------------------------------------------------------- 10. AOV-only
def test_aov_only_render(gpu, glass_scene):
    p, albedo, normal = _restated_aovs(glass_scene, "b16_fw2")
    r = nart_amd.HipRenderer(glass_scene)
    st = nart_amd.RenderStats()
    out = r.render_aovs(p, beauty=False, stats=st)
    assert "beauty" not in out
    assert _bits_equal(out["albedo"], albedo) and _bits_equal(out["normal"], normal)
    assert st.kernel_launches == 0 and st.traced_samples > 0
    one = r.render_aovs(p, albedo=False, beauty=False)
    assert set(one) == {"normal", "aov_ms"} and _bits_equal(one["normal"], normal)
    st2 = nart_amd.RenderStats()
    r.render_aovs(p, stats=st2)
    assert st2.kernel_launches > 0


# ---------------------------------------------------------------- 11. CLI
def test_cli_aovs(gpu, glass_scene, tmp_path):
    def run(out, extra):
        r = subprocess.run([NART, glass_scene.path, out, "-w", "48", "-h", "32", "-s", "4"] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        return r.stdout

    plain_dir, aov_dir = tmp_path / "plain", tmp_path / "aov"
    plain_dir.mkdir()
    aov_dir.mkdir()
    run(str(plain_dir / "out"), [])
    log = run(str(aov_dir / "out"), ["--aovs"])
    assert sorted(os.listdir(plain_dir)) == ["out.exr"]
    assert sorted(os.listdir(aov_dir)) == ["out.albedo.exr", "out.exr", "out.normal.exr"]
    assert (plain_dir / "out.exr").read_bytes() == (aov_dir / "out.exr").read_bytes()
    for name in ("out.exr", "out.albedo.exr", "out.normal.exr"):
        assert ("Writing to %s..." % (aov_dir / name)) in log
    p = nart_amd.parse_args(["nart", glass_scene.path, "out", "-w", "48", "-h", "32", "-s", "4"])
    p = nart_amd.load_sessions(glass_scene.path, p)[0]
    api = nart_amd.HipRenderer(glass_scene).render_aovs(p, beauty=False)
    to_half = nart_amd.scene_lib().nart_float_to_half
    for name in ("albedo", "normal"):
        halves, _hdr = exr_py.read_rgba_halves(str(aov_dir / ("out.%s.exr" % name)))
        final = nart_amd.finalize(p, api[name])
        want = np.array([to_half(ctypes.c_float(v)) for v in final.reshape(-1)], np.uint16).reshape(final.shape)
        assert halves.shape == (32, 48, 4) and np.array_equal(halves, want), name
