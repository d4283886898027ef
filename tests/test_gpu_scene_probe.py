"""The scene-bound device functions on chosen records (nart_hip_scene_eval) against the CPU restatement of the
same functions (oracle.scene_eval): tex_fetch, env_ptn_pdf, light_li / light_bound / light_sample_li,
create_bsdf, dg_lookup / dg_lookup2 and medium_sample_ray / maj_next, bit for bit on every output word, for
every scene of scene_probe_cases.py and every build of the path kernels the scene fits.  No tolerance (DESIGN.md,
"Probing the scene-bound functions").  test_scene_probe_cases.py shows on the CPU that the records reach every
class of trouble; a record for which the reference would read outside one of its tables (oracle.SCENE_OOB) is
never sent to the device.
"""
import ctypes

import numpy as np
import pytest

import nart_amd
import scene_probe_cases as sp

pytestmark = pytest.mark.gpu

f32 = np.float32
BUILD_OPS = ("light_li", "light_bound", "light_sample_li", "create_bsdf")  # the ops compiled per (ENV, feature mask)


@pytest.fixture(scope="module")
def scene_dir(gpu, tmp_path_factory):
    return str(tmp_path_factory.mktemp("scene_probe"))


_CTX = {}


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    """The contexts _context made live as long as this module's tests."""
    yield
    for r in _CTX.values():
        r.close()
    _CTX.clear()


def _context(name, scene_dir):
    """(prepared scene, its context), made once per module (closed by _close_contexts)."""
    prep = sp.prepared(name, scene_dir)
    if name not in _CTX:
        _CTX[name] = nart_amd.HipRenderer(prep["scene"])
    return prep, _CTX[name]


def _builds(prep):
    f = nart_amd.api.scene_features(prep["scene"])
    return nart_amd.scene_builds_fitting(f, bool(f & nart_amd.api.FEATURES["environment"]))


def _sent(op, p):
    return np.nonzero(sp.sendable(p) & ~sp.set_aside(op, p))[0]


def _same(a, b):
    """Bit for bit, a NaN equal to any NaN (one device, so the payloads agree too, but the claim is the value)."""
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("name", sp.SCENES)
def test_device_matches_oracle(scene_dir, name):
    prep, r = _context(name, scene_dir)
    builds = _builds(prep)
    assert "env_all" in builds
    failures = []
    for op, p in prep["ops"].items():
        idx = _sent(op, p)
        for build in (builds if op in BUILD_OPS else builds[:1]):
            got = np.zeros_like(p["want"])
            got[idx] = r.scene_eval(op, p["x"][idx], build)
            bad = np.intersect1d(sp.compare(op, got, p["want"]), idx)
            print("%s %s %s: %d records, %d differ" % (name, op, build, len(idx), len(bad)))
            if len(bad):
                failures.append("build %s, %s" % (build, sp.describe(op, p, got, bad)))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name", sp.SCENES)
def test_device_identities(scene_dir, name):
    """On the device alone: light_bound's tMax is light_li's; light_li with theta_in = the device's acosf(wi.z)
    equals light_li that forms it; every narrow build equals the generic one; the three density look-ups agree."""
    prep, r = _context(name, scene_dir)
    builds = _builds(prep)
    ops = prep["ops"]
    lights = prep["scene"].lights()
    if "light_li" in ops:
        p = ops["light_li"]
        idx = _sent("light_li", p)
        x = p["x"][idx]
        base = {b: r.scene_eval("light_li", x, b) for b in builds}
        for b in builds:
            bound = r.scene_eval("light_bound", x, b)
            assert np.all(_same(bound[:, 4], base[b][:, 4])), b
            assert np.all(_same(base[b], base[builds[0]])), b
        env = np.array([lights[k].type == nart_amd.api.LIGHT_ENVIRONMENT for k in x[:, 0].view(np.uint32)])
        if env.any():
            z = np.zeros((int(env.sum()), nart_amd.EVAL_WORDS), f32)
            z[:, 0] = x[env, 6]
            xt = x[env].copy()
            xt[:, 8] = r.eval("acosf", z)[:, 0]
            # (where |wi.z| > 1 the device's acosf is NaN, which asks the function to form it: the same call)
            assert (~np.isnan(xt[:, 8])).sum() >= 6000
            for b in builds:
                if nart_amd.SCENE_BUILD_MASKS[b][0]:
                    assert np.all(_same(r.scene_eval("light_li", xt, b), base[b][env])), b
    for op in ("light_sample_li", "create_bsdf"):
        if op in ops and len(builds) > 1:
            x = ops[op]["x"][_sent(op, ops[op])]
            base = r.scene_eval(op, x, builds[0])
            for b in builds[1:]:
                assert np.all(_same(r.scene_eval(op, x, b), base)), (op, b)
    if "dg_lookup" in ops:
        got = r.scene_eval("dg_lookup", ops["dg_lookup"]["x"][_sent("dg_lookup", ops["dg_lookup"])])
        assert np.all(_same(got[:, 0], got[:, 1]))
        two = got[:, 3].view(np.uint32) == 1
        assert two.all() == (prep["scene"].medium()["res"] == (2, 2, 2)) and two.all() == two.any()
        assert np.all(_same(got[two, 2], got[two, 0])) and not got[~two, 2].view(np.uint32).any()


@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("name,op", [("lights", "light_li"), ("materials", "create_bsdf"), ("med_223_two", "medium_walk")])
def test_record_count_off_the_block_size(scene_dir, name, op, n):
    """Exactly n records come back when n is no multiple of the block; the rest of the caller's buffer is not written."""
    prep, r = _context(name, scene_dir)
    p = prep["ops"][op]
    idx = np.random.default_rng(11).permutation(_sent(op, p))[:n + 300]
    x, want = np.ascontiguousarray(p["x"][idx]), p["want"][idx]
    got = r.scene_eval(op, x[:n])
    assert got.shape == (n, nart_amd.SCENE_OUT_WORDS) and len(sp.compare(op, got, want[:n])) == 0
    buf = np.full((n + 300, nart_amd.SCENE_OUT_WORDS), 0xA5A5A5A5, np.uint32)
    assert nart_amd.hip_lib().nart_hip_scene_eval(r._ctx, nart_amd.SCENE_OPS[op], 0, x.ctypes.data, n, buf.ctypes.data) == 0
    assert len(sp.compare(op, buf[:n].view(f32), want[:n])) == 0
    assert np.all(buf[n:] == 0xA5A5A5A5)


def test_multi_device_context_answers_as_one_device(scene_dir):
    for name, op in (("lights", "light_sample_li"), ("med_435_none", "dg_lookup")):
        prep, r = _context(name, scene_dir)
        m = nart_amd.HipRenderer(prep["scene"], devices=[0, 0])
        try:
            x = prep["ops"][op]["x"][_sent(op, prep["ops"][op])][::7]
            assert np.array_equal(m.scene_eval(op, x).view(np.uint32), r.scene_eval(op, x).view(np.uint32)), name
        finally:
            m.close()


def test_argument_validation_on_a_live_context(scene_dir):
    prep, r = _context("lights", scene_dir)
    lib, P, O, B = nart_amd.hip_lib(), ctypes.c_void_p, nart_amd.SCENE_OPS, nart_amd.SCENE_BUILDS
    p = prep["ops"]["light_li"]
    x = np.ascontiguousarray(p["x"][_sent("light_li", p)][:4])
    y = np.full((4, nart_amd.SCENE_OUT_WORDS), 3.0, f32)
    ev = lambda ctx, op, b, i, n, o: lib.nart_hip_scene_eval(ctx, op, b, i, n, o)  # noqa: E731
    assert ev(r._ctx, O["light_li"], 0, x.ctypes.data, 0, y.ctypes.data) == 0 and np.all(y == 3.0)
    assert ev(P(), O["light_li"], 0, x.ctypes.data, 4, y.ctypes.data) == -1
    assert ev(r._ctx, O["light_li"], 0, P(), 4, y.ctypes.data) == -1
    assert ev(r._ctx, O["light_li"], 0, x.ctypes.data, 4, P()) == -1
    for bad_op in (len(O), 0xFFFFFFFF):
        assert ev(r._ctx, bad_op, 0, x.ctypes.data, 4, y.ctypes.data) == -1
    for bad_build in (len(B), 0xFFFFFFFF):
        assert ev(r._ctx, O["light_li"], bad_build, x.ctypes.data, 4, y.ctypes.data) == -1
    for n in ((1 << 24) + 1, 0xFFFFFFFF):
        assert ev(r._ctx, O["light_li"], 0, x.ctypes.data, n, y.ctypes.data) == -1
    # builds the scene does not fit (ring lights, an environment light, textures), with and without records
    for b in ("all", "diffuse", "glass", "envtex"):
        for n in (0, 4):
            assert ev(r._ctx, O["light_li"], B[b], x.ctypes.data, n, y.ctypes.data) == -1, b
    # no medium
    for op in ("dg_lookup", "medium_walk"):
        assert ev(r._ctx, O[op], 0, x.ctypes.data, 4, y.ctypes.data) == -1
    # an index outside the scene, in any record
    counts = prep["scene"].counts()
    for op, count in (("tex_fetch", counts["textures"]), ("env_pdf", counts["lights"]), ("light_li", counts["lights"]),
                      ("light_bound", counts["lights"]), ("light_sample_li", counts["lights"]), ("create_bsdf", counts["materials"])):
        for v in (count, 0xFFFFFFFF):
            bad = x.copy()
            bad[:, 0] = np.zeros(4, np.uint32).view(f32)
            bad[:, 1:] = 0.25
            bad[2, 0] = np.uint32(v).view(f32)
            assert ev(r._ctx, O[op], 0, bad.ctypes.data, 4, y.ctypes.data) == -1, (op, v)
    env = next(i for i, L in enumerate(prep["scene"].lights()) if L.type == nart_amd.api.LIGHT_ENVIRONMENT and L.Le.type == 1)
    q = sp.records(4)
    q[:, 1:3] = 0.25
    assert ev(r._ctx, O["env_pdf"], 0, q.ctypes.data, 4, y.ctypes.data) == -1  # light 0 is a disk
    q[:, 0] = sp.u32(np.full(4, env))
    # a cell or more below 0: off the distribution (-inf is not: the x86 conversion the reference runs gives cell 0)
    for word, v in ((1, -0.5), (2, -1.0), (1, -1e6)):
        bad = q.copy()
        bad[3, word] = v
        assert ev(r._ctx, O["env_pdf"], 0, bad.ctypes.data, 4, y.ctypes.data) == -1, (word, v)
    for word, v in ((4, -1e-8), (5, 1.0000001), (4, np.nan), (5, np.inf)):  # a sample outside [0, 1]
        bad = q.copy()
        bad[1, word] = v
        assert ev(r._ctx, O["light_sample_li"], 0, bad.ctypes.data, 4, y.ctypes.data) == -1, (word, v)
    assert np.all(y == 3.0)
    assert ev(r._ctx, O["env_pdf"], 0, q.ctypes.data, 4, y.ctypes.data) == 0 and not np.all(y == 3.0)
    with pytest.raises(ValueError):
        r.scene_eval("light_li", np.zeros((4, 8), f32))
    # a narrow build on a scene that fits it, and the generic build without the environment code on the same scene
    prep, r = _context("mat_diffuse", scene_dir)
    p = prep["ops"]["light_li"]
    x = np.ascontiguousarray(p["x"][_sent("light_li", p)][:4])
    for b in ("env_all", "all", "diffuse", "glass"):
        assert ev(r._ctx, O["light_li"], B[b], x.ctypes.data, 4, y.ctypes.data) == 0, b
    assert ev(r._ctx, O["light_li"], B["envtex"], x.ctypes.data, 4, y.ctypes.data) == -1
