"""One long-lived context against a fresh context per step, bit for bit (as uint32).

A context's device buffers only grow and are owned by the context (csrc/host/device_buf.h): a step
that follows a larger one runs in buffers it did not size, a step that follows a failed allocation
must allocate again, and the entry points that take temporaries of their own must give them back.
Nothing here is compared with the oracle: the suite already pins fresh contexts to it at these sizes
(test_gpu_parity.py, test_gpu_build_matrix.py; test_gpu_robustness.py
test_failed_allocation_then_render is the failing render of step 4 on a context of its own)."""
import contextlib

import numpy as np
import pytest

import nart_amd
from nart_amd import scenes

pytestmark = pytest.mark.gpu


def _params(scene, w, h, spp, **kw):
    p = nart_amd.load_sessions(scene.path)[0]
    p.image_width, p.image_height, p.spp = w, h, spp
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _same(got, want):
    """Images, or dicts of images (the device times in them differ from run to run)."""
    if isinstance(want, dict):
        images = sorted(k for k, v in want.items() if isinstance(v, np.ndarray))
        assert images and images == sorted(k for k, v in got.items() if isinstance(v, np.ndarray))
        return all(_same(got[k], want[k]) for k in images)
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _fresh(scene, call, **kw):
    with contextlib.closing(nart_amd.HipRenderer(scene, **kw)) as r:
        return call(r)


def test_one_context_through_growth_failure_and_every_frame_kind(gpu, glass_scene):
    """glassSphere, bucket_size 16: 32x32x2, 80x48x4 (the slot, sample and bucket groups grow), 32x32x2
    again (nothing shrinks: a stale pointer would show), a render that fails with NART_E_OOM, 32x32x2
    right after it, then one call each of the entry points with buffers of their own, and a plain
    render after them."""
    small = _params(glass_scene, 32, 32, 2, bucket_size=16)
    large = _params(glass_scene, 80, 48, 4, bucket_size=16)
    four = _params(glass_scene, 32, 32, 4, bucket_size=16)
    want_small = _fresh(glass_scene, lambda r: r.render(small))
    calls = [("render_aovs", lambda r: r.render_aovs(four)), ("render_denoised", lambda r: r.render_denoised(four)),
             ("render_cascade", lambda r: r.render_robust(four, with_beauty=True, with_layers=True)),
             ("render_mattes", lambda r: r.render_mattes(four, with_beauty=True, with_planes=True)),
             ("render_adaptive", lambda r: r.render_adaptive(four, nart_amd.AdaptiveParams.defaults(min_spp=2, growth=2)))]
    with contextlib.closing(nart_amd.HipRenderer(glass_scene)) as r:
        assert _same(r.render(small), want_small)
        assert _same(r.render(large), _fresh(glass_scene, lambda f: f.render(large)))
        assert _same(r.render(small), want_small)
        with pytest.raises(nart_amd.NartError) as e:
            r.render(_params(glass_scene, 16, 16, 70_000_000))  # 430 GB of per-sample buffers
        assert e.value.code == -4, e.value  # NART_E_OOM
        assert "hipMalloc" in str(e.value) and " B): " in str(e.value), e.value
        assert _same(r.render(small), want_small)
        for name, call in calls:
            assert _same(call(r), _fresh(glass_scene, call)), name
        assert _same(r.render(small), want_small)


def test_queue_buffers_grow(gpu, materials_scene):
    """materials at 432x300 and then 496x312, 1 spp: the smallest queued frames of
    test_gpu_build_matrix.py; the second needs a longer queue, cost list and sort scratch."""
    a, b = _params(materials_scene, 432, 300, 1), _params(materials_scene, 496, 312, 1)
    with contextlib.closing(nart_amd.HipRenderer(materials_scene)) as r:
        sa, sb = nart_amd.RenderStats(), nart_amd.RenderStats()
        got_a, got_b = r.render(a, sa), r.render(b, sb)
    assert "probe_queue" in sa.schedule_names() and "probe_queue" in sb.schedule_names(), (sa.schedule_names(),
                                                                                           sb.schedule_names())
    assert _same(got_a, _fresh(materials_scene, lambda f: f.render(a)))
    assert _same(got_b, _fresh(materials_scene, lambda f: f.render(b)))


def test_dielectric_list_columns_grow(gpu, tmp_path):
    """nested glass, 32x32: bounces 4 keeps the dielectric list in registers, bounces 16 after it
    allocates the per-thread columns on a context that has rendered."""
    scene = nart_amd.Scene(scenes.nested_glass(str(tmp_path), spp=2, bounces=16))
    shallow, deep = _params(scene, 32, 32, 2, bounces=4), _params(scene, 32, 32, 2, bounces=16)
    with contextlib.closing(nart_amd.HipRenderer(scene)) as r:
        got = [r.render(shallow), r.render(deep), r.render(shallow)]
    want = [_fresh(scene, lambda f: f.render(shallow)), _fresh(scene, lambda f: f.render(deep))]
    assert _same(got[0], want[0]) and _same(got[1], want[1]) and _same(got[2], want[0])


def test_multi_device_tiles_given_back_and_regrown(gpu, glass_scene):
    """Two sub-contexts on one ordinal (as test_gpu_multi.py builds them): a cascade frame grows the
    gathered and per-device tiles to nine outputs and gives the growth back when it returns, the
    render after it allocates them again for one output, and a second cascade equals the first."""
    p = _params(glass_scene, 32, 32, 4, bucket_size=16)
    cascade = lambda r: r.render_robust(p, with_beauty=True, with_layers=True)
    with contextlib.closing(nart_amd.HipRenderer(glass_scene, devices=[0, 0])) as m:
        first, plain, second = cascade(m), m.render(p), cascade(m)
    assert _same(second, first)
    assert _same(first, _fresh(glass_scene, cascade))
    assert _same(plain, first["beauty"])
