"""The whole-frame entry points of the C ABI (nart_hip_render, _render_aovs, _render_device,
_render_denoised) run one frame path (render_frame, render.hip): whatever the entry point, the
device list or the batch split, a buffer has the bits of the single-batch single-device render()
/ render_aovs() of the same parameters (whose oracle parity tests/test_gpu_parity.py and
tests/test_gpu_aovs.py hold).  Also the statistics' meaning on several devices, and the rect check
of the per-sample entry points."""
import ctypes

import numpy as np
import pytest

import nart_amd

pytestmark = pytest.mark.gpu


def _params(scene, w, h, spp):
    p = nart_amd.load_sessions(scene.path)[0]
    p.image_width, p.image_height, p.spp = w, h, spp
    p.bucket_size, p.bounces = 16, 3
    return p


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32),
                          np.ascontiguousarray(b, np.float32).view(np.uint32))


def _device_image(p, dptr):
    """The (totalH, totalW, 5) image at device address dptr, read back through a torch tensor."""
    import torch
    g = nart_amd.session_geometry(p)
    t = torch.empty((g.total_height, g.total_width, 5), dtype=torch.float32, device="cuda:0")
    rc = ctypes.CDLL("libamdhip64.so").hipMemcpy(ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(dptr),
                                                 ctypes.c_size_t(t.numel() * 4), ctypes.c_int(3))  # device to device
    assert rc == 0, rc
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def frame(gpu, glass_scene):
    """40x24 in 16-pixel buckets (3x2, partial buckets on both edges), 2 spp: the parameters, and the
    single-device single-batch images every case compares with (read-only)."""
    p = _params(glass_scene, 40, 24, 2)
    g = nart_amd.session_geometry(p)
    assert (g.n_buckets_x, g.n_buckets_y) == (3, 2)
    r = nart_amd.HipRenderer(glass_scene)
    st = nart_amd.RenderStats()
    ref = r.render_aovs(p)
    ref["plain"] = r.render(p, st)
    ref["denoised"] = r.denoise(p, ref["beauty"], ref["albedo"], ref["normal"])
    r.close()
    assert st.kernel_launches == 1  # one batch
    assert _bits_equal(ref["plain"], ref["beauty"])
    return p, ref, st


def _check_every_entry_point(r, p, ref):
    assert _bits_equal(r.render(p), ref["plain"]), "render"
    assert _bits_equal(_device_image(p, r.render_device(p)), ref["plain"]), "render_device"
    aov = r.render_aovs(p)
    for name in ("beauty", "albedo", "normal"):
        assert _bits_equal(aov[name], ref[name]), ("render_aovs", name)
    dn = r.render_denoised(p, beauty=True)
    assert _bits_equal(dn["beauty"], ref["plain"]), "render_denoised beauty"
    # the filter's inputs were render_aovs' images: denoise() over those gives the same output
    assert _bits_equal(dn["denoised"], ref["denoised"]), "render_denoised"
    assert _bits_equal(r.denoise(p, aov["beauty"], aov["albedo"], aov["normal"]), dn["denoised"])


@pytest.mark.parametrize("devices", [None, [0, 0, 0]], ids=["one-device", "3-rehearsal"])
def test_every_entry_point_same_frame(frame, glass_scene, devices):
    """Case 1: one device, and three ranks of two buckets each."""
    p, ref, _st = frame
    r = nart_amd.HipRenderer(glass_scene, devices=devices)
    _check_every_entry_point(r, p, ref)
    # and again in another order: the cached buffers of one entry point do not leak into the next
    assert _bits_equal(r.render_denoised(p)["denoised"], ref["denoised"])
    assert _bits_equal(_device_image(p, r.render_device(p)), ref["plain"])
    r.close()


def test_batches_with_aov_slabs(frame, glass_scene, monkeypatch):
    """Case 2: NART_BATCH_BYTES=1 leaves 256 slots, one 16x16 bucket per batch, so every batch
    writes at its own offset into the three back-to-back tile slabs."""
    p, ref, _st = frame
    monkeypatch.setenv("NART_BATCH_BYTES", "1")
    r = nart_amd.HipRenderer(glass_scene)
    st = nart_amd.RenderStats()
    aov = r.render_aovs(p, stats=st)
    assert st.kernel_launches == 6
    for name in ("beauty", "albedo", "normal"):
        assert _bits_equal(aov[name], ref[name]), name
    st2 = nart_amd.RenderStats()
    dn = r.render_denoised(p, stats=st2)
    assert st2.kernel_launches == 6
    assert _bits_equal(dn["beauty"], ref["plain"]) and _bits_equal(dn["denoised"], ref["denoised"])
    r.close()


def test_rank_without_buckets(gpu, glass_scene):
    """Case 3: two buckets on three ranks."""
    p = _params(glass_scene, 24, 16, 2)
    g = nart_amd.session_geometry(p)
    assert g.n_buckets_x * g.n_buckets_y == 2
    single = nart_amd.HipRenderer(glass_scene)
    ref = single.render_aovs(p)
    single.close()
    m = nart_amd.HipRenderer(glass_scene, devices=[0, 0, 0])
    got = m.render_aovs(p)
    for name in ("beauty", "albedo", "normal"):
        assert _bits_equal(got[name], ref[name]), name
    only = m.render_aovs(p, beauty=False)
    assert "beauty" not in only
    assert _bits_equal(only["albedo"], ref["albedo"]) and _bits_equal(only["normal"], ref["normal"])
    m.close()


def test_stats_keep_their_meaning(frame, glass_scene):
    """Case 4: work counts and schedule of two ranks equal the single device's; a RenderStats
    reused over two renders holds twice the counts."""
    p, _ref, st1 = frame
    m = nart_amd.HipRenderer(glass_scene, devices=[0, 0])
    st = nart_amd.RenderStats()
    m.render(p, st)
    print("single:", st1.as_dict(), "\ntwo ranks:", st.as_dict())
    assert (st.samples, st.traced_samples, st.schedule) == (st1.samples, st1.traced_samples, st1.schedule)
    assert st.samples == 40 * 24 * 2
    once = (st.samples, st.traced_samples, st.kernel_launches)
    m.render(p, st)
    assert (st.samples, st.traced_samples, st.kernel_launches) == tuple(2 * c for c in once)
    m.close()


def test_wrapping_rect_is_rejected(frame, glass_scene):
    """Case 5: x0 + w wraps to 1 in 32 bits; both per-sample entry points refuse the rect on the
    host (NART_E_INVALID), and the context renders as before."""
    p, ref, _st = frame
    r = nart_amd.HipRenderer(glass_scene)
    before = r.render(p)
    for call in (r.render_samples, r.render_aov_samples):
        with pytest.raises(nart_amd.NartError) as e:
            call(p, 0xFFFFFFFF, 0, 2, 1)
        assert e.value.code == -1, call  # NART_E_INVALID
        with pytest.raises(nart_amd.NartError) as e:
            call(p, 0, 0xFFFFFFFF, 1, 2)
        assert e.value.code == -1, call
    after = r.render(p)
    assert _bits_equal(after, before) and _bits_equal(after, ref["plain"])
    r.close()


def test_first_device_errors_reach_the_caller(gpu, glass_scene):
    """Case 6: calls that a two-device context forwards to its first device and that fail there, after
    the forward: the per-sample entry points with a rect ending one pixel beyond the total image, and
    denoise with image_width = 0.  The caller's context reports the code and the very message a
    single-device context gives, and both render as before."""
    p = _params(glass_scene, 32, 24, 2)
    g = nart_amd.session_geometry(p)
    one = nart_amd.HipRenderer(glass_scene)
    two = nart_amd.HipRenderer(glass_scene, devices=[0, 0])
    before = one.render(p)
    assert _bits_equal(two.render(p), before)
    empty = p.copy()
    empty.image_width = 0
    ge = nart_amd.session_geometry(empty)
    img = np.zeros((ge.total_height, ge.total_width, 5), np.float32)
    calls = [("render_samples", lambda r: r.render_samples(p, g.total_width - 1, 0, 2, 1)),
             ("render_aov_samples", lambda r: r.render_aov_samples(p, 0, g.total_height - 1, 1, 2)),
             ("render_guide_samples", lambda r: r.render_guide_samples(p, g.total_width - 1, g.total_height - 1, 2, 2)),
             ("denoise", lambda r: r.denoise(empty, img, img, img))]
    for name, call in calls:
        messages = []
        for r in (one, two):
            with pytest.raises(nart_amd.NartError) as e:
                call(r)
            assert e.value.code == -1, name  # NART_E_INVALID
            messages.append(r._lib.nart_hip_last_error(r._ctx).decode())
        print(name, messages)
        assert messages[0] and messages[1] == messages[0], name
    for r in (one, two):
        assert _bits_equal(r.render(p), before)
        r.close()
