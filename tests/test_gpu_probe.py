"""The device functions of dmath.h, path.h and volume.h on chosen inputs (nart_hip_eval), against the
CPU restatement of the same functions (oracle_eval) and the host libm: bit for bit on every output
word where the oracle's value is not NaN, NaN where it is.  No tolerance ("Probing the
device functions").  The inputs are probe_cases.py's grids; test_probe_cases.py shows on the CPU that
they reach every range and outcome class.
"""
import ctypes

import numpy as np
import pytest

import nart_amd
import probe_cases as pc

pytestmark = pytest.mark.gpu

FM_OPS = ("bxdf_f_pdf", "bxdf_sample_f")  # templated on the path kernel's feature mask


@pytest.fixture(scope="module")
def dev(gpu, glass_scene):
    return nart_amd.HipRenderer(glass_scene)


def _check(op, x, got, want):
    idx = pc.compare(op, got, want)
    assert len(idx) == 0, pc.describe(op, x, got, want, idx)


@pytest.mark.parametrize("op", [o for o in nart_amd.EVAL_OPS if o not in FM_OPS])
def test_device_matches_oracle(dev, op):
    x = pc.grid(op)
    _check(op, x, dev.eval(op, x), pc.expected(op))


@pytest.mark.parametrize("mask", list(nart_amd.EVAL_MASKS))
@pytest.mark.parametrize("op", FM_OPS)
def test_device_matches_oracle_per_build(dev, op, mask):
    """bxdf_f_pdf<FM> and bxdf_sample_f<FM>: the generic build on the whole grid, a narrow build on the
    BxDF kinds its mask creates."""
    fm, kinds = nart_amd.EVAL_MASKS[mask]
    keep = np.isin(pc.rec_type(pc.grid(op)), kinds)
    x = pc.grid(op)[keep]
    assert len(x) >= 4096
    _check(op, x, dev.eval(op, x, fm=fm), pc.expected(op)[keep])


@pytest.mark.parametrize("mask", list(nart_amd.EVAL_MASKS))
def test_fused_f_pdf_is_its_two_parts(dev, mask):
    """bxdf_f_pdf against the device's own bxdf_f and bxdf_pdf: every lane computes its branch's values with
    its branch's operations (path.h), whatever the oracle says."""
    fm, kinds = nart_amd.EVAL_MASKS[mask]
    x = pc.grid("bxdf_f_pdf")
    x = x[np.isin(pc.rec_type(x), kinds)]
    parts = np.zeros_like(x)
    parts[:, :3] = dev.eval("bxdf_f", x)[:, :3]
    parts[:, 3] = dev.eval("bxdf_pdf", x)[:, 0]
    _check("bxdf_f_pdf", x, dev.eval("bxdf_f_pdf", x, fm=fm), parts)


def test_logf_through_lds_is_logf(dev):
    x = pc.grid("logf")
    _check("logf_lds", x, dev.eval("logf_lds", x), dev.eval("logf", x))


def test_sincos_op_is_eval_sincos(dev):
    x = pc.grid("sincos")
    o = dev.eval("sincos", x)
    s, c = dev.eval_sincos(x[:, 0])
    assert np.array_equal(pc.ubits(o[:, 0]), pc.ubits(s)) and np.array_equal(pc.ubits(o[:, 1]), pc.ubits(c))


@pytest.mark.parametrize("n", [1, 255, 257])
def test_record_count_off_the_block_size(dev, n):
    """Exactly n records come back when n is no multiple of the 256-lane block; the rest of the caller's
    buffer is not written."""
    x = pc.grid("bxdf_sample_f")[1000:1000 + n]
    want = pc.expected("bxdf_sample_f")[1000:1000 + n]
    got = dev.eval("bxdf_sample_f", x)
    assert got.shape == (n, pc.W)
    _check("bxdf_sample_f", x, got, want)
    lib = nart_amd.hip_lib()
    buf = np.full((n + 300, pc.W), -7.0, np.float32)
    xin = np.ascontiguousarray(pc.grid("bxdf_sample_f")[1000:1300 + n])
    assert lib.nart_hip_eval(dev._ctx, nart_amd.EVAL_OPS["bxdf_sample_f"], nart_amd.FT_ALL, xin.ctypes.data, n,
                             buf.ctypes.data) == 0
    _check("bxdf_sample_f", x, buf[:n], want)
    assert np.all(buf[n:] == -7.0)


def test_multi_device_context_answers_as_one_device(gpu, glass_scene, dev):
    m = nart_amd.HipRenderer(glass_scene, devices=[0, 0])
    for op in ("atan2f", "bxdf_sample_f"):
        x = pc.grid(op)[:5000]
        assert np.array_equal(pc.ubits(m.eval(op, x)), pc.ubits(dev.eval(op, x))), op


def test_argument_validation_on_a_live_context(dev):
    lib = nart_amd.hip_lib()
    x = np.zeros((4, pc.W), np.float32)
    y = np.full((4, pc.W), 3.0, np.float32)
    P, ops = ctypes.c_void_p, nart_amd.EVAL_OPS
    ev = lambda ctx, op, fm, i, n, o: lib.nart_hip_eval(ctx, op, fm, i, n, o)  # noqa: E731
    assert ev(dev._ctx, ops["logf"], nart_amd.FT_ALL, x.ctypes.data, 0, y.ctypes.data) == 0 and np.all(y == 3.0)
    assert ev(dev._ctx, ops["logf"], nart_amd.FT_ALL, P(), 4, y.ctypes.data) == -1
    assert ev(dev._ctx, ops["logf"], nart_amd.FT_ALL, x.ctypes.data, 4, P()) == -1
    assert ev(dev._ctx, len(ops), nart_amd.FT_ALL, x.ctypes.data, 4, y.ctypes.data) == -1
    for fm in (0, 0x3, 0x20, 0x400, 0x7FF):  # no mask, two kinds, a light bit, beyond FT_ALL
        assert ev(dev._ctx, ops["bxdf_f_pdf"], fm, x.ctypes.data, 4, y.ctypes.data) == -1, fm
    assert ev(dev._ctx, ops["logf"], nart_amd.FT_ALL, x.ctypes.data, (1 << 24) + 1, y.ctypes.data) == -1
    assert ev(dev._ctx, ops["logf"], nart_amd.FT_ALL, x.ctypes.data, 0xFFFFFFFF, y.ctypes.data) == -1
    assert np.all(y == 3.0)
    with pytest.raises(ValueError):
        dev.eval("logf", np.zeros((4, 3), np.float32))
