"""C ABI of the half buffers and the cross-filtered denoiser: include/nart_hip.h declares the entry points
and documents them under "Half buffers" and "Cross-filtered denoising", libnart_hip.so exports them on a
CPU-only host, the Python bindings name them with the header's signatures, and without a context they
refuse before anything touches a GPU (with one: tests/test_gpu_halves.py, tests/test_gpu_denoise_cross.py;
the cross entry points' null arguments: tests/test_denoise_cross_restatement.py)."""
import ctypes
import os
import re

import numpy as np

import nart_amd
from nart_amd import api
from nart_amd import build as nb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["nart_hip_render_halves", "nart_hip_denoise_cross", "nart_hip_render_denoised_cross",
                "nart_hip_denoise_cross_timings"]


def _header():
    return open(os.path.join(REPO, "include", "nart_hip.h")).read()


def test_header_declares_and_documents_the_entry_point():
    text = _header()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint nart_hip_render_halves\s*\(([^)]*)\)", code)
    assert m
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["nart_ctx* ctx", "const nart_render_params* p", "uint32_t aovs", "const nart_guide_params* gp",
                    "nart_pixel* image", "nart_pixel* albedo", "nart_pixel* normal", "nart_pixel* half_a", "nart_pixel* half_b",
                    "nart_render_stats* stats", "double* halves_ms"]
    assert "/* Half buffers:" in text and "k_half_split" in text and "i mod 2 == h" in text
    assert "/* Cross-filtered denoising:" in text
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(" % name, code), name


def test_library_exports_and_bindings(built):
    lib = ctypes.CDLL(nb.build_hip_lib())
    missing = [n for n in ENTRY_POINTS if not hasattr(lib, n)]
    assert not missing, missing
    assert set(ENTRY_POINTS) <= set(nart_amd.HIP_SYMBOLS)
    res, args = api._HIP_SIGS["nart_hip_render_halves"]
    assert res is ctypes.c_int and len(args) == 11
    assert args[1] == ctypes.POINTER(nart_amd.RenderParams) and args[2] is ctypes.c_uint32
    assert args[3] == ctypes.POINTER(nart_amd.GuideParams)
    assert args[9] == ctypes.POINTER(nart_amd.RenderStats) and args[10] == ctypes.POINTER(ctypes.c_double)
    assert callable(nart_amd.HipRenderer.render_halves) and callable(nart_amd.half_mean)
    for name, n_args in (("nart_hip_denoise_cross", 11), ("nart_hip_render_denoised_cross", 9),
                         ("nart_hip_denoise_cross_timings", 5)):
        assert api._HIP_SIGS[name][0] is ctypes.c_int and len(api._HIP_SIGS[name][1]) == n_args, name
    for name in ("denoise_cross", "render_denoised_cross", "denoise_cross_timings"):
        assert callable(getattr(nart_amd.HipRenderer, name)), name
    assert "half_mean" in nart_amd.__all__


def test_null_context_or_parameters_are_invalid(built):
    lib = nart_amd.hip_lib()
    x = np.zeros(8, np.float32)
    fake = ctypes.c_void_p(x.ctypes.data)  # never dereferenced: every call below fails on a null argument
    d = x.ctypes.data
    p = nart_amd.default_params()
    assert lib.nart_hip_render_halves(None, ctypes.byref(p), 0, None, d, None, None, d, d, None, None) == -1
    assert lib.nart_hip_render_halves(fake, None, 0, None, d, None, None, d, d, None, None) == -1
    assert lib.nart_hip_render_halves(None, None, 3, None, None, None, None, None, None, None, None) == -1
    assert not x.any()


def test_half_mean():
    h = np.zeros((2, 3, 5), np.float32)
    h[0, 0] = [2, 4, 6, 2, 5]
    h[1, 2] = [1, 1, 1, 0, 5]  # no sample of this parity reached the pixel: the mean is 0, not inf
    m = nart_amd.half_mean(h)
    assert m.shape == (2, 3, 3) and m.dtype == np.float32
    assert m[0, 0].tolist() == [1, 2, 3] and not m[1, 2].any() and not m[0, 1].any()
