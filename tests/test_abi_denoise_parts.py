"""C ABI of the parts denoise: include/nart_hip.h declares its four entry points, libnart_hip.so exports
them on a CPU-only host, the Python bindings name them, and without a context they refuse before
anything touches a GPU (with one: tests/test_gpu_denoise_parts.py)."""
import ctypes
import os
import re

import numpy as np

import nart_amd
from nart_amd import build as nb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["nart_hip_denoise_parts", "nart_hip_render_denoised_light_groups", "nart_hip_render_denoised_depth_layers",
                "nart_hip_denoise_parts_timings"]


def _header():
    text = open(os.path.join(REPO, "include", "nart_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_entry_points():
    code = _header()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(" % name, code), name
    assert re.search(r"#define NART_DENOISE_PARTS_MAX 9u", code)
    # the stage is written up where the depth cuts used to call it the next step
    assert "obvious next step" not in open(os.path.join(REPO, "include", "nart_hip.h")).read()


def test_library_exports_and_bindings(built):
    lib = ctypes.CDLL(nb.build_hip_lib())
    missing = [n for n in ENTRY_POINTS if not hasattr(lib, n)]
    assert not missing, missing
    assert set(ENTRY_POINTS) <= set(nart_amd.HIP_SYMBOLS)
    for name in ("denoise_parts", "render_denoised_light_groups", "render_denoised_depth_layers", "denoise_parts_timings"):
        assert callable(getattr(nart_amd.HipRenderer, name)), name


def test_null_context_or_parameters_are_invalid(built):
    lib = nart_amd.hip_lib()
    x = np.zeros(8, np.float32)
    fake = ctypes.c_void_p(x.ctypes.data)  # never dereferenced: every call below fails on a null argument
    p = x.ctypes.data
    assert lib.nart_hip_denoise_parts(None, None, None, 1, p, p, p, p, None, None) == -1
    assert lib.nart_hip_denoise_parts(fake, None, None, 1, p, p, p, p, None, None) == -1
    assert lib.nart_hip_render_denoised_light_groups(None, None, None, None, p, 1, 1, p, None, None, None, None, None) == -1
    assert lib.nart_hip_render_denoised_light_groups(fake, None, None, None, p, 1, 1, p, None, None, None, None, None) == -1
    assert lib.nart_hip_render_denoised_depth_layers(None, None, None, None, p, 1, p, None, None, None, None, None) == -1
    assert lib.nart_hip_render_denoised_depth_layers(fake, None, None, None, p, 1, p, None, None, None, None, None) == -1
    assert lib.nart_hip_denoise_parts_timings(None, None, None, None, None, None, None) == -1
    assert not x.any()
