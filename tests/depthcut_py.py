"""Depth cuts (include/nart_hip.h, "Depth cuts") restated for the tests: the layers in numpy float32, the
bound within which the layers sum back to the beauty, and the frames the tests share.  The yardstick of a
cut image is the unchanged oracle at `bounces = d` where the RNG start states agree: the whole frame at
1 spp, the first sample of every pixel otherwise.  The frames come from lightgroup_py.shared_frames, whose
oracle cache is keyed on p.bounces."""
import numpy as np

import lightgroup_py as lg

f32 = np.float32
CUTS_MAX = 8
bits, bits_equal, report = lg.bits, lg.bits_equal, lg.report


def layers(cut_images, beauty):
    """layers(I[K], B): K + 1 images; per pixel and channel of r, g, b
        layer_0 = I_0;  layer_j = I_j - I_{j-1} (0 < j < K);  layer_K = B - I_{K-1}
    each one float32 subtraction; alpha and filter weight sum of every layer copied from B.

    Summing the layers back (layers_sum: s_0 = layer_0, s_j = s_{j-1} + layer_j in float32) meets B within
        |s_K - B| <= (3 K + 1) 2^-24 M,   M = max(|I_0|, ..., |I_{K-1}|, |B|) of the pixel and channel,
    for finite values whose differences do not overflow.  In exact arithmetic the sum telescopes to B.  Each
    of the K subtractions and K additions is rounded once, by at most half an ulp, i.e. u = 2^-24 of its
    result (float32 addition and subtraction are exact in the denormal range, so nothing else is lost):
    a subtraction's result is at most 2 M (1 + u), a partial sum s_j is I_j but for the errors so far, at
    most M (1 + 3 K u).  The errors add up to at most K (2 M + M) u plus terms in u^2, which the "+ 1"
    covers for K <= 8."""
    I = np.asarray(cut_images, f32)
    B = np.asarray(beauty, f32)
    assert I.ndim == 4 and I.shape[-1] == 5 and I.shape[1:] == B.shape and 1 <= I.shape[0] <= CUTS_MAX
    K = I.shape[0]
    out = np.empty((K + 1,) + B.shape, f32)
    with np.errstate(all="ignore"):
        out[0, ..., :3] = I[0, ..., :3]
        for j in range(1, K + 1):
            upper = I[j, ..., :3] if j < K else B[..., :3]
            out[j, ..., :3] = (upper - I[j - 1, ..., :3]).astype(f32)
    out[..., 3:] = B[..., 3:]
    return out


def layers_sum(L):
    """The r, g, b of the layers summed ascending in float32."""
    L = np.asarray(L, f32)
    with np.errstate(all="ignore"):
        s = L[0, ..., :3].copy()
        for j in range(1, L.shape[0]):
            s = (s + L[j, ..., :3]).astype(f32)
    return s


def layers_bound(cut_images, beauty):
    """(3 K + 1) 2^-24 M per pixel and channel (layers' docstring), in float64."""
    I = np.asarray(cut_images, np.float64)[..., :3]
    B = np.asarray(beauty, np.float64)[..., :3]
    M = np.maximum(np.abs(I).max(0), np.abs(B))
    return (3 * I.shape[0] + 1) * 2.0 ** -24 * M


def with_bounces(p, d):
    """A copy of p with the bounce limit d: the oracle's yardstick frame of cut d."""
    q = type(p).from_buffer_copy(p)
    q.bounces = d
    return q


# The frames the GPU tests compare at 1 spp (tests/test_gpu_depth_cuts.py) and the definition test checks
# with the oracle alone (tests/test_depth_cuts_definition.py): key -> (scene, width, height, params, cuts)
MATERIALS_DIRECT = {"bucket_size": 16, "filter_width": 1.5}
FRAMES_1SPP = {
    "materials_direct": ("materials", 50, 37, MATERIALS_DIRECT, [1, 2, 5]),
    "materials_queue": ("materials", 432, 300, {}, [1, 2, 5]),
    "materials_groups": ("materials", 1056, 750, {}, [1, 2, 5]),
    "veach": ("veach", 48, 32, {}, [1, 2, 3]),
    "ring": ("ring", 48, 32, {}, [1, 2, 3]),
    "env": ("env", 48, 32, {}, [1, 2, 5]),
    "envc": ("envc", 48, 32, {}, [1, 2, 5]),
    "nested": ("nested", 48, 36, {}, [1, 3, 5, 16]),
}


def frame_params(frames, key, spp=1):
    name, w, h, kw, cuts = FRAMES_1SPP[key]
    return name, frames.params(name, w, h, spp, **kw), list(cuts)
