"""Test-side restatement of the half buffers (include/nart_hip.h, "Half buffers"), in float32 numpy,
so that the device images can be compared bit for bit.

Half h is the validated AddSample restatement (tests/test_aov_restatement.py restate_render, which
reproduces the oracle's framebuffer) run once over half h's record stream in the place of Li_alpha:
{L.r, L.g, L.b, 1} for a sample whose index in its pixel's sequence has parity h, {0, 0, 0, 0} for
every other sample.  restate_half_alone is the other reading of the definition: only the samples of
parity h are splatted at all, which gives the same contribution bits and, as the filter weight sum,
the half's own."""
import numpy as np

import nart_amd
from test_aov_restatement import add_sample, restate_render

f32 = np.float32


def split(L, h):
    """Half h's record stream (..., spp, 4) float32 of the records L (..., spp, 4): the colour is
    copied, not multiplied, and the other parity's records are +0."""
    L = np.ascontiguousarray(L, f32)
    out = np.zeros(L.shape, f32)
    out[..., h::2, :3] = L[..., h::2, :3]
    out[..., h::2, 3] = 1
    return out


def restate_half(p, uv, L, h):
    """Half image h (totalH, totalW, 5) over per-sample Li_alpha L (totalH, totalW, spp, 4) at the
    image samples uv."""
    with np.errstate(all="ignore"):
        return restate_render(p, uv, split(L, h))


def restate_halves(p, uv, L):
    return np.stack([restate_half(p, uv, L, 0), restate_half(p, uv, L, 1)])


def restate_half_alone(p, uv, L, h):
    """The splat of the samples of parity h alone, in the beauty's order: restate_render's loops with
    the other samples skipped.  Its filter weight sum is the half's own."""
    g = nart_amd.session_geometry(p)
    table = nart_amd.filter_table().astype(f32)
    fb, B, T = g.filter_bounds, p.bucket_size, g.tile_size
    rec = split(L, h)
    image = np.zeros((g.total_height, g.total_width, 5), f32)
    with np.errstate(all="ignore"):
        for j in range(g.n_buckets_y):
            for i in range(g.n_buckets_x):
                tile = np.zeros((T, T, 5), f32)
                for y in range(B * j, min(B * (j + 1), g.total_height)):
                    for x in range(B * i, min(B * (i + 1), g.total_width)):
                        for s in range(h, p.spp, 2):
                            add_sample(tile, table, p, fb, f32(x + fb) + uv[y, x, s, 0], f32(y + fb) + uv[y, x, s, 1],
                                       rec[y, x, s])
                nx = min(T, p.image_width + fb - i * B)
                ny = min(T, p.image_height + fb - j * B)
                if nx > 0 and ny > 0:
                    image[j * B:j * B + ny, i * B:i * B + nx] += tile[:ny, :nx]
    return image


def half_mean(half):
    """rgb / contribution[3] in float32, 0 where the half holds no sample."""
    half = np.ascontiguousarray(half, f32)
    with np.errstate(all="ignore"):
        return np.where((half[..., 3] > 0)[..., None], half[..., :3] / half[..., 3:4], f32(0)).astype(f32)
