"""Test-side restatements of the second-moment image and of the denoiser's sample-variance mode
(include/nart_hip.h, "Second-moment image" and "Sample variance"), in float32 numpy with the header's
operations in the header's order, so that the device images can be compared bit for bit.

The moment image reuses the validated AddSample restatement (tests/test_aov_restatement.py
add_sample, which reproduces the oracle's framebuffer): each sample is splatted alone into a zeroed
scratch tile with the record {r*r, g*g, b*b, 0}, which leaves (ch*ch)*w and w exactly (0 + x = x) in
the pixels it touches and 0 elsewhere; the scratch is then added to the bucket's tile, the fourth
channel as w*w.  Adding the untouched pixels' +0 changes no sum."""
import numpy as np

import denoise_py as dn
import nart_amd
from test_aov_restatement import add_sample

f32 = np.float32


def restate_moment(p, uv, L, with_bound=False):
    """The moment image over per-sample Li_alpha L (totalH, totalW, spp, 4) at image samples uv:
    RenderTile's pixel and sample order per bucket, tiles combined in bucket raster order.
    with_bound: also a float64 accumulation of the same float32 terms, the number of additions each
    pixel received (sample terms and tile sums) and the float64 sum of the terms' magnitudes."""
    g = nart_amd.session_geometry(p)
    table = nart_amd.filter_table().astype(f32)
    fb, B, T = g.filter_bounds, p.bucket_size, g.tile_size
    assert uv.dtype == f32 and L.dtype == f32
    with np.errstate(all="ignore"):
        L2 = (L * L).astype(f32)
    L2[..., 3] = 0
    shape = (g.total_height, g.total_width, 5)
    image = np.zeros(shape, f32)
    image64, mag64, count = np.zeros(shape, np.float64), np.zeros(shape, np.float64), np.zeros(shape[:2], np.int64)
    scratch, term = np.zeros((T, T, 5), f32), np.zeros((T, T, 5), f32)
    for j in range(g.n_buckets_y):
        for i in range(g.n_buckets_x):
            tile = np.zeros((T, T, 5), f32)
            tile64, tmag, tcount = np.zeros((T, T, 5)), np.zeros((T, T, 5)), np.zeros((T, T), np.int64)
            for y in range(B * j, min(B * (j + 1), g.total_height)):
                for x in range(B * i, min(B * (i + 1), g.total_width)):
                    for s in range(p.spp):
                        scratch[...] = 0
                        add_sample(scratch, table, p, fb, f32(x + fb) + uv[y, x, s, 0], f32(y + fb) + uv[y, x, s, 1],
                                   L2[y, x, s])
                        w = scratch[..., 4]
                        term[..., :3] = scratch[..., :3]
                        term[..., 3] = w * w
                        term[..., 4] = w
                        with np.errstate(all="ignore"):
                            tile += term
                        if with_bound:
                            tile64 += term
                            tmag += np.abs(term.astype(np.float64))
                            tcount += w != 0
            nx = min(T, p.image_width + fb - i * B)
            ny = min(T, p.image_height + fb - j * B)
            if nx > 0 and ny > 0:
                with np.errstate(all="ignore"):
                    image[j * B:j * B + ny, i * B:i * B + nx] += tile[:ny, :nx]
                image64[j * B:j * B + ny, i * B:i * B + nx] += tile64[:ny, :nx]
                mag64[j * B:j * B + ny, i * B:i * B + nx] += tmag[:ny, :nx]
                count[j * B:j * B + ny, i * B:i * B + nx] += tcount[:ny, :nx] + 1
    return (image, image64, count, mag64) if with_bound else image


def variance_of(W, H, fb, beauty, moment, a_d):
    """(V (H, W, 3), v (H, W)) of the cropped image by the header's formula; v ignores validity."""
    crop = lambda im: np.ascontiguousarray(im[fb:fb + H, fb:fb + W], f32)
    B, M = crop(beauty), crop(moment)
    zero = f32(0)
    with np.errstate(all="ignore"):
        bw, mw = B[..., 4], M[..., 4]
        c = np.where((bw > 0)[..., None], B[..., :3] / bw[..., None], zero).astype(f32)
        k = (M[..., 3] / (mw * mw)).astype(f32)
        m2 = (M[..., :3] / mw[..., None]).astype(f32)
        var = dn.mx(zero, m2 - c * c)
        V = np.where((mw > 0)[..., None], var * k[..., None], zero).astype(f32)
        r = (np.sqrt(V) / a_d).astype(f32)
        sd = (f32(0.2126) * r[..., 0] + f32(0.7152) * r[..., 1]) + f32(0.0722) * r[..., 2]
        v = (sd * sd).astype(f32)
        v = np.where(v < f32(1e30), v, f32(1e30)).astype(f32)
    return V, v


def prepare(W, H, fb, beauty, albedo, normal, moment, dp):
    """denoise_py.prepare's state with v from the moment image (an invalid pixel keeps v = -1), and V."""
    with np.errstate(all="ignore"):
        st = dn.prepare(W, H, fb, beauty, albedo, normal, dp)
    V, v = variance_of(W, H, fb, beauty, moment, st["a_d"])
    st["v"] = np.where(st["v"] < 0, st["v"], v).astype(f32)
    return st, V


def denoise(W, H, fb, beauty, albedo, normal, moment, params=None, **kw):
    """The sample-variance mode's denoised nart_pixel image: prepare with the moment image, no
    variance pass, then denoise_py's passes and finalise."""
    dp = dn.params_of(params, **kw)
    assert 1 <= dp["iterations"] <= 8
    with np.errstate(all="ignore"):
        st, _V = prepare(W, H, fb, beauty, albedo, normal, moment, dp)
        for i in range(dp["iterations"]):
            st["s"], st["v"] = dn.atrous(st, dp, 1 << i)
        out = np.zeros((H + 2 * fb, W + 2 * fb, 5), f32)
        out[fb:fb + H, fb:fb + W, :3] = st["s"] * st["a_d"]
    out[fb:fb + H, fb:fb + W, 3] = st["alpha"]
    out[fb:fb + H, fb:fb + W, 4] = 1
    return out


def synthetic_moment(W, H, fb, beauty, spp=4, seed=0, bad_pixels=True):
    """A moment image consistent with `beauty` (denoise_py.synthetic's): the pixel's radiance with a
    relative spread per channel, as `spp` equally weighted samples would leave it, plus the bad-pixel
    cases where the image has room: a pixel with mw = 0, one whose second moment lies below the
    squared mean (clamps to 0), one of 1e38 and one NaN (both with a finite beauty).  Returns the
    image and the (x, y) of those four pixels (None where they do not fit)."""
    rng = np.random.default_rng(seed + 991)
    crop = beauty[fb:fb + H, fb:fb + W]
    bw = crop[..., 4]
    with np.errstate(all="ignore"):
        c = np.where((bw > 0)[..., None], crop[..., :3] / bw[..., None], 0).astype(f32)
    c = np.where(np.isfinite(c), c, 1).astype(f32)
    spread = rng.uniform(0.0, 0.8, (H, W, 3)).astype(f32)
    m2 = (c * c) * (f32(1) + spread * spread)
    M = np.zeros((H + 2 * fb, W + 2 * fb, 5), f32)
    M[..., 4] = beauty[..., 4]
    M[fb:fb + H, fb:fb + W, :3] = m2 * bw[..., None]
    M[fb:fb + H, fb:fb + W, 3] = (bw * bw) / f32(spp)
    spots = [None] * 4
    if bad_pixels and W >= 5 and H >= 3:
        spots = [(0, 0), (W - 1, 0), (1, 0), (W - 2, 0)]  # the top row: denoise_py.synthetic's spots lie below it
        (x, y) = spots[0]
        M[y + fb, x + fb] = 0                                           # mw = 0
        (x, y) = spots[1]
        M[y + fb, x + fb, :3] = f32(0.5) * (c[y, x] * c[y, x]) * bw[y, x]  # M.ch / mw < c^2
        (x, y) = spots[2]
        M[y + fb, x + fb, :3] = f32(1e38)
        (x, y) = spots[3]
        M[y + fb, x + fb, 1] = np.nan
    return M, spots
