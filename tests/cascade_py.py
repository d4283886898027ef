"""Test-side restatement of the firefly cascade (include/nart_hip.h, "Firefly cascade"), in float32
numpy with the header's operations in the header's order, so that the device images can be compared
bit for bit: the split of the per-sample records into brightness layers, the layer images and the
reweighting.

The layer images reuse the validated AddSample restatement (tests/test_aov_restatement.py
add_sample, which reproduces the oracle's framebuffer) exactly as tests/moment_py.py does:
RenderTile's pixel and sample order per bucket, tiles combined in bucket raster order, once per
layer with that layer's records in the place of Li_alpha."""
import numpy as np

import nart_amd
from test_aov_restatement import add_sample

f32 = np.float32
LR, LG, LB = f32(0.2126), f32(0.7152), f32(0.0722)


def levels_of(start, base, layers):
    """b_0 = start, b_{j+1} = b_j * base in float32."""
    b = [f32(start)]
    for _ in range(layers - 1):
        b.append(f32(b[-1] * f32(base)))
    return np.array(b, f32)


def lum(c):
    return ((LR * c[..., 0] + LG * c[..., 1]) + LB * c[..., 2]).astype(f32)


def split_weights(L, levels, base):
    """Per record of L (..., 4): the layer weights (K, ...) float32 and `whole` (K, ...) bool, true
    where the layer takes the record itself (not a product).  A layer the sample does not reach has
    weight 0 and whole false: its record is exactly +0."""
    levels = np.asarray(levels, f32)
    K = len(levels)
    one, bm1 = f32(1), f32(f32(base) - f32(1))
    with np.errstate(all="ignore"):
        l = lum(L)
        low = ~((l - l) == 0) | (l <= levels[0])
        top = ~low & (l > levels[K - 1])
        mid = ~low & ~top
        w = np.zeros((K,) + l.shape, f32)
        whole = np.zeros((K,) + l.shape, bool)
        part = np.zeros((K,) + l.shape, bool)
        whole[0], whole[K - 1] = low, top
        left = mid.copy()
        for j in range(K - 1):  # the first j with l <= b_{j+1}: b_j < l holds since j - 1 failed
            here = left & (l <= levels[j + 1])
            w_lo = ((levels[j + 1] / l - one) / bm1).astype(f32)
            w_hi = (one - w_lo).astype(f32)
            w[j] = np.where(here, w_lo, w[j])
            w[j + 1] = np.where(here, w_hi, w[j + 1])
            part[j] |= here
            part[j + 1] |= here
            left &= ~here
        assert not left.any()
    w = np.where(whole, one, w).astype(f32)
    return w, whole, part


def split(L, levels, base):
    """The layers' record streams (K, ..., 4) float32 of the records L (..., 4)."""
    L = np.ascontiguousarray(L, f32)
    w, whole, part = split_weights(L, levels, base)
    with np.errstate(all="ignore"):
        prod = (L[None] * w[..., None]).astype(f32)
    out = np.zeros(prod.shape, f32)
    out = np.where(part[..., None], prod, out)
    out = np.where(whole[..., None], L[None], out)
    return np.ascontiguousarray(out, f32)


def restate_layers(p, uv, L, levels, base, with_bound=False):
    """The K layer images (K, totalH, totalW, 5) over per-sample Li_alpha L (totalH, totalW, spp, 4) at
    image samples uv.  with_bound: also, per pixel and contribution channel, the float64 sum of the
    magnitudes of the float32 terms (record channel times filter weight, over all layers) and the
    number of additions the pixel's layer sum received: one per (sample, layer) term of a layer the
    sample reaches, one per tile per layer, one per layer."""
    g = nart_amd.session_geometry(p)
    table = nart_amd.filter_table().astype(f32)
    fb, B, T = g.filter_bounds, p.bucket_size, g.tile_size
    assert uv.dtype == f32 and L.dtype == f32
    K = len(levels)
    rec = split(L, levels, base)  # (K, totalH, totalW, spp, 4)
    w_split, whole, part = split_weights(L, levels, base)
    reach = whole | part
    images = np.zeros((K, g.total_height, g.total_width, 5), f32)
    mag = np.zeros((g.total_height, g.total_width, 4), np.float64)
    count = np.zeros((g.total_height, g.total_width), np.int64)
    scratch = np.zeros((T, T, 5), f32)
    zero4 = np.zeros(4, f32)
    for j in range(g.n_buckets_y):
        for i in range(g.n_buckets_x):
            tiles = np.zeros((K, T, T, 5), f32)
            tmag, tcount = np.zeros((T, T, 4)), np.zeros((T, T), np.int64)
            for y in range(B * j, min(B * (j + 1), g.total_height)):
                for x in range(B * i, min(B * (i + 1), g.total_width)):
                    for s in range(p.spp):
                        scx, scy = f32(x + fb) + uv[y, x, s, 0], f32(y + fb) + uv[y, x, s, 1]
                        with np.errstate(all="ignore"):
                            for k in range(K):
                                add_sample(tiles[k], table, p, fb, scx, scy, rec[k, y, x, s])
                        if with_bound:
                            scratch[...] = 0
                            add_sample(scratch, table, p, fb, scx, scy, zero4)
                            w = scratch[..., 4].astype(np.float64)
                            for k in range(K):
                                if reach[k, y, x, s]:
                                    tmag += np.abs(rec[k, y, x, s].astype(np.float64))[None, None, :] * w[..., None]
                                    tcount += w != 0
            nx = min(T, p.image_width + fb - i * B)
            ny = min(T, p.image_height + fb - j * B)
            if nx > 0 and ny > 0:
                with np.errstate(all="ignore"):
                    images[:, j * B:j * B + ny, i * B:i * B + nx] += tiles[:, :ny, :nx]
                mag[j * B:j * B + ny, i * B:i * B + nx] += tmag[:ny, :nx]
                count[j * B:j * B + ny, i * B:i * B + nx] += tcount[:ny, :nx] + K
    count += K
    return (images, mag, count) if with_bound else images


def weights_of(W, H, fb, beauty, layers, levels, spp, kappa):
    """(m (K, H, W, 3), omega (K, H, W), ok (H, W)) of the cropped image by the header's formulas."""
    levels = np.asarray(levels, f32)
    K = len(levels)
    crop = lambda im: np.ascontiguousarray(im[..., fb:fb + H, fb:fb + W, :], f32)
    Bc, C = crop(beauty), crop(np.asarray(layers, f32))
    zero, one, N, kap = f32(0), f32(1), f32(spp), f32(kappa)
    with np.errstate(all="ignore"):
        Wt = Bc[..., 4]
        ok = Wt > 0
        m = np.where(ok[None, ..., None], C[..., :3] / Wt[None, ..., None], zero).astype(f32)
        l = lum(m)
        lam = np.where(l > 0, l, zero).astype(f32)
        omega = np.ones((K, H, W), f32)
        for j in range(1, K):
            s = (lam[j - 1] + lam[j]).astype(f32)
            if j + 1 < K:
                s = (s + lam[j + 1]).astype(f32)
            sp = np.zeros((H + 2, W + 2), f32)
            sp[1:H + 1, 1:W + 1] = s
            inside = np.zeros((H + 2, W + 2), bool)
            inside[1:H + 1, 1:W + 1] = True
            acc, cnt = np.zeros((H, W), f32), np.zeros((H, W), f32)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    v = inside[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
                    acc = np.where(v, acc + sp[1 + dy:1 + dy + H, 1 + dx:1 + dx + W], acc).astype(f32)
                    cnt = np.where(v, cnt + one, cnt).astype(f32)
            gm = (((acc * N) / levels[j]) / cnt).astype(f32)
            t = (gm / kap).astype(f32)
            omega[j] = np.where(t < one, t, one)
    return m, omega, ok


def reweight(W, H, fb, beauty, layers, levels, spp, kappa):
    """The robust nart_pixel image (H + 2 fb, W + 2 fb, 5): cropped pixels {rgb, alpha, 1}, zero in the
    border and where the beauty's filter weight sum is <= 0."""
    m, omega, ok = weights_of(W, H, fb, beauty, layers, levels, spp, kappa)
    Bc = np.ascontiguousarray(beauty[fb:fb + H, fb:fb + W], f32)
    with np.errstate(all="ignore"):
        rgb = m[0].copy()
        for j in range(1, len(m)):
            rgb = (rgb + (omega[j][..., None] * m[j]).astype(f32)).astype(f32)
        alpha = (Bc[..., 3] / Bc[..., 4]).astype(f32)
    out = np.zeros((H + 2 * fb, W + 2 * fb, 5), f32)
    px = np.zeros((H, W, 5), f32)
    px[..., :3] = rgb
    px[..., 3] = alpha
    px[..., 4] = 1
    out[fb:fb + H, fb:fb + W] = np.where(ok[..., None], px, f32(0))
    return out


def synthetic(W, H, fb, levels, spp, seed=0, bad_pixels=True):
    """A beauty and K layer images for the reweighting: random filter weight sums, layer j lit in a
    share of the pixels that shrinks with j (lone bright pixels in the upper layers), brightness about
    what one sample in `spp` of level b_j leaves; where the image has room, a pixel with W = 0 and a
    NaN pixel in layer 1.  Returns (beauty, layers, (zero_xy, nan_xy)) (None where they do not fit)."""
    rng = np.random.default_rng(seed + 4242)
    K = len(levels)
    beauty = np.zeros((H + 2 * fb, W + 2 * fb, 5), f32)
    layers = np.zeros((K,) + beauty.shape, f32)
    Wt = rng.uniform(0.5, float(spp), (H, W)).astype(f32)
    for j in range(K):
        lit = rng.uniform(0, 1, (H, W)) < 0.9 / (1 + j)
        mean = (rng.uniform(0.2, 3.0, (H, W, 3)) * float(levels[j]) / spp).astype(f32)
        layers[j, fb:fb + H, fb:fb + W, :3] = np.where(lit[..., None], mean * Wt[..., None], 0)
        layers[j, fb:fb + H, fb:fb + W, 3] = np.where(lit, Wt * f32(0.125), 0)
        layers[j, fb:fb + H, fb:fb + W, 4] = Wt
    if fb > 0:
        layers[:, :fb] = layers[:, -fb:] = 0.25  # the border is not read
    beauty[fb:fb + H, fb:fb + W, :4] = layers[:, fb:fb + H, fb:fb + W, :4].sum(axis=0)
    beauty[fb:fb + H, fb:fb + W, 4] = Wt
    spots = (None, None)
    if bad_pixels and W >= 5 and H >= 3:
        spots = ((1, 1), (W - 2, H - 2))
        (x, y) = spots[0]
        beauty[y + fb, x + fb, 4] = 0
        (x, y) = spots[1]
        layers[1, y + fb, x + fb, 1] = np.nan
    return beauty, layers, spots
