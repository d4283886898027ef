"""A float32 numpy restatement of the cross-filtered denoiser (include/nart_hip.h, "Cross-filtered
denoising"; device/denoise_cross.h): the same operations in the same order, so that the device images
can be compared with it bit for bit.  The guide, coverage, a_d, slope and alpha, the tap weight and
min / max / lum are tests/denoise_py.py's (the plain denoiser's restatement); a tap the kernels skip
adds an exact +0 here.  Also the synthetic halves the tests share."""
import numpy as np

import denoise_py as dn

f32 = np.float32
mx, mn, lum, shifted = dn.mx, dn.mn, dn.lum, dn.shifted


def prepare(W, H, fb, half_a, half_b, beauty, albedo, normal, dp):
    """denoise_py.prepare's state (n, z, cov, a_d, alpha, slope: from the beauty, albedo and normal
    images) with the two signals: s (2, H, W, 3) and v (2, H, W), v < 0 where the pixel is invalid."""
    st = dn.prepare(W, H, fb, beauty, albedo, normal, dp)
    crop = lambda im: np.ascontiguousarray(im[fb:fb + H, fb:fb + W], f32)
    zero = f32(0)
    c, has = [], []
    for half in (half_a, half_b):
        P = crop(half)
        w = P[..., 3]
        has.append(w > 0)
        c.append(np.where((w > 0)[..., None], P[..., :3] / w[..., None], zero).astype(f32))
    valid = has[0] & has[1] & np.isfinite(c[0]).all(-1) & np.isfinite(c[1]).all(-1)
    s = [np.where(valid[..., None], ch / st["a_d"], zero).astype(f32) for ch in c]
    d = (lum(s[0]) - lum(s[1])).astype(f32)
    v = np.where(valid, f32(0.5) * (d * d), f32(-1)).astype(f32)
    st["s"] = np.stack(s)
    st["v"] = np.stack([v, v])
    st["beauty_mean"] = np.where((crop(beauty)[..., 4] > 0)[..., None], crop(beauty)[..., :3] / crop(beauty)[..., 4:5],
                                 zero).astype(f32)
    return st


def variance(st, dp):
    """v <- sum u v / sum u over the 7x7 window's valid taps, for both halves (which hold one v)."""
    v = st["v"][0]
    zero = np.zeros_like(v)
    su, sv = zero.copy(), zero.copy()
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            vq, inside = shifted(v, dx, dy, -1.0)
            use = inside & ~(vq < 0)
            if dx == 0 and dy == 0:
                u = np.ones_like(v)
            else:
                u, _ = dn.tap_weight(st, dp, dx, dy, f32(0))
            u = np.where(use, u, f32(0)).astype(f32)
            vq = np.where(use, vq, f32(0)).astype(f32)
            su = su + u
            sv = sv + u * vq
    out = np.where(v < 0, v, sv / su).astype(f32)
    return np.stack([out, out])


def atrous(st, dp, step):
    s, v = st["s"], st["v"]
    H, W = v.shape[1:]
    valid_p = [~(v[0] < 0), ~(v[1] < 0)]
    yy, xx = np.mgrid[0:H, 0:W]
    den, lp = [None, None], [None, None]
    for h in (0, 1):
        o = 1 - h
        vb = np.zeros_like(v[o])
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                vq = v[o][np.clip(yy + dy, 0, H - 1), np.clip(xx + dx, 0, W - 1)]
                vb = vb + (dn.K3[dy + 1] * dn.K3[dx + 1]) * mx(vq, f32(0))
        den[h] = f32(dp["sigma_color"]) * np.sqrt(vb) + f32(1e-6)
        lp[h] = lum(s[o])
    sw = [np.zeros_like(v[0]), np.zeros_like(v[0])]
    sv = [np.zeros_like(v[0]), np.zeros_like(v[0])]
    ss = [np.zeros_like(s[0]), np.zeros_like(s[0])]
    for iy in range(-2, 3):
        for ix in range(-2, 3):
            dx, dy = ix * step, iy * step
            sq, vq, use = [None, None], [None, None], [None, None]
            for h in (0, 1):
                sq[h], inside = shifted(s[h], dx, dy)
                vq[h], _ = shifted(v[h], dx, dy, -1.0)
                use[h] = inside & ~(vq[h] < 0)
            for h in (0, 1):
                o = 1 - h
                w = np.full_like(v[0], dn.H5[ix + 2] * dn.H5[iy + 2])
                if ix != 0 or iy != 0:
                    d_l = np.where(valid_p[o] & use[o], np.abs(lp[h] - lum(sq[o])) / den[h], f32(0)).astype(f32)
                    w = w * dn.tap_weight(st, dp, dx, dy, d_l)[0]
                w = np.where(use[h], w, f32(0)).astype(f32)
                vqh = np.where(use[h], vq[h], f32(0)).astype(f32)
                sw[h] = sw[h] + w
                ss[h] = ss[h] + w[..., None] * sq[h]
                sv[h] = sv[h] + (w * w) * vqh
    s2, v2 = [], []
    for h in (0, 1):
        ok = sw[h] > 0
        s2.append(np.where(ok[..., None], ss[h] / sw[h][..., None], f32(0)).astype(f32))
        v2.append(np.where(ok, sv[h] / (sw[h] * sw[h]), f32(-1)).astype(f32))
    return np.stack(s2), np.stack(v2)


def finalize(W, H, fb, st):
    """(denoised, error) nart_pixel images (H + 2 fb, W + 2 fb, 5)."""
    s, v, a_d = st["s"], st["v"], st["a_d"]
    bad = (v[0] < 0) | (v[1] < 0)
    rgb = (((s[0] + s[1]) * f32(0.5)) * a_d).astype(f32)
    t = (((s[0] - s[1]) * f32(0.5)) * a_d).astype(f32)
    e = (t * t).astype(f32)
    out = np.zeros((H + 2 * fb, W + 2 * fb, 5), f32)
    err = np.zeros_like(out)
    out[fb:fb + H, fb:fb + W, :3] = np.where(bad[..., None], st["beauty_mean"], rgb)
    err[fb:fb + H, fb:fb + W, :3] = np.where(bad[..., None], f32(0), e)
    for im in (out, err):
        im[fb:fb + H, fb:fb + W, 3] = st["alpha"]
        im[fb:fb + H, fb:fb + W, 4] = 1
    return out, err


def denoise(W, H, fb, half_a, half_b, beauty, albedo, normal, params=None, **kw):
    """The cross-denoised image and the error image."""
    dp = dn.params_of(params, **kw)
    assert 1 <= dp["iterations"] <= 8
    with np.errstate(all="ignore"):
        st = prepare(W, H, fb, half_a, half_b, beauty, albedo, normal, dp)
        st["v"] = variance(st, dp)
        for i in range(dp["iterations"]):
            st["s"], st["v"] = atrous(st, dp, 1 << i)
        return finalize(W, H, fb, st)


def plain_without_variance(W, H, fb, beauty, albedo, normal, params=None, **kw):
    """The plain restatement's prepare, a-trous passes and finalise with variance 0 in every valid
    pixel (denoise_py.denoise without its variance pass): what the cross filter's rgb equals, bit for
    bit, when the halves are identical and the beauty's mean is theirs."""
    dp = dn.params_of(params, **kw)
    with np.errstate(all="ignore"):
        st = dn.prepare(W, H, fb, beauty, albedo, normal, dp)
        for i in range(dp["iterations"]):
            st["s"], st["v"] = dn.atrous(st, dp, 1 << i)
        out = np.zeros((H + 2 * fb, W + 2 * fb, 5), f32)
        out[fb:fb + H, fb:fb + W, :3] = st["s"] * st["a_d"]
    out[fb:fb + H, fb:fb + W, 3] = st["alpha"]
    out[fb:fb + H, fb:fb + W, 4] = 1
    return out, st


def synthetic(W, H, fb, seed=0, spp=8, bad_pixels=True):
    """Halves to go with denoise_py.synthetic's beauty, albedo and normal images: per pixel the
    beauty's contributions split into two halves of random weight shares, whose means scatter around
    the beauty's mean with independent noise -- so that the halves add up to the beauty (up to
    rounding) as rendered halves do.  With bad_pixels and room for them: the beauty's zero-weight, NaN
    and Inf pixels (the NaN and the Inf each in one half only), a pixel whose half 1 has no weight, and
    one whose half 0 is Inf while the beauty is finite.  Returns ((half_a, half_b, beauty, albedo,
    normal), spots) with spots the (x, y) of those five pixels (None where they do not fit)."""
    (beauty, alb, nrm), cells = dn.synthetic(W, H, fb, seed=seed, bad_pixels=bad_pixels)
    rng = np.random.default_rng(seed + 7717)
    crop = beauty[fb:fb + H, fb:fb + W]
    share = rng.uniform(0.35, 0.65, (H, W)).astype(f32)
    noise = rng.gamma(float(spp), 1.0 / spp, (2, H, W, 3)).astype(f32)
    halves = []
    for h in (0, 1):
        sh = share if h == 0 else (f32(1) - share)
        im = np.zeros_like(beauty)
        im[..., 4] = beauty[..., 4]
        with np.errstate(all="ignore"):
            im[fb:fb + H, fb:fb + W, :3] = crop[..., :3] * sh[..., None] * noise[h]
        im[fb:fb + H, fb:fb + W, 3] = crop[..., 4] * sh
        halves.append(im)
    spots = list(cells) + [None, None]
    if cells[0] is not None:
        (x, y) = cells[0]
        for im in halves:
            im[y + fb, x + fb] = 0
    if bad_pixels and cells[1] is not None:
        (x, y) = cells[1]   # the beauty's NaN came with one sample: half 1's
        halves[0][y + fb, x + fb, :3] = np.nan_to_num(halves[0][y + fb, x + fb, :3], nan=0.25)
        halves[1][y + fb, x + fb, 1] = np.nan
        (x, y) = cells[2]   # the Inf with one of half 0's
        halves[1][y + fb, x + fb, :3] = np.nan_to_num(halves[1][y + fb, x + fb, :3], nan=0.25, posinf=0.5)
        halves[0][y + fb, x + fb, 0] = np.inf
        extra = [(W // 3, 0), ((2 * W) // 3, H - 1)]
        if len(set(extra + list(cells))) == 5:
            spots[3], spots[4] = extra
            (x, y) = extra[0]
            halves[1][y + fb, x + fb, :4] = 0
            (x, y) = extra[1]
            halves[0][y + fb, x + fb, 2] = np.inf
    return (halves[0], halves[1], beauty, alb, nrm), spots
