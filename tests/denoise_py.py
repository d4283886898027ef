"""A float32 numpy restatement of the a-trous denoiser (include/nart_hip.h, "Edge-avoiding a-trous
denoiser"; device/denoise.h): the same operations in the same order, so that the device image can be
compared with it bit for bit.  min and max are comparisons (mn, mx: a < b ? a : b, a > b ? a : b)
with the header's argument order; every sum starts at 0 and runs in the header's tap order, and a
tap the kernels skip adds an exact +0 here.  Also the synthetic inputs the tests share."""
import numpy as np

f32 = np.float32
DEFAULTS = dict(iterations=5, normal_squarings=5, sigma_color=4.0, sigma_depth=1.0, depth_eps=1e-3,
                sigma_coverage=0.05, albedo_floor=0.01)
H5 = [f32(0.0625), f32(0.25), f32(0.375), f32(0.25), f32(0.0625)]
K3 = [f32(0.25), f32(0.5), f32(0.25)]


def mx(a, b):
    return np.where(a > b, a, b).astype(f32)


def mn(a, b):
    return np.where(a < b, a, b).astype(f32)


def lum(s):
    return (f32(0.2126) * s[..., 0] + f32(0.7152) * s[..., 1]) + f32(0.0722) * s[..., 2]


def shifted(a, dx, dy, fill=0.0):
    """q[y, x] = a[y + dy, x + dx] where that lies inside, else fill; and the inside mask."""
    H, W = a.shape[:2]
    out = np.full_like(a, fill)
    inside = np.zeros((H, W), bool)
    ys0, ys1 = max(0, -dy), min(H, H - dy)
    xs0, xs1 = max(0, -dx), min(W, W - dx)
    if ys0 < ys1 and xs0 < xs1:
        out[ys0:ys1, xs0:xs1] = a[ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx]
        inside[ys0:ys1, xs0:xs1] = True
    return out, inside


def params_of(params=None, **kw):
    d = dict(DEFAULTS)
    if params is not None:
        d.update(params if isinstance(params, dict) else {k: getattr(params, k) for k in DEFAULTS})
    d.update(kw)
    return d


def prepare(W, H, fb, beauty, albedo, normal, dp):
    """-> n (H, W, 3), z, cov, s (H, W, 3), v (< 0: invalid), a_d (H, W, 3), alpha, slope."""
    crop = lambda im: np.ascontiguousarray(im[fb:fb + H, fb:fb + W], f32)
    B, A, N = crop(beauty), crop(albedo), crop(normal)
    zero = f32(0)
    bw, aw, hs = B[..., 4], A[..., 4], A[..., 3]
    c = np.where((bw > 0)[..., None], B[..., :4] / bw[..., None], zero).astype(f32)
    al = np.where((aw > 0)[..., None], A[..., :3] / aw[..., None], zero).astype(f32)
    cov = np.where(aw > 0, A[..., 3] / aw, zero).astype(f32)
    z = np.where(hs > 0, N[..., 3] / hs, zero).astype(f32)
    empty = ~(hs > 0) | (z == 0)
    z = np.where(empty, zero, z).astype(f32)
    n = np.where(empty[..., None], zero, N[..., :3] / hs[..., None]).astype(f32)
    miss = f32(1) - cov
    a_d = mx(al + miss[..., None], f32(dp["albedo_floor"]))
    valid = np.isfinite(c[..., :3]).all(-1)
    s = np.where(valid[..., None], c[..., :3] / a_d, zero).astype(f32)
    v = np.where(valid, zero, f32(-1)).astype(f32)

    def axis_slope(size, pos, lo, hi):
        if size == 1:
            return np.zeros_like(z)
        d_lo = np.abs(z - lo)
        d_hi = np.abs(hi - z)
        return np.where(pos == 0, d_hi, np.where(pos == size - 1, d_lo, mn(d_lo, d_hi))).astype(f32)

    yy, xx = np.mgrid[0:H, 0:W]
    sx = axis_slope(W, xx, shifted(z, -1, 0)[0], shifted(z, 1, 0)[0])
    sy = axis_slope(H, yy, shifted(z, 0, -1)[0], shifted(z, 0, 1)[0])
    return dict(n=n, z=z, cov=cov, s=s, v=v, a_d=a_d, alpha=c[..., 3].copy(), slope=(sx + sy).astype(f32))


def tap_weight(st, dp, dx, dy, d_l):
    """w_n * f(d_g + d_l) of the tap at (dx, dy) for every centre, and the tap's inside mask."""
    nq, inside = shifted(st["n"], dx, dy)
    zq, _ = shifted(st["z"], dx, dy)
    cq, _ = shifted(st["cov"], dx, dy)
    n_p, zp, cp = st["n"], st["z"], st["cov"]
    dot = (n_p[..., 0] * nq[..., 0] + n_p[..., 1] * nq[..., 1]) + n_p[..., 2] * nq[..., 2]
    wn = mn(f32(1), mx(f32(0), dot))
    for _ in range(dp["normal_squarings"]):
        wn = wn * wn
    wn = np.where((zp == 0) & (zq == 0), f32(1), wn).astype(f32)
    cheb = f32(max(abs(dx), abs(dy)))
    dz = np.abs(zp - zq) / ((f32(dp["sigma_depth"]) * (st["slope"] * cheb) + f32(dp["depth_eps"]) * mx(zp, zq)) + f32(1e-30))
    dg = dz + np.abs(cp - cq) / f32(dp["sigma_coverage"])
    t = mx(f32(0), f32(1) - (dg + d_l) * f32(0.125))
    t2 = t * t
    t4 = t2 * t2
    return (wn * (t4 * t4)).astype(f32), inside


def variance(st, dp):
    s, v = st["s"], st["v"]
    zero = np.zeros_like(v)
    su, sl, sl2 = zero.copy(), zero.copy(), zero.copy()
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            sq, inside = shifted(s, dx, dy)
            vq, _ = shifted(v, dx, dy, -1.0)
            use = inside & ~(vq < 0)
            if dx == 0 and dy == 0:
                u = np.ones_like(v)
            else:
                u, _ = tap_weight(st, dp, dx, dy, f32(0))
            u = np.where(use, u, f32(0)).astype(f32)
            l = lum(sq)
            su = su + u
            sl = sl + u * l
            sl2 = sl2 + u * (l * l)
    m1, m2 = sl / su, sl2 / su
    return np.where(v < 0, v, mx(f32(0), m2 - m1 * m1)).astype(f32)


def atrous(st, dp, step):
    s, v = st["s"], st["v"]
    H, W = v.shape
    valid_p = ~(v < 0)
    yy, xx = np.mgrid[0:H, 0:W]
    vb = np.zeros_like(v)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            vq = v[np.clip(yy + dy, 0, H - 1), np.clip(xx + dx, 0, W - 1)]
            vb = vb + (K3[dy + 1] * K3[dx + 1]) * mx(vq, f32(0))
    den = f32(dp["sigma_color"]) * np.sqrt(vb) + f32(1e-6)
    lp = lum(s)
    sw, sv = np.zeros_like(v), np.zeros_like(v)
    ss = np.zeros_like(s)
    for iy in range(-2, 3):
        for ix in range(-2, 3):
            dx, dy = ix * step, iy * step
            sq, inside = shifted(s, dx, dy)
            vq, _ = shifted(v, dx, dy, -1.0)
            use = inside & ~(vq < 0)
            w = np.full_like(v, H5[ix + 2] * H5[iy + 2])
            if ix != 0 or iy != 0:
                d_l = np.where(valid_p, np.abs(lp - lum(sq)) / den, f32(0)).astype(f32)
                w = w * tap_weight(st, dp, dx, dy, d_l)[0]
            w = np.where(use, w, f32(0)).astype(f32)
            vq = np.where(use, vq, f32(0)).astype(f32)
            sw = sw + w
            ss = ss + w[..., None] * sq
            sv = sv + (w * w) * vq
    ok = sw > 0
    s2 = np.where(ok[..., None], ss / sw[..., None], f32(0)).astype(f32)
    v2 = np.where(ok, sv / (sw * sw), f32(-1)).astype(f32)
    return s2, v2


def denoise(W, H, fb, beauty, albedo, normal, params=None, **kw):
    """The denoised nart_pixel image, (H + 2 fb, W + 2 fb, 5) float32."""
    dp = params_of(params, **kw)
    assert 1 <= dp["iterations"] <= 8
    with np.errstate(all="ignore"):
        st = prepare(W, H, fb, beauty, albedo, normal, dp)
        st["v"] = variance(st, dp)
        for i in range(dp["iterations"]):
            st["s"], st["v"] = atrous(st, dp, 1 << i)
        out = np.zeros((H + 2 * fb, W + 2 * fb, 5), f32)
        out[fb:fb + H, fb:fb + W, :3] = st["s"] * st["a_d"]
    out[fb:fb + H, fb:fb + W, 3] = st["alpha"]
    out[fb:fb + H, fb:fb + W, 4] = 1
    return out


def images_of(W, H, fb, rgb, alpha, albedo, cov, n, z, weight=None):
    """nart_pixel images (beauty, albedo, normal) whose filtered values are the given per-pixel
    ones: contributions are value * weight, the normal image's n and z are scaled by weight * cov
    (means over hit samples).  Border pixels get weight 1 and zeros."""
    shape = (H + 2 * fb, W + 2 * fb, 5)
    w = np.ones((H, W), f32) if weight is None else weight.astype(f32)
    out = []
    for rgb4 in (np.concatenate([rgb, alpha[..., None]], -1), np.concatenate([albedo, cov[..., None]], -1),
                 np.concatenate([n, z[..., None]], -1) * cov[..., None]):
        im = np.zeros(shape, f32)
        im[..., 4] = 1
        im[fb:fb + H, fb:fb + W, :4] = rgb4.astype(f32) * w[..., None]
        im[fb:fb + H, fb:fb + W, 4] = w
        out.append(im)
    return out


def synthetic(W, H, fb, seed=0, bad_pixels=True):
    """Inputs with several guide regions (a tilted floor, a wall with another normal, a sphere-like
    blob), empty pixels (a sky band), partially covered pixels along the sky's edge, varying filter
    weights, one zero-weight pixel and, with bad_pixels, one NaN and one Inf beauty pixel.  Returns
    (beauty, albedo, normal) and the (x, y) of the zero-weight, NaN and Inf pixels (None where the
    image is too small to hold them apart)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(f32)
    u, t = xx / f32(max(W - 1, 1)), yy / f32(max(H - 1, 1))
    wall = u > 0.55
    blob = ((u - 0.3) ** 2 + (t - 0.6) ** 2) < 0.03
    sky = t < 0.2
    n = np.zeros((H, W, 3), f32)
    n[...] = (0.0, 0.8, 0.6)
    n[wall] = (-0.9, 0.1, 0.4)
    n[blob] = (0.2, 0.3, 0.9)
    z = (f32(4) + f32(3) * t + f32(0.5) * u).astype(f32)
    z[wall] = (f32(6) - f32(2) * u + f32(0.2) * t)[wall]
    z[blob] = f32(2.5)
    cov = np.ones((H, W), f32)
    cov[sky] = 0
    edge = (~sky) & (shifted(sky.astype(f32), 0, -1)[0] > 0)
    cov[edge] = rng.uniform(0.2, 0.8, int(edge.sum())).astype(f32)
    albedo = np.zeros((H, W, 3), f32)
    albedo[...] = (0.7, 0.6, 0.5)
    albedo[wall] = (0.2, 0.5, 0.8)
    albedo[blob] = (0.9, 0.9, 0.1)
    albedo = albedo * cov[..., None]
    light = np.where(wall, f32(0.5), f32(1.5)) + np.where(blob, f32(2), f32(0))
    light = np.where(sky, f32(0.3), light).astype(f32)
    noise = rng.gamma(2.0, 0.5, (H, W, 3)).astype(f32)
    rgb = (albedo + (f32(1) - cov)[..., None]) * light[..., None] * noise
    alpha = np.maximum(cov, f32(0.25)).astype(f32)
    weight = rng.uniform(0.5, 2.0, (H, W)).astype(f32)
    beauty, alb, nrm = images_of(W, H, fb, rgb, alpha, albedo, cov, n, z, weight)
    spots = [None, None, None]
    if W * H >= 15:
        cells = [(W // 2, H // 2), (W // 4, H - 1), (W - 1, H // 3)]
        if len(set(cells)) == 3:
            spots = cells
            (x0, y0) = cells[0]
            for im in (beauty, alb, nrm):
                im[y0 + fb, x0 + fb] = 0  # zero weight: nothing was splatted here
            if bad_pixels:
                beauty[cells[1][1] + fb, cells[1][0] + fb, 1] = np.nan
                beauty[cells[2][1] + fb, cells[2][0] + fb, 0] = np.inf
            else:
                spots[1] = spots[2] = None
    return (beauty, alb, nrm), spots
