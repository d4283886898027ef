"""A float32 numpy restatement of the parts denoise (include/nart_hip.h, "Denoised parts";
device/denoise_parts.h) in its fused form: the guides are prepared once, every tap offset's guide terms
w_n and d_g are computed once and shared by the parts, and only d_l, the falloff and the sums are per
part.  The operations and their order are tests/denoise_py.py's (which it borrows where they do not
change), so part k must equal denoise_py.denoise over part k bit for bit
(tests/test_denoise_parts_restatement.py).  Also parts_sum, and the designed inputs the tests share."""
import numpy as np

import denoise_py as dn

f32 = np.float32
PARTS_MAX = 9


# ---------------------------------------------------------------- the restatement
def prepare_shared(W, H, fb, albedo, normal, dp):
    """What the albedo and normal images alone decide: n, z, cov, a_d, slope (denoise_py.prepare's; its
    beauty argument decides none of them)."""
    st = dn.prepare(W, H, fb, np.zeros_like(albedo), albedo, normal, dp)
    return {k: st[k] for k in ("n", "z", "cov", "a_d", "slope")}


def prepare_part(W, H, fb, part, a_d):
    """One part's signal s, variance v (< 0: invalid) and alpha."""
    B = np.ascontiguousarray(part[fb:fb + H, fb:fb + W], f32)
    zero = f32(0)
    bw = B[..., 4]
    c = np.where((bw > 0)[..., None], B[..., :4] / bw[..., None], zero).astype(f32)
    valid = np.isfinite(c[..., :3]).all(-1)
    s = np.where(valid[..., None], c[..., :3] / a_d, zero).astype(f32)
    v = np.where(valid, zero, f32(-1)).astype(f32)
    return dict(s=s, v=v, alpha=c[..., 3].copy())


def guide_terms(sh, dp, dx, dy):
    """w_n and d_g of the tap at (dx, dy) for every centre: the guide half of denoise_py.tap_weight."""
    nq, _ = dn.shifted(sh["n"], dx, dy)
    zq, _ = dn.shifted(sh["z"], dx, dy)
    cq, _ = dn.shifted(sh["cov"], dx, dy)
    n_p, zp, cp = sh["n"], sh["z"], sh["cov"]
    dot = (n_p[..., 0] * nq[..., 0] + n_p[..., 1] * nq[..., 1]) + n_p[..., 2] * nq[..., 2]
    wn = dn.mn(f32(1), dn.mx(f32(0), dot))
    for _ in range(dp["normal_squarings"]):
        wn = wn * wn
    wn = np.where((zp == 0) & (zq == 0), f32(1), wn).astype(f32)
    cheb = f32(max(abs(dx), abs(dy)))
    dz = np.abs(zp - zq) / ((f32(dp["sigma_depth"]) * (sh["slope"] * cheb) + f32(dp["depth_eps"]) * dn.mx(zp, zq)) + f32(1e-30))
    dg = dz + np.abs(cp - cq) / f32(dp["sigma_coverage"])
    return wn, dg.astype(f32)


def falloff(wn, dg, d_l):
    """w_n * f(d_g + d_l): the falloff half."""
    t = dn.mx(f32(0), f32(1) - (dg + d_l) * f32(0.125))
    t2 = t * t
    t4 = t2 * t2
    return (wn * (t4 * t4)).astype(f32)


def variance_parts(sh, sigs, dp):
    """The variance pass over all parts: u = w_n * f(d_g) once per offset, su, sl, sl2 per part."""
    acc = [[np.zeros_like(p["v"]) for _ in range(3)] for p in sigs]
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            if dx == 0 and dy == 0:
                u = np.ones_like(sh["z"])
            else:
                wn, dg = guide_terms(sh, dp, dx, dy)
                u = falloff(wn, dg, f32(0))
            for p, a in zip(sigs, acc):
                sq, inside = dn.shifted(p["s"], dx, dy)
                vq, _ = dn.shifted(p["v"], dx, dy, -1.0)
                uk = np.where(inside & ~(vq < 0), u, f32(0)).astype(f32)
                l = dn.lum(sq)
                a[0] = a[0] + uk
                a[1] = a[1] + uk * l
                a[2] = a[2] + uk * (l * l)
    out = []
    for p, (su, sl, sl2) in zip(sigs, acc):
        m1, m2 = sl / su, sl2 / su
        out.append(np.where(p["v"] < 0, p["v"], dn.mx(f32(0), m2 - m1 * m1)).astype(f32))
    return out


def atrous_parts(sh, sigs, dp, step):
    """One a-trous pass over all parts: w_n, d_g once per offset; per part d_l, the weight, the sums."""
    H, W = sh["z"].shape
    yy, xx = np.mgrid[0:H, 0:W]
    per = []
    for p in sigs:
        v = p["v"]
        vb = np.zeros_like(v)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                vq = v[np.clip(yy + dy, 0, H - 1), np.clip(xx + dx, 0, W - 1)]
                vb = vb + (dn.K3[dy + 1] * dn.K3[dx + 1]) * dn.mx(vq, f32(0))
        per.append(dict(valid=~(v < 0), den=f32(dp["sigma_color"]) * np.sqrt(vb) + f32(1e-6), lp=dn.lum(p["s"]),
                        sw=np.zeros_like(v), sv=np.zeros_like(v), ss=np.zeros_like(p["s"])))
    for iy in range(-2, 3):
        for ix in range(-2, 3):
            dx, dy = ix * step, iy * step
            centre = ix == 0 and iy == 0
            if not centre:
                wn, dg = guide_terms(sh, dp, dx, dy)
            for p, a in zip(sigs, per):
                sq, inside = dn.shifted(p["s"], dx, dy)
                vq, _ = dn.shifted(p["v"], dx, dy, -1.0)
                use = inside & ~(vq < 0)
                w = np.full_like(p["v"], dn.H5[ix + 2] * dn.H5[iy + 2])
                if not centre:
                    d_l = np.where(a["valid"], np.abs(a["lp"] - dn.lum(sq)) / a["den"], f32(0)).astype(f32)
                    w = w * falloff(wn, dg, d_l)
                w = np.where(use, w, f32(0)).astype(f32)
                vq = np.where(use, vq, f32(0)).astype(f32)
                a["sw"] = a["sw"] + w
                a["ss"] = a["ss"] + w[..., None] * sq
                a["sv"] = a["sv"] + (w * w) * vq
    out = []
    for a in per:
        ok = a["sw"] > 0
        s2 = np.where(ok[..., None], a["ss"] / a["sw"][..., None], f32(0)).astype(f32)
        v2 = np.where(ok, a["sv"] / (a["sw"] * a["sw"]), f32(-1)).astype(f32)
        out.append((s2, v2))
    return out


def denoise_parts(W, H, fb, parts, albedo, normal, params=None, **kw):
    """The K denoised nart_pixel images, (K, H + 2 fb, W + 2 fb, 5) float32."""
    dp = dn.params_of(params, **kw)
    assert 1 <= dp["iterations"] <= 8 and 1 <= len(parts) <= PARTS_MAX
    out = np.zeros((len(parts), H + 2 * fb, W + 2 * fb, 5), f32)
    with np.errstate(all="ignore"):
        sh = prepare_shared(W, H, fb, albedo, normal, dp)
        sigs = [prepare_part(W, H, fb, part, sh["a_d"]) for part in parts]
        for p, v in zip(sigs, variance_parts(sh, sigs, dp)):
            p["v"] = v
        for i in range(dp["iterations"]):
            for p, (s2, v2) in zip(sigs, atrous_parts(sh, sigs, dp, 1 << i)):
                p["s"], p["v"] = s2, v2
        for k, p in enumerate(sigs):
            out[k, fb:fb + H, fb:fb + W, :3] = p["s"] * sh["a_d"]
            out[k, fb:fb + H, fb:fb + W, 3] = p["alpha"]
            out[k, fb:fb + H, fb:fb + W, 4] = 1
    return out


def parts_sum(images):
    """((d_0 + d_1) + d_2) + ... per r, g, b, starting from d_0 itself (-0 stays); alpha and the filter
    weight sum are d_0's."""
    out = np.array(images[0], f32, copy=True)
    with np.errstate(all="ignore"):
        for im in images[1:]:
            out[..., :3] = out[..., :3] + np.asarray(im, f32)[..., :3]
    return out


# ---------------------------------------------------------------- designed inputs
# The role of part k, whatever K is, so that part k is the same image for every K > k:
#   plain    the base image (denoise_py.synthetic without bad pixels) times its own noise
#   bad      as plain, with 8 + k scattered pixels made NaN or Inf: valid in the plain parts
#   invalid  every cropped pixel NaN, weight 1: the part is invalid everywhere
#   zero     every float 0 (weight 0 too)
# One pixel, everywhere(), is NaN in every part -- also in the zero part, which is otherwise all zero.
ROLES = ["plain", "bad", "invalid", "zero", "bad", "plain", "bad", "plain", "bad"]


def everywhere(W, H):
    """The (x, y) of the pixel that is invalid in every part (None if the image is too small to keep it
    apart from denoise_py.synthetic's zero-weight pixel)."""
    if W * H < 15:
        return None
    return (W // 3, H // 2) if (W // 3, H // 2) != (W // 2, H // 2) else None


def synthetic_parts(W, H, fb, K, seed=0):
    """-> (parts (K, totalH, totalW, 5), albedo, normal).  Guide regions, a sky band of empty pixels,
    partial coverage and a zero-weight pixel come from denoise_py.synthetic."""
    (beauty, albedo, normal), _spots = dn.synthetic(W, H, fb, seed=seed, bad_pixels=False)
    parts = np.zeros((K,) + beauty.shape, f32)
    crop = (slice(fb, fb + H), slice(fb, fb + W))
    for k in range(K):
        rng = np.random.default_rng([seed, k, 977])
        role = ROLES[k]
        if role == "zero":
            pass
        elif role == "invalid":
            parts[k] = beauty
            parts[k][crop + (slice(0, 3),)] = np.nan
            parts[k][crop + (4,)] = 1
        else:
            parts[k] = beauty
            noise = rng.gamma(2.0, 0.5, (H, W, 3)).astype(f32) * f32(0.25 + 0.5 * k)
            parts[k][crop + (slice(0, 3),)] *= noise
            if role == "bad":
                n_bad = min(8 + k, (W * H) // 2)
                for j, i in enumerate(rng.choice(W * H, n_bad, replace=False)):
                    parts[k][fb + i // W, fb + i % W, j % 3] = np.nan if j % 2 else np.inf
                    parts[k][fb + i // W, fb + i % W, 4] = max(parts[k][fb + i // W, fb + i % W, 4], f32(0.5))
        e = everywhere(W, H)
        if e is not None:
            parts[k][fb + e[1], fb + e[0], 1] = np.nan
            parts[k][fb + e[1], fb + e[0], 4] = 1
    return parts, albedo, normal
