"""Test-side restatement of adaptive sampling (include/nart_hip.h, "Adaptive sampling"): the level
list, the per-bucket error in float32 numpy with the header's operations in the header's order, and
the whole selection loop, so that the device's sample counts and errors can be compared bit for bit.

The tiles are restated out of per-sample radiance with the validated AddSample restatement
(tests/test_aov_restatement.py add_sample) and the per-bucket loop of tests/moment_py.py, kept per
tile instead of combined."""
import numpy as np

import nart_amd
from test_aov_restatement import add_sample, total_frame_uv

f32 = np.float32
MAX_LEVELS = 32


def levels(min_spp, growth, spp):
    """L_0 = min_spp, L_{i+1} = min(L_i * growth, spp), ending on spp; at most 32 levels."""
    out, L = [], int(min_spp)
    while L < spp and len(out) + 1 < MAX_LEVELS:
        out.append(L)
        L = min(L * int(growth), int(spp))
    out.append(int(spp))
    return out


def own_size(p, g, bucket_id):
    """(nx, ny): the pixels the bucket traces (render.cpp:163-168), extra rows included."""
    bx, by = bucket_id % g.n_buckets_x, bucket_id // g.n_buckets_x
    B = p.bucket_size
    return min(B, g.total_width - B * bx), min(B, g.total_height - B * by)


def _mx(a, b):
    return np.where(a > b, a, b).astype(f32)  # max(a, b) = a > b ? a : b


def bucket_error(T, M, nx, ny, fb, floor):
    """E of one bucket from its beauty tile T and moment tile M, both (tile, tile, 5) float32."""
    T = np.ascontiguousarray(T, f32)[fb:fb + ny, fb:fb + nx]
    M = np.ascontiguousarray(M, f32)[fb:fb + ny, fb:fb + nx]
    zero = f32(0)
    with np.errstate(all="ignore"):
        tw, mw = T[..., 4], M[..., 4]
        c = (T[..., :3] / tw[..., None]).astype(f32)
        k = (M[..., 3] / (mw * mw)).astype(f32)
        m2 = (M[..., :3] / mw[..., None]).astype(f32)
        var = _mx(zero, (m2 - c * c).astype(f32))
        V = (var * k[..., None]).astype(f32)
        r = np.sqrt(V).astype(f32)
        sd = ((f32(0.2126) * r[..., 0] + f32(0.7152) * r[..., 1]) + f32(0.0722) * r[..., 2]).astype(f32)
        lum = ((f32(0.2126) * c[..., 0] + f32(0.7152) * c[..., 1]) + f32(0.0722) * c[..., 2]).astype(f32)
        l = _mx(lum, zero)
        lit = tw > 0
        sd = np.where(lit, sd, zero).astype(f32)
        l = np.where(lit, l, zero).astype(f32)
        rs, rl = np.zeros(ny, f32), np.zeros(ny, f32)
        for dx in range(nx):  # every row from left to right
            rs = (rs + sd[:, dx]).astype(f32)
            rl = (rl + l[:, dx]).astype(f32)
        S, Ls = f32(0), f32(0)
        for dy in range(ny):  # the rows from top to bottom
            S = f32(S + rs[dy])
            Ls = f32(Ls + rl[dy])
        return f32(S / f32(Ls + f32(f32(floor) * f32(nx * ny))))


def restate_tiles(p, uv, L, ids, with_moment=True):
    """The beauty and the second-moment tile of every listed bucket, (len(ids), tile, tile, 5) each,
    over per-sample Li_alpha L (totalH, totalW, spp, 4) at image samples uv: RenderTile's pixel and
    sample order (restate_render, moment_py.restate_moment), without the combine.  Any per-sample
    float4 stream splats as Li_alpha does (the AOV records); with_moment False skips the moment tiles
    (they stay zero)."""
    g = nart_amd.session_geometry(p)
    table = nart_amd.filter_table().astype(f32)
    fb, B, T = g.filter_bounds, p.bucket_size, g.tile_size
    assert uv.dtype == f32 and L.dtype == f32
    with np.errstate(all="ignore"):
        L2 = (L * L).astype(f32)
    L2[..., 3] = 0
    beauty, moment = np.zeros((len(ids), T, T, 5), f32), np.zeros((len(ids), T, T, 5), f32)
    scratch, term = np.zeros((T, T, 5), f32), np.zeros((T, T, 5), f32)
    for n, b in enumerate(ids):
        i, j = int(b) % g.n_buckets_x, int(b) // g.n_buckets_x
        for y in range(B * j, min(B * (j + 1), g.total_height)):
            for x in range(B * i, min(B * (i + 1), g.total_width)):
                for s in range(p.spp):
                    scx, scy = f32(x + fb) + uv[y, x, s, 0], f32(y + fb) + uv[y, x, s, 1]
                    with np.errstate(all="ignore"):
                        add_sample(beauty[n], table, p, fb, scx, scy, L[y, x, s])
                        if not with_moment:
                            continue
                        scratch[...] = 0
                        add_sample(scratch, table, p, fb, scx, scy, L2[y, x, s])
                        w = scratch[..., 4]
                        term[..., :3] = scratch[..., :3]
                        term[..., 3] = w * w
                        term[..., 4] = w
                        moment[n] += term
    return beauty, moment


def select(p, min_spp, growth, threshold, floor, samples_of, first_errors=None, tiles_out=None):
    """The selection loop over the whole frame.  samples_of(spp) gives the per-sample Li_alpha of the
    total frame at that sample count, (totalH, totalW, spp, 4).  Returns (bucket_spp uint32,
    bucket_error float32, lists, threshold): the first two in bucket-id order, lists[i] the ids
    rendered at level i, and the threshold used.  threshold may be a function of the level-0 errors
    (called once, for tests that derive it).  first_errors: a list that receives the level-0 errors;
    tiles_out: a list that receives (level spp, ids, beauty tiles, moment tiles) per level."""
    g = nart_amd.session_geometry(p)
    nb = g.n_buckets_x * g.n_buckets_y
    lv = levels(min_spp, growth, p.spp)
    spp_out, err_out = np.zeros(nb, np.uint32), np.zeros(nb, f32)
    cur, lists = list(range(nb)), []
    for li, L in enumerate(lv):
        if not cur:
            break
        pl = p.copy()
        pl.spp = L
        beauty, moment = restate_tiles(pl, total_frame_uv(pl), np.ascontiguousarray(samples_of(L), f32), cur)
        E = np.array([bucket_error(beauty[n], moment[n], *own_size(p, g, b), g.filter_bounds, floor)
                      for n, b in enumerate(cur)], f32)
        if li == 0:
            if first_errors is not None:
                first_errors.extend(E.tolist())
            if callable(threshold):
                threshold = threshold(E)
        lists.append(list(cur))
        if tiles_out is not None:
            tiles_out.append((L, list(cur), beauty, moment))
        spp_out[cur], err_out[cur] = L, E
        last = li + 1 == len(lv)
        cur = [b for n, b in enumerate(cur) if not last and not (E[n] <= f32(threshold))]
    return spp_out, err_out, lists, threshold
