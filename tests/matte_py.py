"""Numpy restatement of the first-hit ID mattes (include/nart_hip.h, "First-hit ID mattes"): the
coverage planes' per-sample records, the plane images (the records through the restated AddSample and
tile combine of tests/test_aov_restatement.py), the ranking and the extraction, the last two written as
plain loops over the definition, one float32 operation at a time."""
import numpy as np

import nart_amd
from test_aov_restatement import add_sample, restate_render

f32 = np.float32
NO_HIT = 0xFFFFFFFF
MAX_IDS = 32


def n_planes(n):
    return (n + 3) // 4


def ids_of(scene, tri, kind):
    """The matte id per sample of first-hit triangle indices tri (any shape; NO_HIT or negative: a
    miss), as int64 with -1 for a miss: the triangle's mesh in scene order (kind 0) or that mesh's
    material (kind 1)."""
    tri = np.asarray(tri).astype(np.int64)
    meshes = scene.meshes().astype(np.int64)
    ntri = scene.counts()["triangles"]
    table = np.full(ntri + 1, -1, np.int64)  # the last entry serves the misses
    for m, (first, num, material, _prio) in enumerate(meshes):
        table[first:first + num] = m if kind == 0 else material
    hit = (tri >= 0) & (tri < ntri)
    return table[np.where(hit, tri, ntri)]


def records(ids, q, n=MAX_IDS):
    """Plane q's per-sample records (..., 4) float32 of the ids (..., ): {[id == 4q], .., [id == 4q+3]}
    as 1 or +0; a miss (a negative id) or an id >= n gives all +0."""
    ids = np.asarray(ids).astype(np.int64)
    ok = (ids >= 0) & (ids < n)
    out = np.zeros(ids.shape + (4,), f32)
    for c in range(4):
        out[..., c] = np.where(ok & (ids == 4 * q + c), f32(1), f32(0))
    return out


def restate_planes(p, uv, ids, n, with_terms=False):
    """The P = ceil(n / 4) plane images (P, totalH, totalW, 5) over per-sample ids (totalH, totalW, spp)
    at the image samples uv.  with_terms: also, per total-image pixel, the number of additions a sum
    of that pixel receives (count_terms)."""
    planes = [restate_render(p, uv, records(ids, q, n)) for q in range(n_planes(n))]
    g = nart_amd.session_geometry(p)
    out = np.stack(planes) if planes else np.zeros((0, g.total_height, g.total_width, 5), f32)
    return (out, count_terms(p, uv)) if with_terms else out


def count_terms(p, uv):
    """Additions per total-image pixel (totalH, totalW) int64 that a pixel's sum receives: one per
    (sample, pixel) pair of AddSample whose filter weight is not zero, and one per tile that is
    added into the pixel.  Counted by running the restated render with a filter table of ones where
    the real table is not zero, so that every such pair adds exactly 1 (small integers: exact)."""
    g = nart_amd.session_geometry(p)
    fb, B, T = g.filter_bounds, p.bucket_size, g.tile_size
    table = (nart_amd.filter_table() != 0).astype(f32)
    image = np.zeros((g.total_height, g.total_width), np.int64)
    zero4 = np.zeros(4, f32)
    for j in range(g.n_buckets_y):
        for i in range(g.n_buckets_x):
            tile = np.zeros((T, T, 5), f32)
            for y in range(B * j, min(B * (j + 1), g.total_height)):
                for x in range(B * i, min(B * (i + 1), g.total_width)):
                    for s in range(p.spp):
                        add_sample(tile, table, p, fb, f32(x + fb) + uv[y, x, s, 0], f32(y + fb) + uv[y, x, s, 1],
                                   zero4)
            nx = min(T, p.image_width + fb - i * B)
            ny = min(T, p.image_height + fb - j * B)
            if nx > 0 and ny > 0:
                image[j * B:j * B + ny, i * B:i * B + nx] += tile[:ny, :nx, 4].astype(np.int64) + 1
    return image


def rank(W, H, fb, planes, n, R):
    """The R / 2 rank images (R / 2, H + 2 fb, W + 2 fb, 5) float32 of the plane images
    (ceil(n / 4), H + 2 fb, W + 2 fb, 5), by the header's definition."""
    planes = np.asarray(planes, f32)
    assert R % 2 == 0 and 2 <= R <= 8 and 0 <= n <= MAX_IDS and (n == 0 or planes.shape[0] == n_planes(n))
    out = np.zeros((R // 2, H + 2 * fb, W + 2 * fb, 5), f32)
    for y in range(H):
        for x in range(W):
            Y, X = y + fb, x + fb
            Wt = planes[0, Y, X, 4] if n else f32(0)
            cand = []  # (c_m, m) of the candidates, m ascending
            if Wt > 0:
                for m in range(n):
                    with np.errstate(all="ignore"):
                        c = f32(planes[m // 4, Y, X, m % 4]) / f32(Wt)
                    if c > 0:  # false for zero, negative and NaN
                        cand.append((c, m))
            for r in range(R):
                best = None
                for c, m in cand:
                    if best is None or c > best[0]:  # among equal values the least m stays
                        best = (c, m)
                if best is None:
                    pair = (f32(-1), f32(0))
                else:
                    cand.remove(best)
                    pair = (f32(best[1]), best[0])
                out[r // 2, Y, X, 2 * (r % 2)] = pair[0]
                out[r // 2, Y, X, 2 * (r % 2) + 1] = pair[1]
            out[:, Y, X, 4] = 1
    return out


def extract(W, H, fb, ranks, mask):
    """The matte (H + 2 fb, W + 2 fb, 5) float32 of the id set `mask` (bit m: id m) from the rank
    images: per cropped pixel the float32 sum, r ascending, from 0, of the coverages of the ranks
    whose id is in the set."""
    ranks = np.asarray(ranks, f32)
    R = 2 * ranks.shape[0]
    out = np.zeros((H + 2 * fb, W + 2 * fb, 5), f32)
    for y in range(H):
        for x in range(W):
            Y, X = y + fb, x + fb
            m = f32(0)
            for r in range(R):
                i, c = ranks[r // 2, Y, X, 2 * (r % 2)], ranks[r // 2, Y, X, 2 * (r % 2) + 1]
                if i >= 0 and i < 64 and (mask >> int(i)) & 1:
                    with np.errstate(all="ignore"):
                        m = f32(m + c)
            out[Y, X, :4] = m
            out[Y, X, 4] = 1
    return out


def synthetic(W, H, fb, n, seed=0, bad_pixels=True):
    """Plane images (ceil(n / 4), H + 2 fb, W + 2 fb, 5) for the ranking: random filter weight sums,
    coverages drawn from a few values so that ties are common, most ids absent in most pixels; where
    the image has room, pixels with W = 0, W < 0 and W = NaN, and zero, negative, NaN and infinite
    contributions.  The border and the channels of ids >= n hold values that must not be read as ids.
    Returns (planes, spots): spots maps a name to the (x, y) of that pixel."""
    rng = np.random.default_rng(seed + 977)
    P = n_planes(n)
    planes = np.zeros((P, H + 2 * fb, W + 2 * fb, 5), f32)
    Wt = rng.uniform(0.5, 4.0, (H, W)).astype(f32)
    values = np.array([0, 0, 0, 0.125, 0.25, 0.25, 0.5, 1.0], f32)
    for m in range(4 * P):
        c = values[rng.integers(0, len(values), (H, W))]
        if m >= n:
            c = np.full((H, W), 0.75, f32)  # a channel beyond n: never an id
        planes[m // 4, fb:fb + H, fb:fb + W, m % 4] = c * Wt
    planes[:, fb:fb + H, fb:fb + W, 4] = Wt
    if fb > 0:
        planes[:, :fb] = planes[:, -fb:] = 0.25  # the border is not read
        planes[:, :, :fb] = planes[:, :, -fb:] = 0.25
    spots = {}
    if bad_pixels and W >= 8 and H >= 3:
        def at(name, x, y):
            spots[name] = (x, y)
            return (slice(None), y + fb, x + fb)
        planes[at("w_zero", 1, 1)][..., 4] = 0
        planes[at("w_negative", 2, 1)][..., 4] = -1
        planes[at("w_nan", 3, 1)][..., 4] = np.nan
        x, y = 4, 1
        spots["c_nan"] = (x, y)
        planes[0, y + fb, x + fb, 0] = np.nan
        x, y = 5, 1
        spots["c_negative"] = (x, y)
        planes[0, y + fb, x + fb, 0] = -2
        x, y = 6, 1
        spots["c_inf"] = (x, y)
        planes[0, y + fb, x + fb, 0] = np.inf
        x, y = 1, 2
        spots["all_equal"] = (x, y)
        planes[:, y + fb, x + fb, :4] = planes[0, y + fb, x + fb, 4] * f32(0.5)
        x, y = 2, 2
        spots["all_zero"] = (x, y)
        planes[:, y + fb, x + fb, :4] = 0
    return planes, spots
