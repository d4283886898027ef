"""The cost image (include/nart_hip.h, "Cost image") restated for the tests: the grid's size, the image of a
grid and the per-bucket sums in numpy, the invariants of a sample's record, and the oracle's path counts of
the frames the tests share.  Integers are compared exactly everywhere.  The frames are depthcut_py's
(FRAMES_1SPP over lightgroup_py.shared_frames), plus materials 50x37 at 8 spp."""
import numpy as np

import depthcut_py as dc

f32 = np.float32
KEYS = sorted(dc.FRAMES_1SPP)
# (key of depthcut_py.FRAMES_1SPP, spp): every frame the GPU test compares with the oracle's counts
FRAMES = [(k, 1) for k in KEYS] + [("materials_direct", 8)]


def grid_shape(p, g):
    """(grid_h, grid_w): the traced pixels, RenderTile's x, y range (g: session_geometry(p))."""
    return (min(p.bucket_size * g.n_buckets_y, g.total_height), min(p.bucket_size * g.n_buckets_x, g.total_width))


def cost_image(p, g, cost):
    """Grid pixel (x, y) to image pixel (y + fb, x + fb) of the (total_height, total_width, 5) image as
    {float32(w0), float32(w1), float32(w2), float32(w3), float32(spp)}, the conversions rounded to nearest
    even (numpy's uint32 -> float32 cast); grid pixels that fall outside the image are dropped; zero
    elsewhere."""
    cost = np.asarray(cost, np.uint32)
    gh, gw = grid_shape(p, g)
    assert cost.shape == (gh, gw, 4)
    fb = g.filter_bounds
    out = np.zeros((g.total_height, g.total_width, 5), f32)
    h, w = min(gh, g.total_height - fb), min(gw, g.total_width - fb)
    out[fb:fb + h, fb:fb + w, :4] = cost[:h, :w].astype(f32)
    out[fb:fb + h, fb:fb + w, 4] = f32(p.spp)
    return out


def bucket_sums(p, g, cost):
    """(n_buckets_y, n_buckets_x, 4) uint64: the sums over the pixels of every bucket, bucket (bx, by)
    holding the grid's x in [B bx, B (bx + 1)) and y likewise."""
    cost = np.asarray(cost, np.uint64)
    B = p.bucket_size
    out = np.zeros((g.n_buckets_y, g.n_buckets_x, 4), np.uint64)
    for by in range(g.n_buckets_y):
        for bx in range(g.n_buckets_x):
            out[by, bx] = cost[B * by:B * (by + 1), B * bx:B * (bx + 1)].reshape(-1, 4).sum(axis=0, dtype=np.uint64)
    return out


def sample_invariants(rec, bounces):
    """What holds for every sample's record {w0 extension rays, w1 shadow rays, w2 shaded hits, w3 steps}
    at a bounce limit > 0: the camera ray is an extension ray and every continued bounce adds one, up to
    the limit; every extension ray but possibly the last found a hit that was shaded; a shaded hit traces
    at most the two shadow rays of EstimateDirect.  Returns the list of the violated ones."""
    r = np.asarray(rec, np.int64).reshape(-1, 4)
    w0, w1, w2 = r[:, 0], r[:, 1], r[:, 2]
    bad = []
    if not ((1 <= w0) & (w0 <= bounces)).all():
        bad.append("1 <= w0 <= bounces")
    if not ((w0 - 1 <= w2) & (w2 <= w0)).all():
        bad.append("w0 - 1 <= w2 <= w0")
    if not (w1 <= 2 * w2).all():
        bad.append("w1 <= 2 w2")
    return bad


def frame_params(frames, key, spp=1):
    name, p, _cuts = dc.frame_params(frames, key, spp)
    return name, p


_counts = {}


def oracle_counts(frames, key, spp=1, bounces=None):
    """The unchanged oracle's path counts (oracle.PATH_COUNTS) of a frame, at the session's bounce limit
    or at `bounces`; rendered once per test session."""
    import oracle
    k = (key, spp, bounces)
    if k not in _counts:
        name, p = frame_params(frames, key, spp)
        if bounces is not None:
            p = dc.with_bounces(p, bounces)
        c = {}
        oracle.Oracle(frames.scene(name)).render(p, counts=c)
        _counts[k] = c
    return dict(_counts[k])
