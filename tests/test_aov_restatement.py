"""A float32 numpy restatement of the reference's AddSample (src/core/render.cpp:23-70) and tile
combine (:183-203), the yardstick of the AOV images (tests/test_gpu_aovs.py): any per-sample
float4 stream, splatted and combined as Li_alpha is.  It is validated here against the oracle's
own framebuffer first, so it is independent of the code under test; the AOV entry points' argument
checks, which need no GPU, are tested here too."""
import ctypes

import numpy as np

import nart_amd
import oracle

f32 = np.float32
FILTER_TABLE_RESOLUTION = 64


def total_frame_uv(p):
    """The Latin-square image samples of every pixel of the total frame, (totalH, totalW, spp, 2):
    RenderTile seeds each pixel's RNG with y * totalWidth + x (render.cpp:81-85)."""
    g = nart_amd.session_geometry(p)
    uv = np.zeros((g.total_height, g.total_width, p.spp, 2), f32)
    for y in range(g.total_height):
        for x in range(g.total_width):
            uv[y, x] = oracle.latin_square(y * g.total_width + x, p.spp)[0]
    return uv


def add_sample(tile, table, p, fb, scx, scy, L):
    """AddSample: one sample at total-image coordinates (scx, scy) into its bucket's tile.  Every
    operation is a float32 one in the reference's order; a sample touches a tile pixel at most
    once, so the window is handled as arrays."""
    fw, B = f32(p.filter_width), f32(p.bucket_size)
    x0, x1 = int(np.floor(scx - fw)), int(np.ceil(scx + fw))
    y0, y1 = int(np.floor(scy - fw)), int(np.ceil(scy + fw))
    dist_x = (np.arange(x0, x1).astype(f32) + f32(0.5)) - scx
    dist_y = (np.arange(y0, y1).astype(f32) + f32(0.5)) - scy
    dist = np.sqrt(dist_x[None, :] * dist_x[None, :] + dist_y[:, None] * dist_y[:, None])
    q = (dist / fw) * f32(FILTER_TABLE_RESOLUTION)
    index = np.minimum(q.astype(np.int32) & 0xFF, FILTER_TABLE_RESOLUTION - 1)  # uint8 cast, then min
    weight = table[index]

    def mod(a, b):  # glm::mod
        return a - b * np.floor(a / b)

    tile_x = np.floor(dist_x + mod(scx - f32(fb), B) + f32(fb)).astype(np.int64)
    tile_y = np.floor(dist_y + mod(scy - f32(fb), B) + f32(fb)).astype(np.int64)
    assert len(set(tile_x.tolist())) == len(tile_x) and len(set(tile_y.tolist())) == len(tile_y)
    iy, ix = tile_y[:, None], tile_x[None, :]
    tile[iy, ix, :4] += L[None, None, :] * weight[:, :, None]
    tile[iy, ix, 4] += weight


def restate_render(p, uv, L):
    """RenderSession::Render over per-sample values L (totalH, totalW, spp, 4) at the image samples
    uv (totalH, totalW, spp, 2): RenderTile's pixel and sample order per bucket, then the tiles
    summed into the image in bucket raster order.  Returns (totalH, totalW, 5) float32."""
    g = nart_amd.session_geometry(p)
    table = nart_amd.filter_table().astype(f32)
    fb, B, T = g.filter_bounds, p.bucket_size, g.tile_size
    assert uv.dtype == f32 and L.dtype == f32
    image = np.zeros((g.total_height, g.total_width, 5), f32)
    for j in range(g.n_buckets_y):
        for i in range(g.n_buckets_x):
            tile = np.zeros((T, T, 5), f32)
            for y in range(B * j, min(B * (j + 1), g.total_height)):
                for x in range(B * i, min(B * (i + 1), g.total_width)):
                    for s in range(p.spp):
                        add_sample(tile, table, p, fb, f32(x + fb) + uv[y, x, s, 0], f32(y + fb) + uv[y, x, s, 1],
                                   L[y, x, s])
            # tile pixels beyond imageWidth + filterBounds / imageHeight + filterBounds are ignored
            nx = min(T, p.image_width + fb - i * B)
            ny = min(T, p.image_height + fb - j * B)
            if nx > 0 and ny > 0:
                image[j * B:j * B + ny, i * B:i * B + nx] += tile[:ny, :nx]
    return image


def _params(scene, w, h, spp, **kw):
    p = nart_amd.load_sessions(scene.path)[0]
    p.image_width, p.image_height, p.spp = w, h, spp
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_restatement_reproduces_oracle_framebuffer(glass_scene):
    """glassSphere 24x20, 2 spp, bucket 16 (ragged buckets, extra rows): the restatement over the
    oracle's own per-sample Li_alpha equals the oracle's framebuffer bit for bit."""
    p = _params(glass_scene, 24, 20, 2, bucket_size=16)
    g = nart_amd.session_geometry(p)
    orc = oracle.Oracle(glass_scene)
    L, uv = orc.render_samples(p, 0, 0, g.total_width, g.total_height, with_uv=True)
    assert _bits_equal(uv, total_frame_uv(p))
    got, ref = restate_render(p, uv, L), orc.render(p)
    assert _bits_equal(got, ref), "%d floats differ" % int((got.view(np.uint32) != ref.view(np.uint32)).sum())


def test_restatement_other_bucket_and_filter(glass_scene):
    """Bucket 12 / filter width 1.0, where the last total-frame columns and rows are never traced
    (nBuckets * bucketSize < totalWidth): the second configuration of the AOV splat test."""
    p = _params(glass_scene, 24, 20, 2, bucket_size=12, filter_width=1.0, bounces=2)
    g = nart_amd.session_geometry(p)
    orc = oracle.Oracle(glass_scene)
    L, uv = orc.render_samples(p, 0, 0, g.total_width, g.total_height, with_uv=True)
    assert _bits_equal(restate_render(p, uv, L), orc.render(p))


def test_aov_entry_points_reject_null_without_gpu(built):
    from nart_amd import build as nb
    nb.build_hip_lib()
    lib = nart_amd.hip_lib()
    p = nart_amd.default_params()
    assert lib.nart_hip_render_aovs(None, ctypes.byref(p), 3, None, None, None, None, None) == -1  # NART_E_INVALID
    assert lib.nart_hip_render_aov_samples(None, ctypes.byref(p), 0, 0, 1, 1, None, None) == -1
