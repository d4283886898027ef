// Which buckets of a list one launch takes and which pixels they trace (no HIP, no context):
// render.hip render_buckets cuts its bucket list into batches with gather_batch; tests/test_bucket_batch.py
// compares it with a restatement.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace nd {

// The image a bucket list is cut from: total_* is the image grown by the filter bounds on each side,
// which the buckets tile (nart_session_geometry); image_* the image itself.
struct BucketGrid {
    uint32_t B = 16;  // bucket size
    uint32_t n_buckets_x = 0, total_width = 0, total_height = 0;
    uint32_t image_width = 0, image_height = 0;
};

// A traced pixel (a slot) as the kernels read it.
inline uint32_t pack_xy(uint32_t x, uint32_t y) { return x | (y << 16); }

// The pixels of a w x h rect at (x0, y0), row by row, appended to xy.
inline void append_rect(std::vector<uint32_t>& xy, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h) {
    for (uint32_t y = y0; y < y0 + h; ++y)
        for (uint32_t x = x0; x < x0 + w; ++x) xy.push_back(pack_xy(x, y));
}

// A batch of buckets whose traced pixels fit the slot budget: ids[b0 .. b1) with b1 returned, the first
// always taken.  xy receives the buckets' pixels, bucket by bucket in list order (edge buckets end at the
// total size: render.cpp:163-168), base each bucket's first slot; counted grows by the batch's pixels
// that lie inside the image.
inline uint32_t gather_batch(const BucketGrid& g, const uint32_t* ids, uint32_t b0, uint32_t n, size_t limit,
                             std::vector<uint32_t>& xy, std::vector<uint32_t>& base, uint64_t& counted) {
    xy.clear();
    base.clear();
    uint32_t b1 = b0;
    for (; b1 < n; ++b1) {
        const uint32_t bx = ids[b1] % g.n_buckets_x, by = ids[b1] / g.n_buckets_x;
        const uint32_t x0 = g.B * bx, y0 = g.B * by;
        const uint32_t x1 = std::min(g.B * (bx + 1), g.total_width), y1 = std::min(g.B * (by + 1), g.total_height);
        if (b1 > b0 && xy.size() + (size_t)(x1 - x0) * (y1 - y0) > limit) break;
        base.push_back((uint32_t)xy.size());
        append_rect(xy, x0, y0, x1 - x0, y1 - y0);
        // the part of the bucket inside the image
        const uint32_t ix = std::min(x1, std::max(x0, g.image_width)), iy = std::min(y1, std::max(y0, g.image_height));
        counted += (uint64_t)(ix - x0) * (iy - y0);
    }
    return b1;
}

}  // namespace nd
