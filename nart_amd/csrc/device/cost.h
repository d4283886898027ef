// Cost image (include/nart_hip.h, "Cost image"): from the path kernel's per-sample cost records
// (kernels.h k_render_rq with CS) to the per-pixel grid, and from a grid to an image.
//   k_cost_reduce   per slot of a batch: the sum of the slot's spp records, stored at the slot's pixel
//                   of the grid of traced pixels (every pixel is a slot of exactly one batch, so a store,
//                   not an add; the grid starts the frame at zero)
//   k_cost_image    per grid pixel (x, y): image pixel (y + fb, x + fb) of the totalW x totalH image
//                   = {float(w0), float(w1), float(w2), float(w3), float(spp)}; grid pixels that fall
//                   outside the image are dropped, the rest of the image is zero (the caller's memset)
// One lane per slot / per grid pixel, no LDS, no atomics; integer sums are order-free, and the
// conversions round to nearest even: tests/cost_py.py restates both in numpy bit for bit.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace nd {

struct CostReduceArgs {
    const uint4* records;     // per sample, RenderArgs::Lout's indexing
    const uint32_t* slot_xy;  // [n_slots] traced pixel (x | y << 16)
    const SlotSO* slot_so;    // [n_slots]
    uint4* grid;              // [grid_h][grid_w]
    uint32_t n_slots, spp, grid_w, grid_h;
};

__global__ __launch_bounds__(256) void k_cost_reduce(CostReduceArgs A) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n_slots) return;
    const SlotSO so = A.slot_so[i];
    uint4 sum = make_uint4(0u, 0u, 0u, 0u);
    for (uint32_t s = 0; s < A.spp; ++s) {
        const uint4 r = A.records[so.first + (uint64_t)s * so.stride];
        sum.x += r.x;
        sum.y += r.y;
        sum.z += r.z;
        sum.w += r.w;
    }
    const uint32_t xy = A.slot_xy[i], x = xy & 0xFFFFu, y = xy >> 16;
    if (x < A.grid_w && y < A.grid_h) A.grid[(size_t)y * A.grid_w + x] = sum;
}

struct CostImageArgs {
    const uint4* grid;  // [grid_h][grid_w]
    float* out;         // nart_pixel image, zero
    uint32_t grid_w, grid_h, spp;
    uint32_t W, H, totalW, totalH, fb;
};

__global__ __launch_bounds__(256) void k_cost_image(CostImageArgs A) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)A.grid_w * A.grid_h) return;
    const uint32_t x = (uint32_t)(i % A.grid_w), y = (uint32_t)(i / A.grid_w);
    const uint32_t ox = x + A.fb, oy = y + A.fb;
    if (ox >= A.totalW || oy >= A.totalH) return;
    const uint4 c = A.grid[i];
    float* o = A.out + ((size_t)oy * A.totalW + ox) * 5;
    o[0] = (float)c.x;  // (v_cvt_f32_u32: round to nearest even)
    o[1] = (float)c.y;
    o[2] = (float)c.z;
    o[3] = (float)c.w;
    o[4] = (float)A.spp;
}

}  // namespace nd
