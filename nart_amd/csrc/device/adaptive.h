// Adaptive sampling (include/nart_hip.h, nart_hip_render_adaptive): the two device kernels of the
// refinement loop (render.hip render_buckets_adaptive).
//   k_bucket_error   one float per listed bucket from its beauty and second-moment tiles: the
//                    relative standard error of the bucket's mean luminance
//   k_scatter_tiles  list-ordered scratch tiles -> the buckets' slots in the frame's tile buffers
//
// k_bucket_error runs one wavefront per bucket.  The lanes first evaluate the bucket's own pixels
// side by side (consecutive lanes read consecutive tile pixels) and park {sd, l} in LDS; then lane
// dy adds row dy from left to right, and lane 0 adds the row sums from top to bottom.  The sums
// therefore have one fixed order: the result depends neither on the launch shape nor on where the
// bucket sits in the list, and no atomics are involved.  Buckets too large to stage (2 B (B + 1)
// + 2 B floats of LDS) skip the staging: lane dy evaluates its row's pixels itself, in the same order.
//
// The arithmetic is float32 + - * / sqrt and comparisons only, in the order the header fixes, built
// without contraction: tests/adaptive_py.py restates it in numpy and the values agree bit for bit.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace nd {

struct BucketErrorArgs {
    const float* beauty;  // [list index][tile * tile][5]
    const float* moment;  // likewise: the second-moment tiles of the same render
    const uint32_t* ids;  // [list index] bucket id = by * nbx + bx
    float* err;           // [list index] E
    uint32_t n;           // buckets listed
    uint32_t B, fb, tile, nbx, totalW, totalH;
    float floor;
};

__device__ __forceinline__ float ae_max(float a, float b) { return a > b ? a : b; }

// {sd, l} of one own pixel: T the beauty tile pixel, M the moment tile pixel (5 floats each).
__device__ __forceinline__ void ae_pixel(const float* T, const float* M, float& sd, float& l) {
    const float tw = T[4];
    sd = 0.f;
    l = 0.f;
    if (tw > 0.f) {
        const float cr = T[0] / tw, cg = T[1] / tw, cb = T[2] / tw;
        const float mw = M[4];
        const float k = M[3] / (mw * mw);
        const float vr = ae_max(0.f, M[0] / mw - cr * cr) * k;
        const float vg = ae_max(0.f, M[1] / mw - cg * cg) * k;
        const float vb = ae_max(0.f, M[2] / mw - cb * cb) * k;
        sd = (0.2126f * sqrtf(vr) + 0.7152f * sqrtf(vg)) + 0.0722f * sqrtf(vb);
        l = ae_max((0.2126f * cr + 0.7152f * cg) + 0.0722f * cb, 0.f);
    }
}

// One block of one wavefront per listed bucket.  Dynamic LDS: STAGE 2 B (B + 1) + 2 B floats, else 2 B.
template <bool STAGE>
__global__ __launch_bounds__(64) void k_bucket_error(BucketErrorArgs A) {
    extern __shared__ float ae_lds[];
    const uint32_t i = blockIdx.x;
    if (i >= A.n) return;  // (the whole block)
    const uint32_t id = A.ids[i];
    const uint32_t bx = id % A.nbx, by = id / A.nbx;
    // the pixels render_buckets traces for the bucket (render.cpp:163-168), extra rows included
    const uint32_t nx = A.B * bx < A.totalW ? min(A.B, A.totalW - A.B * bx) : 0u;
    const uint32_t ny = A.B * by < A.totalH ? min(A.B, A.totalH - A.B * by) : 0u;
    const size_t tile0 = (size_t)i * A.tile * A.tile * 5;
    const float* T = A.beauty + tile0;
    const float* M = A.moment + tile0;
    const uint32_t pitch = A.B + 1;  // staged rows: lanes that walk rows side by side miss each other's banks
    float* row_sd = ae_lds;          // [B]
    float* row_l = ae_lds + A.B;     // [B]
    float* px_sd = ae_lds + 2 * A.B; // [B][pitch]
    float* px_l = px_sd + (size_t)A.B * pitch;
    if (STAGE) {
        for (uint32_t k = threadIdx.x; k < nx * ny; k += blockDim.x) {
            const uint32_t dy = k / nx, dx = k - dy * nx;
            const size_t t = ((size_t)(A.fb + dy) * A.tile + (A.fb + dx)) * 5;
            float sd, l;
            ae_pixel(T + t, M + t, sd, l);
            px_sd[dy * pitch + dx] = sd;
            px_l[dy * pitch + dx] = l;
        }
        __syncthreads();
    }
    for (uint32_t dy = threadIdx.x; dy < ny; dy += blockDim.x) {
        float rs = 0.f, rl = 0.f;
        for (uint32_t dx = 0; dx < nx; ++dx) {
            float sd, l;
            if (STAGE) {
                sd = px_sd[dy * pitch + dx];
                l = px_l[dy * pitch + dx];
            } else {
                const size_t t = ((size_t)(A.fb + dy) * A.tile + (A.fb + dx)) * 5;
                ae_pixel(T + t, M + t, sd, l);
            }
            rs += sd;
            rl += l;
        }
        row_sd[dy] = rs;
        row_l[dy] = rl;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float S = 0.f, Ls = 0.f;
        for (uint32_t dy = 0; dy < ny; ++dy) {
            S += row_sd[dy];
            Ls += row_l[dy];
        }
        A.err[i] = S / (Ls + A.floor * (float)(nx * ny));
    }
}

// Tile i of each listed scratch buffer to slot[i] of its frame buffer.  Grid (n, buffers).
constexpr int SCATTER_BUFS = 4;
struct ScatterArgs {
    const float* src[SCATTER_BUFS];  // [list index][tile_floats]
    float* dst[SCATTER_BUFS];        // [slot][tile_floats]
    const uint32_t* slot;            // [list index]
    uint32_t n, tile_floats;
};
__global__ __launch_bounds__(256) void k_scatter_tiles(ScatterArgs A) {
    const uint32_t i = blockIdx.x;
    if (i >= A.n) return;
    const float* src = A.src[blockIdx.y] + (size_t)i * A.tile_floats;
    float* dst = A.dst[blockIdx.y] + (size_t)A.slot[i] * A.tile_floats;
    for (uint32_t k = threadIdx.x; k < A.tile_floats; k += blockDim.x) dst[k] = src[k];
}

}  // namespace nd
