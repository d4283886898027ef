// Firefly cascade (include/nart_hip.h, nart_hip_render_cascade): the two device kernels.
//   k_cascade_split     per sample record: the share of one brightness layer, into a second
//                       per-sample record buffer that the plain splat kernels then consume
//   k_cascade_reweight  per cropped-image pixel: the layers' means, each trusted as far as the 3x3
//                       neighbourhood holds samples of about its brightness, summed into one image
//
// k_cascade_split runs one lane per record along the sample layout (dense in both sample orders, as
// k_moment relies on): no LDS, no atomics.  It runs once per layer per batch; the layer's levels
// (its own and its two neighbours', the first and the top one) are passed by value, so the kernel
// indexes no table.
//
// k_cascade_reweight works on 32 x 8-pixel tiles in 256-thread blocks, lanes along x.  The K planes
// of lambda for the tile plus a one-pixel halo are staged in LDS (34 x 10 x K floats: 10.9 KB at
// K = 8); every lane then reads the layer and beauty pixels of its own centre once.  No atomics and
// no cross-lane reduction: the result is a pure function of the inputs, whatever the launch shape.
//
// The arithmetic is float32 + - * / and comparisons only, in the order the header fixes, built
// without contraction: tests/cascade_py.py restates it in numpy and the values agree bit for bit.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace nd {

constexpr uint32_t CASCADE_MAX_LAYERS = 8;

__device__ __forceinline__ float cs_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// The levels layer j's split needs: b_0, b_{K-1}, and b_{j-1}, b_j, b_{j+1} (unused ones 0).
struct CascadeSplitArgs {
    const float4* L;  // the batch's Li_alpha records
    float4* out;      // layer j's records
    uint64_t n;       // records
    float b_first, b_top, b_prev, b_cur, b_next;
    float base_m1;    // B - 1
    uint32_t j, K;
};

__global__ __launch_bounds__(256) void k_cascade_split(CascadeSplitArgs A) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const float4 v = A.L[i];
    const float l = cs_lum(v.x, v.y, v.z);
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!(l - l == 0.f) || l <= A.b_first) {
        if (A.j == 0) o = v;
    } else if (l > A.b_top) {
        if (A.j + 1 == A.K) o = v;
    } else {
        // b_first < l <= b_top: the one interval b_j < l <= b_{j+1} that holds l has this layer as
        // its lower end (weight w_lo), as its upper end (w_hi), or not at all
        float w = 0.f;
        bool mine = false;
        if (A.j + 1 < A.K && A.b_cur < l && l <= A.b_next) {
            w = (A.b_next / l - 1.f) / A.base_m1;
            mine = true;
        } else if (A.j > 0 && A.b_prev < l && l <= A.b_cur) {
            const float w_lo = (A.b_cur / l - 1.f) / A.base_m1;
            w = 1.f - w_lo;
            mine = true;
        }
        if (mine) o = make_float4(v.x * w, v.y * w, v.z * w, v.w * w);
    }
    A.out[i] = o;
}

constexpr uint32_t CS_TW = 32, CS_TH = 8, CS_HW = CS_TW + 2, CS_HH = CS_TH + 2, CS_PLANE = CS_HW * CS_HH;

struct CascadeReweightArgs {
    const float* beauty;  // nart_pixel image, totalW x totalH
    const float* layers;  // K such images back to back
    float* out;           // nart_pixel image; the border is zeroed by the caller
    uint32_t W, H, totalW, totalH, fb, K;
    float N, kappa;
    float b[CASCADE_MAX_LAYERS];
};

// Dynamic LDS: K planes of CS_PLANE floats.
__global__ __launch_bounds__(256) void k_cascade_reweight(CascadeReweightArgs A) {
    extern __shared__ float cs_lam[];
    const uint32_t x0 = blockIdx.x * CS_TW, y0 = blockIdx.y * CS_TH;
    const size_t img = (size_t)A.totalW * A.totalH * 5;
    for (uint32_t idx = threadIdx.x; idx < A.K * CS_PLANE; idx += blockDim.x) {
        const uint32_t k = idx / CS_PLANE, r = idx - k * CS_PLANE;
        const uint32_t hy = r / CS_HW, hx = r - hy * CS_HW;
        const int x = (int)(x0 + hx) - 1, y = (int)(y0 + hy) - 1;
        float lam = 0.f;
        if (x >= 0 && y >= 0 && x < (int)A.W && y < (int)A.H) {
            const size_t px = ((size_t)(y + A.fb) * A.totalW + (x + A.fb)) * 5;
            const float w = A.beauty[px + 4];
            if (w > 0.f) {
                const float* C = A.layers + k * img + px;
                const float l = cs_lum(C[0] / w, C[1] / w, C[2] / w);
                lam = l > 0.f ? l : 0.f;
            }
        }
        cs_lam[idx] = lam;
    }
    __syncthreads();
    const uint32_t tx = threadIdx.x % CS_TW, ty = threadIdx.x / CS_TW;
    const uint32_t x = x0 + tx, y = y0 + ty;
    if (x >= A.W || y >= A.H) return;
    const size_t px = ((size_t)(y + A.fb) * A.totalW + (x + A.fb)) * 5;
    float* o = A.out + px;
    const float w = A.beauty[px + 4];
    if (!(w > 0.f)) {
        o[0] = o[1] = o[2] = o[3] = o[4] = 0.f;
        return;
    }
    float r = A.layers[px] / w, g = A.layers[px + 1] / w, b = A.layers[px + 2] / w;
#pragma unroll
    for (uint32_t j = 1; j < CASCADE_MAX_LAYERS; ++j) {
        if (j >= A.K) break;
        float acc = 0.f, cnt = 0.f;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int qx = (int)x + dx, qy = (int)y + dy;
                if (qx < 0 || qy < 0 || qx >= (int)A.W || qy >= (int)A.H) continue;
                const float* q = cs_lam + (ty + 1 + dy) * CS_HW + (tx + 1 + dx);
                float s = q[(j - 1) * CS_PLANE] + q[j * CS_PLANE];
                if (j + 1 < A.K) s = s + q[(j + 1) * CS_PLANE];
                acc = acc + s;
                cnt = cnt + 1.f;
            }
        const float gm = ((acc * A.N) / A.b[j]) / cnt;
        const float t = gm / A.kappa;
        const float om = t < 1.f ? t : 1.f;
        const float* C = A.layers + j * img + px;
        r = r + om * (C[0] / w);
        g = g + om * (C[1] / w);
        b = b + om * (C[2] / w);
    }
    o[0] = r;
    o[1] = g;
    o[2] = b;
    o[3] = A.beauty[px + 3] / w;
    o[4] = 1.f;
}

}  // namespace nd
