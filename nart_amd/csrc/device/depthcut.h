// Depth cuts (include/nart_hip.h, "Depth cuts"): the layers between the cut images.  The cut records
// themselves are the path kernel's own (kernels.h k_render_rq with DC) and reach their images through
// the plain splat and combine.
//   k_depth_layers   per pixel of the totalW x totalH image and channel c of r, g, b:
//                    layer_0 = I_0;  layer_j = I_j - I_{j-1};  layer_K = beauty - I_{K-1};
//                    alpha and filter_weight_sum of every layer copied from the beauty
// One lane per pixel, no LDS, no atomics; one float32 subtraction per layer and channel:
// tests/depthcut_py.py restates it in numpy bit for bit.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace nd {

constexpr uint32_t DEPTH_CUTS_MAX = 8;

struct DepthLayersArgs {
    const float* cuts;    // K nart_pixel images back to back
    const float* beauty;  // nart_pixel image
    float* out;           // K + 1 nart_pixel images back to back
    uint32_t W, H, totalW, totalH, fb, K;
};

__global__ __launch_bounds__(256) void k_depth_layers(DepthLayersArgs A) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n = (uint64_t)A.totalW * A.totalH;
    if (i >= n) return;
    const size_t img = (size_t)n * 5, px = (size_t)i * 5;
    const float alpha = A.beauty[px + 3], wsum = A.beauty[px + 4];
    float prev[3] = {0.f, 0.f, 0.f};
    for (uint32_t j = 0; j <= A.K; ++j) {
        const float* cur = (j < A.K ? A.cuts + (size_t)j * img : A.beauty) + px;
        float* o = A.out + (size_t)j * img + px;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = cur[c];
            o[c] = j ? v - prev[c] : v;  // (layer_0 is I_0 itself: no 0 subtracted, so -0 stays -0)
            prev[c] = v;
        }
        o[3] = alpha;
        o[4] = wsum;
    }
}

}  // namespace nd
