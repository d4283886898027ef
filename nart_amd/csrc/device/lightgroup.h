// Light groups (include/nart_hip.h, "Light groups"): the mix of the group images.  The group records
// themselves are the path kernel's own (kernels.h k_render_rq with LG) and reach their images through
// the plain splat and combine.
//   k_light_mix   per pixel of the totalW x totalH image: per channel c of r, g, b
//                 acc = 0.f; for g ascending: acc = acc + gains[g][c] * I_g.contribution[c];
//                 alpha and filter_weight_sum copied from I_0
// One lane per pixel, no LDS, no atomics; one float32 multiply and one float32 add per group and
// channel, built without contraction: tests/lightgroup_py.py restates it in numpy bit for bit.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace nd {

constexpr uint32_t LIGHT_GROUPS_MAX = 8;

struct LightMixArgs {
    const float* groups;  // G nart_pixel images back to back
    float* out;           // nart_pixel image
    uint32_t W, H, totalW, totalH, fb, G;
    float gains[LIGHT_GROUPS_MAX][3];
};

__global__ __launch_bounds__(256) void k_light_mix(LightMixArgs A) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n = (uint64_t)A.totalW * A.totalH;
    if (i >= n) return;
    const size_t img = (size_t)n * 5, px = (size_t)i * 5;
    float acc[3] = {0.f, 0.f, 0.f};
    for (uint32_t g = 0; g < A.G; ++g) {
        const float* k = A.groups + (size_t)g * img + px;
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = acc[c] + A.gains[g][c] * k[c];
    }
    float* o = A.out + px;
    o[0] = acc[0];
    o[1] = acc[1];
    o[2] = acc[2];
    o[3] = A.groups[px + 3];
    o[4] = A.groups[px + 4];
}

}  // namespace nd
