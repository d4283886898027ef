// First-hit ID mattes (include/nart_hip.h, nart_hip_render_mattes): the three device kernels.
//   k_matte_ids      per sample record: the four coverage indicators of one plane, from the sample's
//                    first-hit triangle, into the per-sample record buffer that the plain splat
//                    kernels then consume
//   k_matte_rank     per cropped-image pixel: the R greatest positive coverages and their ids
//   k_matte_extract  per cropped-image pixel: the summed coverage of an id set, from the rank images
//
// k_matte_ids runs one lane per record along the sample layout (dense in both sample orders, as
// k_moment and k_cascade_split rely on): hit[i] -> tri_mesh -> (mesh table) -> id, no traversal, no
// fill_isect, no LDS, no atomics.  It runs once per plane per batch.
//
// k_matte_rank works on 32 x 8-pixel tiles in 256-thread blocks, lanes along x.  Every lane divides
// its pixel's 4 P coverages once and keeps them in LDS, [id][lane] (4 P x 256 floats: 32 KB at 32
// ids; a lane's column is its own, so no barrier and no bank conflict), then selects R times over
// them with a bit mask of the ids already taken.  No cross-lane reduction and no atomics: the result
// is a pure function of the inputs, whatever the launch shape.
//
// The arithmetic is one float32 divide per coverage, float32 adds in k_matte_extract, and
// comparisons, built without contraction: tests/matte_py.py restates it in numpy bit for bit.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "dscene.h"

namespace nd {

constexpr uint32_t MATTE_MAX_IDS = 32, MATTE_MAX_PLANES = 8, MATTE_MAX_RANKS = 8;
constexpr uint32_t MATTE_MESH = 0, MATTE_MATERIAL = 1;

struct MatteIdArgs {
    const uint32_t* hit;       // first-hit triangle per sample (k_primary), 0xFFFFFFFF: a miss
    const uint32_t* tri_mesh;  // DScene::tri_mesh
    const DMesh* meshes;       // DScene::meshes
    float4* out;               // plane q's records
    uint64_t n;                // records
    uint32_t num_tris, num_meshes;
    uint32_t kind, q, n_ids;
};

__global__ __launch_bounds__(256) void k_matte_ids(MatteIdArgs A) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const uint32_t g = A.hit[i];
    uint32_t id = 0xFFFFFFFFu;
    if (g < A.num_tris) {  // a miss (0xFFFFFFFF) has no id
        const uint32_t mesh = A.tri_mesh[g];
        if (mesh < A.num_meshes) id = A.kind == MATTE_MATERIAL ? A.meshes[mesh].material : mesh;
    }
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (id < A.n_ids) {
        const uint32_t b = 4u * A.q;
        o.x = id == b ? 1.f : 0.f;
        o.y = id == b + 1u ? 1.f : 0.f;
        o.z = id == b + 2u ? 1.f : 0.f;
        o.w = id == b + 3u ? 1.f : 0.f;
    }
    A.out[i] = o;
}

constexpr uint32_t MT_TW = 32, MT_TH = 8, MT_LANES = MT_TW * MT_TH;

struct MatteRankArgs {
    const float* planes;  // P nart_pixel images back to back, totalW x totalH (null with no ids)
    float* out;           // R / 2 such images; the border is zeroed by the caller
    uint32_t W, H, totalW, totalH, fb;
    uint32_t n_ids, R;
};

// Dynamic LDS: 4 * ceil(n_ids / 4) rows of MT_LANES floats.
__global__ __launch_bounds__(256) void k_matte_rank(MatteRankArgs A) {
    extern __shared__ float mt_cov[];
    const uint32_t tx = threadIdx.x % MT_TW, ty = threadIdx.x / MT_TW;
    const uint32_t x = blockIdx.x * MT_TW + tx, y = blockIdx.y * MT_TH + ty;
    if (x >= A.W || y >= A.H) return;
    const size_t img = (size_t)A.totalW * A.totalH * 5;
    const size_t px = ((size_t)(y + A.fb) * A.totalW + (x + A.fb)) * 5;
    const uint32_t P = (A.n_ids + 3u) / 4u;
    const float w = P ? A.planes[px + 4] : 0.f;
    const bool ok = w > 0.f;
    float* cov = mt_cov + threadIdx.x;
    if (ok)
        for (uint32_t q = 0; q < P; ++q) {
            const float* C = A.planes + q * img + px;
            cov[(4u * q) * MT_LANES] = C[0] / w;
            cov[(4u * q + 1u) * MT_LANES] = C[1] / w;
            cov[(4u * q + 2u) * MT_LANES] = C[2] / w;
            cov[(4u * q + 3u) * MT_LANES] = C[3] / w;
        }
    uint32_t taken = 0;
    for (uint32_t r = 0; r < A.R; ++r) {
        float best = 0.f;
        uint32_t bm = 0xFFFFFFFFu;
        if (ok)
            for (uint32_t m = 0; m < A.n_ids; ++m) {
                const float c = cov[m * MT_LANES];
                // c > best >= 0: zero, negative and NaN coverages never rank; among equals the least m stays
                if (!((taken >> m) & 1u) && c > best) {
                    best = c;
                    bm = m;
                }
            }
        float* o = A.out + (size_t)(r / 2u) * img + px;
        if (bm != 0xFFFFFFFFu) {
            taken |= 1u << bm;
            o[2u * (r & 1u)] = (float)bm;
            o[2u * (r & 1u) + 1u] = best;
        } else {
            o[2u * (r & 1u)] = -1.f;
            o[2u * (r & 1u) + 1u] = 0.f;
        }
        if (r & 1u) o[4] = 1.f;
    }
}

struct MatteExtractArgs {
    const float* ranks;  // R / 2 nart_pixel images back to back
    float* out;          // nart_pixel image; the border is zeroed by the caller
    uint32_t W, H, totalW, totalH, fb, R;
    uint64_t mask;
};

__global__ __launch_bounds__(256) void k_matte_extract(MatteExtractArgs A) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)A.W * A.H) return;
    const uint32_t y = (uint32_t)(i / A.W), x = (uint32_t)(i - (uint64_t)y * A.W);
    const size_t img = (size_t)A.totalW * A.totalH * 5;
    const size_t px = ((size_t)(y + A.fb) * A.totalW + (x + A.fb)) * 5;
    float m = 0.f;
    for (uint32_t r = 0; r < A.R; ++r) {
        const float* k = A.ranks + (size_t)(r / 2u) * img + px + 2u * (r & 1u);
        const float id = k[0];
        if (id >= 0.f && id < 64.f && ((A.mask >> (uint32_t)id) & 1ull)) m = m + k[1];
    }
    float* o = A.out + px;
    o[0] = o[1] = o[2] = o[3] = m;
    o[4] = 1.f;
}

}  // namespace nd
