// Half buffers (include/nart_hip.h, "Half buffers", nart_hip_render_halves): the device kernel.
//   k_half_split   per sample record: the record of half h -- the sample's colour with weight 1 where
//                  the sample's index has parity h, all zero else -- into a second per-sample record
//                  buffer that the plain splat kernels then consume
//
// k_half_split runs one lane per record along the sample layout (dense in both sample orders, as
// k_moment and k_cascade_split rely on): no LDS, no atomics, consecutive lanes read and write
// consecutive 16-byte records.  It runs once per half per batch.
//
// The sample index i of record r (i is the sample's index 0..spp-1 in its pixel's sequence, the s of
// kernels.h sample_index), in the two orders k_slot_table lays a batch out in:
//   pixel-major   slot t keeps sample s at t * spp + s, so                    i = r mod spp;
//   sample-major  slot base_b + p of bucket b, which has cnt_b = base_{b+1} - base_b traced pixels
//                 (base_{nbk} = n_slots), keeps sample s at base_b * spp + s * cnt_b + p with p < cnt_b.
//                 Bucket b's records are therefore [base_b * spp, base_{b+1} * spp), the bases ascend,
//                 and b is the last bucket with base_b * spp <= r (a bucket without traced pixels has
//                 an empty range and the search passes it: cnt_b > 0 for the b found, since r lies in
//                 its range).  Then                                            i = (r - base_b * spp) / cnt_b.
// The search is a bisection over the batch's bucket bases: at most 32 loads of a table that the
// lanes of a wave share.
//
// The colour is copied, not multiplied: a non-finite colour reaches exactly one half, and the other
// half's record is a literal zero.  The splat's fourth accumulator L.w * w then sums the filter weights
// of the half's own samples, and its fifth, w alone, those of all samples: the beauty's
// filter_weight_sum.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace nd {

struct HalfSplitArgs {
    const float4* L;              // the batch's Li_alpha records
    float4* out;                  // half h's records
    uint64_t n;                   // records: n_slots * spp
    const uint32_t* bucket_base;  // [nbk] first slot of every bucket of the batch, ascending (sample-major)
    uint32_t nbk, n_slots, spp;
    uint32_t h;                   // the parity this half keeps
    uint32_t pixel_major;         // the batch's sample order (k_slot_table)
};

// The sample index of record r: see the derivation above.
__device__ __forceinline__ uint32_t half_sample_index(const HalfSplitArgs& A, uint64_t r) {
    if (A.pixel_major) return (uint32_t)(r % A.spp);
    uint32_t lo = 0, hi = A.nbk;  // base[lo] * spp <= r, and base[hi] * spp > r (hi == nbk: n_slots * spp = n > r)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if ((uint64_t)A.bucket_base[mid] * A.spp <= r) lo = mid;
        else hi = mid;
    }
    const uint32_t base = A.bucket_base[lo];
    const uint32_t end = lo + 1 < A.nbk ? A.bucket_base[lo + 1] : A.n_slots;
    return (uint32_t)((r - (uint64_t)base * A.spp) / (end - base));
}

__global__ __launch_bounds__(256) void k_half_split(HalfSplitArgs A) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= A.n) return;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((half_sample_index(A, r) & 1u) == A.h) {
        const float4 v = A.L[r];
        o = make_float4(v.x, v.y, v.z, 1.0f);
    }
    A.out[r] = o;
}

}  // namespace nd
