// How the K parts of a parts denoise (device/denoise_parts.h) are cut into the chunks its kernels take,
// decided from plain values (no HIP, no context, no environment).  render.hip reads the one knob,
// NART_DN_PARTS_CHUNK, once per call and hands it in; tests/test_denoise_parts_plan.py asserts what the
// launches rely on for every K and every knob value.
#pragma once
#include <cstdint>

namespace nd {

constexpr uint32_t PARTS_MAX = 9;   // NART_DENOISE_PARTS_MAX, device DNP_MAX_PARTS
constexpr uint32_t PARTS_CHUNK_MAX = 4;  // device DNP_MAX_CHUNK

// The chunks in launch order: chunk j holds the parts first[j] .. first[j] + size[j] - 1.  Every part is
// in exactly one chunk, the parts ascend through the chunks, every size is in 1..4.
struct PartsPlan {
    uint32_t n_chunks = 0;
    uint32_t first[PARTS_MAX] = {}, size[PARTS_MAX] = {};
};

// The chunk size the automatic choice uses for K parts (index K; 0 unused): per K the forced size that
// measured fastest, where it beat the next smaller size by more than the run-to-run spread (DESIGN.md,
// "Denoised parts", A: 1920x1080, default parameters, device ms of the stage, median of 5, spread <= 3%):
//     K   K x denoise   size 1   size 2   size 3   size 4
//     2      1.894      2.023    1.453      =        =
//     3      2.838      3.020    2.460    2.054      =
//     4      3.778      4.073    2.936    3.070    2.860
//     8      7.594      8.129    5.842    5.638    5.694
//     9      8.531      9.072    6.878    6.188    6.661
// ("=": the same plan as the size to its left.)  Three parts per launch cost least per part (0.68 ms; two
// 0.73, four 0.72, one 1.01): at four the passes that read global memory need 111 VGPRs (4 waves per
// SIMD) and the LDS passes 3 blocks per CU.  K = 5, 6, 7 were not measured; their sizes are those with the least sum
// of the measured chunk costs (3+2, 3+3, 4+3), a sum that predicts the measured K = 8 and 9 within 2%.
constexpr uint32_t PARTS_AUTO_CHUNK[PARTS_MAX + 1] = {0, 1, 2, 3, 4, 3, 3, 4, 3, 3};

// K parts (1..9; anything else: no chunks) in chunks of `knob` parts (NART_DN_PARTS_CHUNK: 1..4), the
// last one ragged; knob 0 (unset) or out of range: the automatic size for K.
inline PartsPlan plan_denoise_parts(uint32_t K, uint32_t knob) {
    PartsPlan plan;
    if (K < 1 || K > PARTS_MAX) return plan;
    const uint32_t c = knob >= 1 && knob <= PARTS_CHUNK_MAX ? knob : PARTS_AUTO_CHUNK[K];
    for (uint32_t k = 0; k < K; k += c) {
        plan.first[plan.n_chunks] = k;
        plan.size[plan.n_chunks++] = K - k < c ? K - k : c;
    }
    return plan;
}

}  // namespace nd
