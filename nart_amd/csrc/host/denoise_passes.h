// What the three a-trous denoisers (device/denoise.h, denoise_cross.h, denoise_parts.h) launch, in which
// order, between which signal buffers and into which timing slot, and how their work buffers are laid
// out -- decided from plain values (no HIP, no context, no environment).  image_stages.h walks a
// sequence with one driver (run_denoise_passes); tests/test_denoise_passes.py asserts what that driver
// and the kernels rely on.
#pragma once
#include <cstddef>
#include <cstdint>

#include "denoise_parts_plan.h"

namespace nd {

constexpr uint32_t DN_MAX_ITERATIONS = 8;  // denoise_params_error (stage_params.h): iterations in 1..8

// The timing slots of a run, as the nart_hip_denoise*_timings getters report them.
constexpr uint32_t DN_SLOT_PREPARE = 0, DN_SLOT_VARIANCE = 1, DN_SLOT_PASS0 = 2,
                   DN_SLOT_FINALIZE = DN_SLOT_PASS0 + DN_MAX_ITERATIONS, DN_SLOT_SUM = DN_SLOT_FINALIZE + 1,
                   DN_SLOTS = DN_SLOT_SUM + 1;

enum class DnKind : uint8_t { Prepare, Variance, Atrous, Finalize, Sum };

// One launch.  in / out: the ping-pong signal buffer (0 or 1) it reads / writes, -1 for none.
struct DnLaunch {
    DnKind kind;
    uint8_t halo;   // pixels of halo its blocks stage in LDS; 0: the taps are read from global memory
    uint8_t slot;   // the timing slot its interval is added to
    int8_t in, out;
    uint8_t chunk;  // parts denoise: the chunk of the PartsPlan it works on (0 elsewhere)
    uint32_t step;  // a-trous: 2^i; 1 elsewhere
};

// The halo of the a-trous pass of step 2^i: the taps reach 2 * 2^i pixels, which LDS holds for the
// first two passes; beyond them the tile's halo would outgrow the tile.
constexpr uint8_t dn_pass_halo(uint32_t i) { return i == 0 ? 2 : (i == 1 ? 4 : 0); }
constexpr uint8_t DN_VARIANCE_HALO = 3;  // the 7x7 window

// The most launches a sequence holds (the parts denoise at PARTS_MAX chunks of one part, DN_MAX_ITERATIONS
// passes and the sum), and the events around them: one before the first launch, one after each.
constexpr uint32_t DN_CHUNK_LAUNCHES = 1 + DN_MAX_ITERATIONS + 1;  // variance, passes, finalize
constexpr uint32_t DN_MAX_LAUNCHES = 1 + PARTS_MAX * DN_CHUNK_LAUNCHES + 1;
constexpr uint32_t DN_EVENT_BUDGET = DN_MAX_LAUNCHES + 1;

struct DnSequence {
    uint32_t n = 0;
    DnLaunch launch[DN_MAX_LAUNCHES] = {};
    void add(DnKind kind, uint8_t halo, uint32_t slot, int in, int out, uint32_t chunk = 0, uint32_t step = 1) {
        launch[n++] = {kind, halo, (uint8_t)slot, (int8_t)in, (int8_t)out, (uint8_t)chunk, step};
    }
};

// What follows prepare for the signals of one chunk: the variance kernel (buffer 0 -> 1) if there is
// one, the passes ping-ponging from buffer 1, finalize reading what the last pass wrote.
inline void dn_add_filter(DnSequence& s, uint32_t iterations, bool variance_kernel, uint32_t chunk) {
    if (variance_kernel) s.add(DnKind::Variance, DN_VARIANCE_HALO, DN_SLOT_VARIANCE, 0, 1, chunk);
    int cur = 1;
    for (uint32_t i = 0; i < iterations; ++i, cur ^= 1)
        s.add(DnKind::Atrous, dn_pass_halo(i), DN_SLOT_PASS0 + i, cur, cur ^ 1, chunk, 1u << i);
    s.add(DnKind::Finalize, 0, DN_SLOT_FINALIZE, cur, -1, chunk);
}

// The launches of one denoise of `iterations` passes (1..DN_MAX_ITERATIONS; anything else: none).
// Without the variance kernel (the sample-variance mode: prepare writes the variance itself) prepare
// writes buffer 1, where the variance kernel would have left the signal.
inline DnSequence plan_denoise_passes(uint32_t iterations, bool variance_kernel) {
    DnSequence s;
    if (iterations < 1 || iterations > DN_MAX_ITERATIONS) return s;
    s.add(DnKind::Prepare, 0, DN_SLOT_PREPARE, -1, variance_kernel ? 0 : 1);
    dn_add_filter(s, iterations, variance_kernel, 0);
    return s;
}

// The launches of a parts denoise: prepare once for all parts, the rest of the sequence once per chunk
// of the plan (their intervals add up in their slots), and the sum of the outputs if asked for.
inline DnSequence plan_denoise_parts_passes(const PartsPlan& plan, uint32_t iterations, bool sum) {
    DnSequence s;
    if (iterations < 1 || iterations > DN_MAX_ITERATIONS || !plan.n_chunks) return s;
    s.add(DnKind::Prepare, 0, DN_SLOT_PREPARE, -1, 0);
    for (uint32_t j = 0; j < plan.n_chunks; ++j) dn_add_filter(s, iterations, true, j);
    if (sum) s.add(DnKind::Sum, 0, DN_SLOT_SUM, -1, -1);
    return s;
}

// The work buffer of a denoise over npx cropped pixels, as planes of npx elements: the float4 planes
// first (so that each is 16-byte aligned whatever npx is), then the float planes.
//   float4: guide, centre (a_d; with alpha where there is one image), signal [ping-pong][n_sig]
//   float:  cov, slope, alpha [n_alpha] (the parts' alphas: one per part)
struct DnWorkLayout {
    uint32_t n_sig, n_alpha;
    constexpr uint32_t guide() const { return 0; }
    constexpr uint32_t centre() const { return 1; }
    constexpr uint32_t sig(uint32_t pingpong, uint32_t c) const { return 2 + pingpong * n_sig + c; }
    constexpr uint32_t n4() const { return 2 + 2 * n_sig; }
    constexpr uint32_t cov() const { return 0; }
    constexpr uint32_t slope() const { return 1; }
    constexpr uint32_t alpha(uint32_t k) const { return 2 + k; }
    constexpr uint32_t n1() const { return 2 + n_alpha; }
    constexpr size_t bytes_per_pixel() const { return 16 * (size_t)n4() + 4 * (size_t)n1(); }
    // byte offsets of a plane in the buffer
    constexpr size_t off4(uint32_t plane, size_t npx) const { return 16 * npx * plane; }
    constexpr size_t off1(uint32_t plane, size_t npx) const { return 16 * npx * n4() + 4 * npx * plane; }
};
constexpr DnWorkLayout DN_WORK_PLAIN = {1, 0}, DN_WORK_CROSS = {2, 0};
constexpr DnWorkLayout dn_work_parts(uint32_t K) { return {K, K}; }

}  // namespace nd
