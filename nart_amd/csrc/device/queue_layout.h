// Layout of the probe-ordered pixel queue (render.hip k_build_queue, host/path_schedule.h), as one
// function of the queue position that host and device share (tests/test_path_schedule.py checks it
// on the CPU).
#pragma once
#include <cstdint>

#ifdef __HIP__
#define NART_HD __host__ __device__
#else
#define NART_HD
#endif

// flag bits of a queue entry (k_render_rq strips them from the slot)
#define RQ_PRIO_BIT 0x80000000u
#define RQ_PAIR_BIT 0x40000000u
#define RQ_QUAD_BIT 0x20000000u  // with RQ_PAIR_BIT: the pixel's group has four lanes, not rq_pairs

namespace nd {

// Entries of the queue over n slots: every costly pixel (k per first-round wave, W waves) takes
// `pairs` lanes instead of one, and with quad each wave's costliest pixel two more.
NART_HD inline uint32_t queue_length(uint32_t n, uint32_t W, uint32_t k, uint32_t pairs, uint32_t quad) {
    return n + (pairs ? (pairs - 1u) * k * W : 0u) + (quad ? 2u * W : 0u);
}

struct QueueEntry {
    uint32_t top;    // 1: entry `index` of the costly pixels (by rank); 0: of the rest (slot order)
    uint32_t index;
    uint32_t flags;  // RQ_*_BIT, or'ed into the slot
};

// Queue: in the first round of W waves, lanes j < k of wave w take the costly pixel of rank
// j*W + w (each wave holds k of them); every other position takes the remaining pixels in
// slot order (spatially coherent waves).
// With prio set (k_render_rq) the costly entries carry RQ_PRIO_BIT; with pairs = Q (2 or 4) each
// costly pixel goes to Q adjacent lanes (Qj .. Qj + Q - 1) with RQ_PAIR_BIT too, and the queue is
// n + (Q - 1)*k*W long.  p < queue_length(n, W, k, pairs, quad).
NART_HD inline QueueEntry queue_entry(uint32_t p, uint32_t n, uint32_t W, uint32_t k, uint32_t prio, uint32_t pairs,
                                      uint32_t half, uint32_t quad) {
    (void)n;
    const uint32_t per = pairs ? pairs : 1u, kk = per * k;  // first-round lanes of the costly pixels
    const uint32_t g = 64u * W, pair = pairs ? RQ_PAIR_BIT : 0u;
    if (p < g && quad) {
        // quad: each first-round wave's costliest pixel (ranks 0..W-1) on four lanes, its other k-1
        // costly pixels on pairs
        const uint32_t w = p / 64u, j = p % 64u, kq = kk + 2u;
        if (j < 4u) return {1u, w, prio | RQ_PAIR_BIT | RQ_QUAD_BIT};
        if (j < kq) return {1u, ((j - 4u) / per + 1u) * W + w, prio | RQ_PAIR_BIT};
        return {0u, w * (64u - kq) + (j - kq), 0u};
    }
    if (p >= g && quad) return {0u, (64u - kk - 2u) * W + (p - g), 0u};
    if (p < g && half) {
        // half = BW, the waves of a ray-queue block (8 or 12: PB = 2 or 3 per SIMD): only its first 4
        // waves hold costly pixels (PB k each), so each SIMD has one priority wave
        const uint32_t BW = half, PB = BW / 4u;
        const uint32_t w = p / 64u, j = p % 64u, b = w / BW, i = w % BW, k2 = PB * kk;
        const uint32_t pw = b * 4u + i;  // priority wave index
        const uint32_t roff = b * BW * (64u - kk) + (i < 4u ? i * (64u - k2) : 4u * (64u - k2) + (i - 4u) * 64u);
        if (i < 4u && j < k2) return {1u, (j / per) * (W / PB) + pw, prio | pair};
        return {0u, roff + (i < 4u ? j - k2 : j), 0u};
    }
    if (p < g) {
        const uint32_t w = p / 64u, j = p % 64u;
        if (j < kk) return {1u, (j / per) * W + w, prio | pair};
        return {0u, w * (64u - kk) + (j - kk), 0u};
    }
    return {0u, (64u - kk) * W + (p - g), 0u};
}

}  // namespace nd
