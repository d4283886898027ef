// How a call splats, decided once from plain values (no HIP, no context, no environment): the filter
// tables (splat_thresholds, splat_lut), which splat kernel runs and with which sample layout (plan_splat),
// the shape of its launch over a batch (splat_launch) and the call-constant kernel arguments
// (splat_scalars).  render.hip plan_splat reads the knobs and the CU count, uploads the tables and calls
// these; launch_splat_as finds the instantiation a SplatLaunch names and launches it.
// tests/test_splat_plan.py compares plan_splat with a restatement of the policy and asserts what the
// kernels rely on in every splat_launch; tests/test_abi.py checks the tables through the C ABI.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../device/sample_layout.h"
#include "path_schedule.h"  // Knob, NART_SCHED_*

namespace nd {

// ---------------------------------------------------------------- filter tables
// Filter index of AddSample (render.cpp:43-49) as a function of d2 = distX^2 + distY^2:
// fi(d2) = min(63, uint8(RN(RN(sqrt(d2)) / fw) * 64)).  sqrt and / are correctly rounded and the
// scaling by 64 is exact, so below the uint8 wrap fi is a non-decreasing step function of d2 and
// fi(d2) >= k  <=>  d2 >= thr[k].  thr[0] = 0, thr[64] = inf; thr[k] is found by bisection over the
// float bit patterns with the same float operations.  A splat hit has |distX|, |distY| <= fw + 0.5,
// so the thresholds are exact for every hit when RN(sqrt(2) (fw + 0.5) / fw) * 64 stays below 256
// (fw > ~0.28); otherwise returns false and the splat keeps the direct computation.
inline uint32_t filter_index_host(float d2, float fw) {
    volatile float dist = std::sqrt(d2);
    volatile float q = dist / fw;
    return std::min(63u, (uint32_t)(int32_t)(q * 64.f) & 0xFFu);
}

inline bool splat_thresholds(float fw, float thr[65]) {
    if (!(fw > 0.f)) return false;
    const float hmax = fw + 0.5f;
    const double worst = std::sqrt(2.0 * (double)hmax * hmax) / fw * 64.0;
    if (!(worst < 250.0)) return false;
    const float d2max = 2.f * hmax * hmax * 1.001f;
    uint32_t hi_bits;
    std::memcpy(&hi_bits, &d2max, 4);
    thr[0] = 0.f;
    thr[64] = __builtin_inff();
    for (uint32_t k = 1; k < 64; ++k) {
        uint32_t lo = 0, hi = hi_bits;  // f(lo) < k <= f(hi) unless no hit reaches index k
        if (filter_index_host(d2max, fw) < k) {
            thr[k] = __builtin_inff();
            continue;
        }
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            float m;
            std::memcpy(&m, &mid, 4);
            if (filter_index_host(m, fw) >= k) hi = mid;
            else lo = mid;
        }
        std::memcpy(&thr[k], &hi, 4);
        if (filter_index_host(0.f, fw) >= k) thr[k] = 0.f;
    }
    return true;
}

// One cell of the filter-weight table; the kernels read it as a float4 (render.hip asserts the size).
struct LutCell {
    float t, below, above, pad;  // the threshold inside the cell (or inf), the weights below / from it
};

// Filter weight by d2 cell for the splat (k_splat_col4<.., true>): cell c covers the floats whose
// bits >> 16 equal b0 + c (128 cells per octave of d2).  Consecutive thresholds differ by at
// least a factor (64/63)^2 = 1.03 > 1 + 1/128, so a cell holds at most one threshold t: the
// filter index in the cell is base + (d2 >= t), base = fi(cell start).  Cell 0 lies wholly below
// thr[1] (index 0 for every smaller d2 too); the last cell starts past thr[63] (index 63 beyond).
// Stored per cell: {t (or inf), table[base], table[base + 1]}.  Returns false when the thresholds
// do not apply (then the splat keeps the sqrt estimate) or a cell would hold two of them.
inline bool splat_lut(const float thr[65], const float table[64], std::vector<LutCell>& lut, uint32_t& b0) {
    uint32_t u1, u63;
    std::memcpy(&u1, &thr[1], 4);
    std::memcpy(&u63, &thr[63], 4);
    if (!(thr[1] > 0.f) || !(thr[63] < __builtin_inff())) return false;
    b0 = (u1 >> 16) - 1;
    const uint32_t last = (u63 >> 16) + 1;
    const uint32_t n = last - b0 + 1;
    if (n > SPLAT_LUT_MAX) return false;
    lut.assign(n, LutCell{0.f, 0.f, 0.f, 0.f});
    for (uint32_t c = 0; c < n; ++c) {
        const uint32_t lo = (b0 + c) << 16, hi = lo | 0xFFFFu;
        float flo, fhi;
        std::memcpy(&flo, &lo, 4);
        std::memcpy(&fhi, &hi, 4);
        uint32_t base = 0, inside = 0;
        float t = __builtin_inff();
        for (uint32_t k = 1; k < 64; ++k) {
            if (thr[k] <= flo) base = k;
            else if (thr[k] <= fhi) {
                ++inside;
                t = thr[k];
            }
        }
        if (inside > 1) return false;
        lut[c] = LutCell{t, table[std::min(base, 63u)], table[std::min(base + inside, 63u)], 0.f};
    }
    return true;
}

// ---------------------------------------------------------------- which kernel
struct SplatIn {
    int mode = -1;         // the context's splat mode (nart_hip_set_splat_mode, NART_SPLAT_MODE); -1: the default
    bool volume = false;   // the volume integrator (else the path integrator)
    uint32_t B = 16, fb = 2, tile = 20;  // bucket size, filter bounds, tile = B + 2 fb
    uint32_t n_buckets = 0;              // buckets of the whole call
    uint32_t n_cus = 1;                  // compute units of the device
    bool lut_ok = false;                 // splat_lut applies to the filter width
    bool small_col4 = false;             // NART_SPLAT_SMALL=col4: small launches take k_splat_col4
    Knob skew_bands;                     // NART_SKEW_BANDS: 1 or 2 forces the band count
};

// Splat modes (all bit-identical): 5 / 4 skewed time (k_splat_rows / k_splat_skew), 3 four tile pixels per
// lane (k_splat_col4, power-of-two buckets), 1 / 0 one tile pixel per lane with the threshold / direct
// filter-index arithmetic (k_splat, any bucket size; 2 selects 1 since the compare-only one-pixel kernel
// was retired).
struct SplatChoice {
    int mode = 0;
    bool skew = false;   // a pixel-major sample layout, for k_splat_skew (mode 4) or k_splat_rows (mode 5)
    bool rows = false;   // k_splat_rows
    uint32_t bands = 1;  // tile-row bands per bucket (k_splat_skew's NB)
};

constexpr double SKEW_MIN_WAVES = 2.0;  // waves per SIMD from which k_splat_skew runs one band per bucket

// Waves of a k_splat_skew launch with one band per bucket: floor(64 / tile) buckets share a wave.
inline double skew_waves(uint32_t tile, uint32_t n_buckets) {
    return tile >= 1 && tile <= 64 ? (double)((n_buckets + 64 / tile - 1) / (64 / tile)) : 0.0;
}

inline SplatChoice plan_splat(const SplatIn& in) {
    // skewed-time splat (k_splat_skew, pixel-major samples) where its preconditions hold, else
    // k_splat_col4 / k_splat over the sample-major layout
    // It runs one lane per tile column for ~W*B steps, so its time is one wave's latency once the
    // launch has fewer than ~2 waves per SIMD: small shards keep k_splat_col4 (C5 1/8 shard:
    // 54 ms skewed vs 23 ms col4; whole frame 72 vs 113 ms).  SKEW_MIN_WAVES: waves per SIMD.
    const double waves = skew_waves(in.tile, in.n_buckets), simds = 4.0 * in.n_cus;
    // splat mode -1 (default): 4 where the launch is large enough, else 3; an explicit 4 forces it.
    // Launches of 1-2 waves per SIMD split each bucket's tile rows into two bands (twice the waves
    // for ~2/3 of the steps each): C5 1/2 shard 60 -> 49 ms (k_splat_col4: 62); a whole frame keeps
    // one band (C5 73 vs 92 ms with two).  Below 1 wave per SIMD k_splat_col4 is faster (C5 1/4,
    // 1/8 shards: 36 / 23 ms vs 41 / 37 with two bands; profiles/r03k_skew_band_ab.log).
    // The two-band range is the volume integrator's only: for the path integrator the splat's
    // gain at the C3 1/2 shard (17 -> 12.5 ms) is within the path kernels' run-to-run spread under
    // the pixel-major layout (186-208 ms on one box; profiles/r03l_c3_half_shard_splat_ab.log).
    const double skew_from = in.volume ? 0.5 * SKEW_MIN_WAVES : SKEW_MIN_WAVES;
    // Below that, k_splat_rows (mode 5: W lanes per tile column, five times k_splat_skew's
    // parallelism, each sample still fetched once per bucket) unless NART_SPLAT_SMALL=col4
    const int small_mode = in.small_col4 ? 3 : 5;
    SplatChoice c;
    c.mode = in.mode >= 0 ? in.mode : (waves >= skew_from * simds ? 4 : small_mode);
    const int forced = (int)in.skew_bands.or_(0.0);
    c.bands = forced > 0 ? (forced >= 2 ? 2u : 1u) : (waves >= SKEW_MIN_WAVES * simds ? 1u : 2u);
    c.skew = c.mode >= 4 && in.lut_ok && (in.B & (in.B - 1)) == 0 && in.B <= 32 && in.tile <= 64 && in.fb >= 1 &&
             in.fb <= 3;
    c.rows = c.skew && c.mode == 5;
    return c;
}

// ---------------------------------------------------------------- the launch over a batch
enum class SplatKernel { Rows, Skew, Col4, Pixel };

// One launch of a splat kernel over the nbk buckets of a batch: the kernel and its template values
// (k_splat_rows<fb, MOM>, k_splat_skew<fb, bands, MOM>, k_splat_col4<NART_SPLAT_NP, lut, MOM>,
// k_splat<thr, MOM>), its grid and the schedule bit it reports.
struct SplatLaunch {
    SplatKernel kernel = SplatKernel::Pixel;
    uint32_t fb = 0, bands = 1;  // Rows, Skew
    bool lut = false;            // Col4: weights from the filter cells
    bool thr = false;            // Pixel: the filter index from the thresholds, else computed directly
    uint32_t per_block = 1;      // Rows, Skew: buckets (Skew: bucket bands) of one block
    uint32_t blocks = 0, threads = 256;
    size_t lds = 0;      // dynamic LDS of a block
    uint32_t sched = 0;  // NART_SCHED_SPLAT_*
};

inline SplatLaunch splat_launch(const SplatChoice& c, uint32_t fb, uint32_t tile, bool thr_ok, bool invB_ok,
                                uint32_t lut_cells, uint32_t nbk) {
    SplatLaunch l;
    const size_t lut_bytes = (size_t)lut_cells * sizeof(LutCell);
    if (c.rows) {
        // tile * (2 fb + 1) lanes per bucket, as many whole buckets as 512 lanes hold, whole waves; behind
        // the filter cells two flag words per bucket of the block
        const uint32_t U = tile * (2 * fb + 1);
        l.kernel = SplatKernel::Rows;
        l.fb = fb;
        l.per_block = std::max(1u, 512u / U);
        l.threads = (l.per_block * U + 63) / 64 * 64;
        l.blocks = (nbk + l.per_block - 1) / l.per_block;
        l.lds = lut_bytes + 2u * l.per_block * sizeof(uint32_t);
        l.sched = NART_SCHED_SPLAT_ROWS;
    } else if (c.skew) {
        // a band of a bucket is tile lanes, floor(64 / tile) of them per wave, four waves per block; two
        // flag words per unit
        const uint32_t pb = 64u / tile;
        l.kernel = SplatKernel::Skew;
        l.fb = fb;
        l.bands = c.bands;
        l.per_block = 4 * pb;
        l.blocks = (nbk * c.bands + l.per_block - 1) / l.per_block;
        l.lds = lut_bytes + 2u * l.per_block * sizeof(uint32_t);
        l.sched = NART_SCHED_SPLAT_SKEW;
    } else if (thr_ok && invB_ok && c.mode >= 3) {
        // a lane per NART_SPLAT_NP rows of a tile column
        const uint64_t n4 = (uint64_t)nbk * tile * ((tile + NART_SPLAT_NP - 1) / NART_SPLAT_NP);
        l.kernel = SplatKernel::Col4;
        l.lut = lut_cells != 0;
        l.blocks = (uint32_t)((n4 + 255) / 256);
    } else {
        // a lane per tile pixel
        const uint64_t lanes = (uint64_t)nbk * tile * tile;
        l.kernel = SplatKernel::Pixel;
        l.thr = thr_ok && c.mode >= 1;
        l.blocks = (uint32_t)((lanes + 255) / 256);
    }
    return l;
}

// ---------------------------------------------------------------- call-constant kernel arguments
// The scalars of SplatArgs (kernels.h) that hold for a whole call; render.hip adds the device pointers
// and, per batch, the bucket count.
struct SplatScalars {
    float idx_scale = 0.f;  // 64 / fw: the estimate of the filter index that the thresholds correct
    uint32_t spp = 0, B = 0, fb = 0, tile = 0, nbx = 0, totalW = 0, totalH = 0;
    float fw = 0.f;
    float invB = 0.f, invFw = 0.f;  // exact reciprocals when B / fw are powers of two, else 0
    uint32_t lut_b0 = 0, lut_n = 0;
};

inline SplatScalars splat_scalars(float fw, uint32_t spp, uint32_t B, uint32_t fb, uint32_t tile, uint32_t nbx,
                                  uint32_t totalW, uint32_t totalH, uint32_t lut_b0, uint32_t lut_n) {
    SplatScalars s;
    s.idx_scale = 64.f / fw;
    s.spp = spp, s.B = B, s.fb = fb, s.tile = tile, s.nbx = nbx, s.totalW = totalW, s.totalH = totalH;
    s.fw = fw;
    s.invB = (B & (B - 1)) == 0 ? 1.f / (float)B : 0.f;
    int ex = 0;
    s.invFw = std::frexp(fw, &ex) == 0.5f ? 1.f / fw : 0.f;
    s.lut_b0 = lut_b0, s.lut_n = lut_n;
    return s;
}

}  // namespace nd
