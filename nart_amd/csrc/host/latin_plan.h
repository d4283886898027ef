// Which form of the LatinSquare a batch runs, where its scratch arrays lie and how its kernels are
// launched, decided once from plain values (no HIP, no context, no environment): render.hip launch_latin
// calls plan_latin, offsets five pointers into the record buffer and launches; tests/test_latin_plan.py
// compares plan_latin with a restatement and asserts that the arrays, with the words the kernels read
// ahead, lie apart and inside the buffer.
//
// LatinSquare per traced pixel: float arrays in LDS up to 256 spp, LDS index shuffles up to 1024
// spp (scratch in Lout: 2*spp floats per lane of every launched block, within Lout's 4*spp per
// slot once there are >= 64 slots), the global-memory variant beyond.  From 65 to 1024 spp the
// three-kernel form (k_latin_draws / _perm / _emit) runs instead where its scratch fits in Lout
// (C3, 256 spp: 6.7 -> 4.6 ms; k_latin_idx at <= 256 spp measured slower: 11.0 vs 6.6 ms).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../device/sample_layout.h"

namespace nd {

enum class LatinForm { Three, Lds, Idx, Global };  // k_latin_draws + _perm + _emit, k_latin_lds, k_latin_idx, k_latin

struct Grid {
    uint32_t blocks = 0, threads = 0;
    size_t lds = 0;  // dynamic LDS of a block
};

struct LatinPlan {
    LatinForm form = LatinForm::Global;
    uint32_t n2 = 0;  // (spp + 1) / 2 word rows (LatinScratch::n2)
    // Three: each of cx, cy, sx, sy takes `words` u32 words, the states st take `stw`; the arrays start
    // at these word offsets of the record buffer
    size_t words = 0, stw = 0;
    size_t cx = 0, cy = 0, sx = 0, sy = 0, st = 0;
    uint32_t perm_block = 64;  // lanes of a k_latin_perm block: its template argument
    Grid draws, perm, emit;    // Three
    Grid one;                  // the single kernel of the other forms
};

inline LatinPlan plan_latin(uint32_t n_slots, uint32_t spp, size_t sample_capacity_bytes) {
    LatinPlan p;
    const uint32_t groups = (n_slots + 63) / 64;
    const uint32_t emit_blocks = (n_slots + LATIN_EMIT_SLOTS - 1) / LATIN_EMIT_SLOTS;
    p.n2 = (spp + 1) / 2;
    // + padding rows per array: k_latin_perm / k_latin_emit load a batch of words ahead,
    // unconditionally
    p.words = (size_t)groups * 64 * p.n2 + (size_t)std::max(NART_LATIN_PF, 2 * LATIN_EMIT_U * 16) * 64;
    p.stw = (size_t)emit_blocks * LATIN_EMIT_SLOTS * spp + LATIN_ST_PAD;
    if (spp > 64 && spp <= 1024 && (4 * p.words + p.stw) * 4 <= sample_capacity_bytes) {
        p.form = LatinForm::Three;
        p.cy = p.words, p.sx = 2 * p.words, p.sy = 3 * p.words, p.st = 4 * p.words;
        p.draws = Grid{(n_slots + 255) / 256, 256, 0};
        // a lane's u16 column of [2 n2] indices: one 64-lane block per CU is all the LDS holds above 640
        // spp, where 80 lanes fill it
        p.perm_block = (size_t)p.n2 * 4 * 128 > 160 * 1024 ? 80 : 64;
        p.perm = Grid{(n_slots + p.perm_block - 1) / p.perm_block, p.perm_block,
                      (size_t)p.n2 * 2 * p.perm_block * sizeof(uint16_t)};
        p.emit = Grid{emit_blocks, 256, (size_t)spp * LATIN_EMIT_SLOTS * sizeof(uint32_t)};
    } else if (spp <= 256) {
        p.form = LatinForm::Lds;
        p.one = Grid{groups, 64, (size_t)spp * 2 * 64 * sizeof(float)};
    } else if (spp <= 1024 && n_slots >= 64) {
        p.form = LatinForm::Idx;  // both index arrays up to 512 spp, one beyond (two passes)
        p.one = Grid{groups, 64, (size_t)spp * (spp <= 512 ? 2 : 1) * 64 * sizeof(uint16_t)};
    } else {
        p.one = Grid{(n_slots + 255) / 256, 256, 0};
    }
    return p;
}

}  // namespace nd
