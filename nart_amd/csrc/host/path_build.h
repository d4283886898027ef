// Which build of the path kernels a launch runs and the LDS layout it runs with, decided once from plain
// values (no HIP, no context, no environment): render.hip dispatch_megakernel reads the knobs and the
// occupancy of k_render, calls plan_build, finds the build's instantiation of launch_render in its table
// and launches it; tests/test_path_build.py compares plan_build with a restatement of the policy and
// asserts what the product of plan_build and plan_path (host/path_schedule.h) can never give.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../device/path_layout.h"
#include "path_schedule.h"

namespace nd {

// Scene-specialised builds of the path kernels (k_render_rq, k_primary): glassSphere's (C3:
// Lambert + glass, one kind of area light, constant patterns), the Cornell box's (C2: Lambert,
// disk) and the textured environment-lit plastic of C4.  A render takes the first build whose mask
// covers the scene's; others, the counter pass and renders with bounces > ILIST_REG
// run the generic build.  Same operations per kind, so every build renders the same image
// (tests/test_gpu_specialize.py compares them on every suite scene).
constexpr uint32_t FM_DIFFUSE = FT_LAMBERT | FT_DISK;
constexpr uint32_t FM_GLASS = FT_LAMBERT | FT_GLASS | FT_DISK;
constexpr uint32_t FM_ENVTEX = FT_LAMBERT | FT_PLASTIC | FT_ENV | FT_TEX | FT_NMAP;

constexpr size_t CU_LDS_BYTES = (size_t)160 * 1024;  // LDS of a gfx950 compute unit

enum class Specialize { Off, On, Lean };  // nart_hip_set_specialize 0 / 1 / 2 (the default)

struct PathBuildIn {
    uint32_t features = FT_ALL;  // the scene's feature mask (scene_features)
    bool has_env = false;        // the scene has an environment light
    Specialize specialize = Specialize::Lean;
    bool counters = false;  // the counter pass
    // the light-group build (include/nart_hip.h, "Light groups"): always the generic two-wave build without
    // priority lanes, on the ray-queue kernel only
    bool light_groups = false;
    // the depth-cut build (include/nart_hip.h, "Depth cuts"): the light groups' rule
    bool depth_cuts = false;
    // the cost build (include/nart_hip.h, "Cost image"): the light groups' rule
    bool cost = false;
    uint32_t bounces = 0;
    int variant = 0;  // 0: the ray-queue kernel where its LDS fits; 3: k_render
    uint32_t stack_depth = 1, num_nodes = 0;  // of the scene's BVH
    uint32_t n_slots = 0;
    uint32_t resident_k = 1;  // resident 256-lane blocks of k_render on the device
    // test hooks (none changes an image): NART_RQ_LDS_LIMIT, NART_LEAN_STACK, NART_LEAN_ROUNDS
    Knob rq_lds_limit, lean_stack, lean_rounds;
};

// The template arguments of one build of k_render / k_render_rq / k_primary (render.hip's table).
struct BuildId {
    bool ext = false, count = false, env = false;
    uint32_t fm = FT_ALL;
    int wv = 2;
    bool pr = true;
    bool lg = false;  // the light-group build of k_render_rq
    bool dc = false;  // the depth-cut build of k_render_rq
    bool cs = false;  // the cost build of k_render_rq
    bool operator==(const BuildId& o) const {
        return ext == o.ext && count == o.count && env == o.env && fm == o.fm && wv == o.wv && pr == o.pr && lg == o.lg &&
               dc == o.dc && cs == o.cs;
    }
};

struct LdsLayout {
    uint32_t nodes = 0;  // top BVH nodes staged behind the kernel's fixed part
    size_t bytes = 0;    // dynamic LDS of a block
};

struct PathBuild {
    const char* error = nullptr;  // a layout that cannot be launched (NART_E_INVALID)
    bool unsupported = false;     // the error is a combination that has no kernel (NART_E_UNSUPPORTED)
    BuildId id;
    bool rq = false;             // the ray-queue kernel runs, else k_render
    uint32_t rq_block = 512;     // lanes of a ray-queue block
    uint32_t stack_lds = 1;      // traversal-stack levels the ray-queue kernel keeps in LDS
    LdsLayout k_render, rq_lds;  // k_render (the cost probe, the fallback); the ray-queue kernel
    uint32_t fm_used = FT_ALL;   // the feature mask of the kernel that traces the paths
};

// Top BVH nodes staged in what `fixed` bytes leave of `budget`.
inline uint32_t staged_nodes(uint32_t num_nodes, size_t fixed, size_t budget) {
    const size_t n = budget > fixed ? (budget - fixed) / node_lds_bytes(1) : 0;
    return (uint32_t)std::min<size_t>(n, num_nodes);
}

// LDS of one k_render block: the traversal stack + as many top BVH nodes as fit while
// NART_RENDER_WAVES blocks share a CU's LDS.  Every k_render build has this layout (the occupancy
// query of dispatch_megakernel needs it before plan_build's other inputs are known).
inline LdsLayout k_render_layout(uint32_t stack_depth, uint32_t num_nodes) {
    const size_t stack = (size_t)stack_depth * 256 * 8;
    LdsLayout l;
    l.nodes = staged_nodes(num_nodes, stack, CU_LDS_BYTES / NART_RENDER_WAVES);
    l.bytes = stack + node_lds_bytes(l.nodes);
    return l;
}

// Traversal-stack levels the lean build keeps in LDS: all of them where the 768-lane block's LDS
// then still stages 320 BVH nodes (or the whole BVH), else as many as leave room for them (>= 4;
// deeper levels go to per-thread global columns).  C3 (14 levels, 759 nodes): 8 levels and 352
// nodes; 7 / 8 / 10 levels measured 241 / 241 / 245 ms per frame, +-7 ms run to run
// (profiles/r06e_lean_stack_ab.log).  NART_LEAN_STACK (tests) forces a depth.
inline uint32_t lean_stack_levels(const PathBuildIn& in) {
    if (in.lean_stack.set)
        return std::max<uint32_t>(1u, std::min<uint32_t>(in.stack_depth, (uint32_t)in.lean_stack.or_(1.0)));
    const size_t nodes = node_lds_bytes(std::min<uint32_t>(in.num_nodes, 320u));
    uint32_t k = in.stack_depth;
    while (k > 4 && rq_lds_bytes(k, 768) + nodes > CU_LDS_BYTES) --k;
    return k;
}

inline PathBuild plan_build(const PathBuildIn& in) {
    PathBuild b;
    b.k_render = k_render_layout(in.stack_depth, in.num_nodes);
    // variant 0: ray-queue kernel; 3: k_render (one lane per pixel, the fallback below).
    // The ray-queue kernel's 512-lane blocks keep a stack_depth * 4 KiB traversal stack plus
    // 60 KiB of outboxes, results and id rings in LDS, one block per CU: a BVH deeper than 25 levels
    // does not fit, and those scenes run k_render (256-lane blocks, stack_depth * 2 KiB) instead --
    // same image.  NART_RQ_LDS_LIMIT lowers the budget (tests of the fallback).
    const size_t limit = (size_t)std::min(in.rq_lds_limit.or_((double)CU_LDS_BYTES), (double)CU_LDS_BYTES);
    b.rq = in.variant == 0 && rq_lds_bytes(in.stack_depth, NART_RQ_BLOCK) <= limit;

    // the build: the first specialised mask that covers the scene's, else the generic one
    BuildId& id = b.id;
    id.env = in.has_env;
    const uint32_t f = in.features;
    auto covers = [f](uint32_t m) { return (f & ~m) == 0u; };
    if (in.light_groups) {
        // Priority lanes and speculative pairs hold a sample's result pending and may drop it: a group
        // frame does without them (pr = false: small shards run the plain schedule) rather than make
        // its G records droppable.  The counter pass has no light-group build: its counts are those of
        // a plain render of the frame.
        id.lg = true;
        if (!b.rq) {
            b.error = "light groups need the ray-queue kernel: not variant 3, nor a BVH deeper than its LDS holds";
            b.unsupported = true;
        }
    } else if (in.depth_cuts) {
        // As for light groups: a pending result that may be dropped would make the cut records droppable
        // too, and the counter pass has no depth-cut build.
        id.dc = true;
        if (!b.rq) {
            b.error = "depth cuts need the ray-queue kernel: not variant 3, nor a BVH deeper than its LDS holds";
            b.unsupported = true;
        }
    } else if (in.cost) {
        // As for light groups: work that may be dropped (a doomed speculative job's rays) would enter the
        // traversal steps, which must depend on the sample alone, and the counter pass has no cost build:
        // its records are the counts.
        id.cs = true;
        if (!b.rq) {
            b.error = "the cost image needs the ray-queue kernel: not variant 3, nor a BVH deeper than its LDS holds";
            b.unsupported = true;
        }
    } else if (in.specialize != Specialize::Off && !in.counters && in.bounces <= ILIST_REG) {
        if (!in.has_env && covers(FM_DIFFUSE)) id.fm = FM_DIFFUSE;
        else if (!in.has_env && covers(FM_GLASS)) id.fm = FM_GLASS;
        else if (in.has_env && covers(FM_ENVTEX)) id.fm = FM_ENVTEX;
    }
    if (id.fm == FT_ALL) {
        // a path grows the dielectric list by at most one entry per bounce: the register list alone
        // serves bounces <= ILIST_REG; deeper ones (up to 32) spill it to the per-lane columns
        id.ext = in.bounces > ILIST_REG;
        id.count = in.counters && !id.lg && !id.dc && !id.cs;
        if (id.lg || id.dc || id.cs) id.pr = false;
    } else {
        // The lean three-waves-per-SIMD build (kernels.h WV = 3) for throughput-bound launches.  It raises
        // throughput (C3 whole frame, 16 rounds of resident waves: path kernels 276.6 -> ~241 ms; C4 4K
        // frame and its 1/8 shards, 8 rounds: 492 -> 456 ms) but each of its waves runs slower, which
        // lengthens the serial sample chains of a scene's costliest pixels.  Glass scenes' chains (caustic
        // paths behind the dielectric) set the time of their smaller launches, where the two-wave build
        // stays faster (C3 1/2 and 1/4 shards, 8 and 4 rounds: 172-185 / 114 ms vs 202-206 / 131 ms lean;
        // profiles/r06k_lean_rounds_ab.log), so they take it from 12 rounds on, other scenes from 3.
        // Glass scenes' small launches are bound by their costly pixels' chains, which the priority
        // lanes of the two-wave build shorten (C3 1/2, 1/4 shards: 183 / 115 ms two-wave vs 194 / 130
        // lean); scenes without glass or an environment light take the lean build from 1.5 rounds
        // (C2 1/8 shards, 2 rounds: mean 22.1 vs 23.9 ms, profiles/r06zg_c2_shard8.log).
        // Small shards keep two waves per SIMD: the priority-lane build at three (WV = 3, PR = true: no
        // launch takes it), 168 VGPRs with 14 spilled, measured C3 1/8 shards worst 83-85 vs 79-81 ms,
        // mean 79.5-79.8 vs 75.9-76.0 (profiles/r06l_three_wave_prio_ab.log).
        // The rounds are those of k_render's resident waves, as in plan_path (NART_LEAN_ROUNDS, tests,
        // replaces the threshold).  b.rq tests the 512-lane layout against the limit although the lean
        // block has 768 lanes: a 768-lane layout that does not fit (only NART_LEAN_STACK can force one)
        // is refused by the range check below, which is what keeps this test sufficient.
        const double from = (in.features & FT_GLASS) ? 12.0 : (in.has_env ? 3.0 : 1.5);
        if (b.rq && in.specialize == Specialize::Lean && rounds_of(in.n_slots, in.resident_k) >= in.lean_rounds.or_(from)) {
            id.wv = 3;
            id.pr = false;
        }
    }
    b.fm_used = b.rq ? id.fm : FT_ALL;  // every k_render build is generic

    // The ray-queue kernel, one block per CU (2 or 3 waves per SIMD): outbox, results and id lists take
    // part of the LDS; the lean build keeps lean_stack_levels there and the rest in a global column per
    // thread; the top BVH nodes fill what is left.  (Staging them for k_primary too measured slower: a
    // wave's coherent rays read the same node, which the L1 broadcasts: 9.7 vs 8.2 ms at 64 spp)
    b.rq_block = RQ_BLOCK_OF(id.count, id.wv);
    b.stack_lds = id.wv == 3 ? lean_stack_levels(in) : in.stack_depth;
    const size_t fixed = rq_lds_bytes(b.stack_lds, b.rq_block);
    b.rq_lds.nodes = staged_nodes(in.num_nodes, fixed, CU_LDS_BYTES);
    b.rq_lds.bytes = fixed + node_lds_bytes(b.rq_lds.nodes);
    if (!b.error && b.rq && (b.stack_lds < 1 || b.stack_lds > in.stack_depth || b.rq_lds.bytes > CU_LDS_BYTES))
        b.error = "ray-queue LDS layout out of range";
    return b;
}

}  // namespace nd
