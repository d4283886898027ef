// What the path kernels and the host's choice of their build (host/path_build.h plan_build) share, as
// plain C++ that compiles with and without HIP: the scene feature mask, the size of the dielectric
// list's register part, the block sizes and the LDS layouts.  tests/test_path_build.py checks the
// arithmetic on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>

#include "queue_layout.h"  // NART_HD

namespace nd {

// Scene feature mask (template parameter FM of the shading functions and k_render_rq): the
// material, light and pattern kinds a scene holds (scene_features, render.hip).  A kernel built
// for a mask compiles only those kinds' code -- no plastic lobes, ring lights, texture fetches or
// normal-map frames in glassSphere's build -- and serves every scene whose mask it covers; FT_ALL
// is the generic build.  Each kind's operations are unchanged, so every build renders the same bits.
enum : uint32_t {
    FT_LAMBERT = 1u << 0,   // diffusematerial.cpp
    FT_SPECMAT = 1u << 1,   // specularmaterial.cpp
    FT_GLASS = 1u << 2,     // glassmaterial.cpp
    FT_GLOSSY = 1u << 3,    // glossydielectricmaterial.cpp
    FT_PLASTIC = 1u << 4,   // plasticmaterial.cpp (the only two-lobe BSDF)
    FT_DISK = 1u << 5,      // disklight.cpp
    FT_RING = 1u << 6,      // ringlight.cpp
    FT_ENV = 1u << 7,       // environmentlight.cpp
    FT_TEX = 1u << 8,       // any TexturePattern (materials or light Le)
    FT_NMAP = 1u << 9,      // any material with a normal map
    FT_ALL = (1u << 10) - 1u
};

// ---------------------------------------------------------------- nested-dielectric list
// IntersectionInfo list (pathintegrator.h:9-19, pathintegrator.cpp:7-36, 123-142).  The first
// ILIST_REG entries live in registers (every access an unrolled compare/select, no dynamic
// indexing); a path can only grow the list by one entry per bounce, so renders with bounces <=
// ILIST_REG never need more.  With EXT (bounces up to 32) entries ILIST_REG.. live in a per-lane
// column of global memory, entry k at x[(k - ILIST_REG) * xs] as {id, eta bits}: deep nesting is
// rare, so the kernels keep the register footprint of the short list and spill nothing (the
// former 16- and 32-entry register lists spilled 50-97 VGPRs to scratch on every access).
#define ILIST_REG 10
#define ILIST_MAX 32

// ---------------------------------------------------------------- BVH nodes staged in LDS
// LDS-staged nodes, 64 B each (a 16-B pad after every 4 nodes measured C3 276.3 -> 282.5 ms,
// C4 51.9 -> 51.6 ms and was retired, profiles/r05ae_node_pad_ab.txt).  node_slot: first float4 of
// node i.
NART_HD inline uint32_t node_slot(uint32_t i) { return 4u * i; }
NART_HD inline size_t node_lds_bytes(uint32_t n) { return (size_t)16 * (n ? node_slot(n - 1u) + 4u : 0u); }

// ---------------------------------------------------------------- blocks of the path kernels
// k_render: min waves per SIMD requested from the register allocator.  Without it the allocator takes
// >256 registers (VGPR + AGPR) once the environment-light code is inlined and the kernel drops
// to 1 wave/SIMD (C3 at 64 spp: 260 ms vs 151 ms at 2 waves; 3 waves spills: 178 ms).
#ifndef NART_RENDER_WAVES
#define NART_RENDER_WAVES 2
#endif

// The ray-queue kernel's fixed LDS per wave (kernels.h k_render_rq): the traversal stack, the outbox,
// the results and two 256-entry rings of queued (lane, kind) ids.
#define RQ_RING 256u
NART_HD inline size_t rq_lds_bytes(uint32_t stack_depth, uint32_t block) {
    const uint32_t waves = block / 64;
    return (size_t)stack_depth * block * 8 + (size_t)waves * 3 * 64 * 32 + (size_t)block * 16 +
           (size_t)waves * 2 * RQ_RING;
}

// 512-thread blocks: one block of 8 waves per CU shares one copy of the staged BVH nodes (twice
// as many nodes in LDS).  With the wave-group refill (no wave waits for its block) C3 392 vs
// 407 ms per frame (profiles/r02m_rq_block_ab.log); before it, blocks retiring as a whole made
// 256 faster (132.6 vs 121.5 ms at 64 spp)
#ifndef NART_RQ_BLOCK
#define NART_RQ_BLOCK 512
#endif
// The counter pass (COUNT: untimed; its path counts are per accepted sample and do not depend on the
// schedule, its traversal counts include the speculative lanes' dropped work) runs
// 256-lane blocks at one wave per SIMD, so its counters do not push the kernel past 256 VGPRs.
//
// WV = 3: the lean throughput build for launches of >= 3 rounds of resident waves (whole frames),
// which never use priority lanes or speculative pairs: that code and its state compiled out, 768-lane
// blocks (12 waves per CU) at three waves per SIMD; only for scenes whose specialised build fits
// 168 VGPRs and whose traversal stack fits the block's LDS (host/path_build.h plan_build).
#define RQ_BLOCK_OF(COUNT, WV) ((COUNT) ? 256 : ((WV) == 3 ? 768 : NART_RQ_BLOCK))

}  // namespace nd
