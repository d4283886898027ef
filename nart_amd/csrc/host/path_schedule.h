// The schedule of one path-kernel launch, decided once from plain values (no HIP, no context, no
// environment): render.hip launch_render reads the knobs and the occupancy, calls plan_path and executes
// what it returns; tests/test_path_schedule.py compares plan_path with a restatement of the policy.
// The volume integrator's launch is decided the same way at the end of this file (plan_volume and
// sparse_hot_groups, executed by dispatch_volume, compared by tests/test_path_build.py); which build of
// the path kernels runs, in host/path_build.h.
//
// A pixel's samples are one serial chain (its RNG stream), so a frame can finish no earlier than its
// costliest pixels, and a wave of 64 costly pixels runs several times longer than one such pixel alone
// (the wave executes the union of its lanes' work).  With the work queue the grid is persistent: lanes
// take pixels from a queue ordered by a cost probe (one sample per pixel), the costliest pixels spread
// over all waves so that each holds only a few of them, and a lane whose pixel is done takes the next one
// instead of idling until its wave ends.  The image is unchanged (each pixel keeps its own RNG stream).
#pragma once
#include <algorithm>
#include <cstdint>

#include "../../../include/nart_hip.h"
#include "../device/queue_layout.h"

#ifndef NART_RQ_GROUP_LANES
#define NART_RQ_GROUP_LANES 2
#endif
// traversal-phase quorum of throughput-bound ray-queue launches: the phase ends once the wave's queue is
// empty and at most this many lanes still trace (0/4/16/32: 134.7/123.5/123.0/129.9 vs 121.6 ms at 8)
#ifndef NART_RQ_QUORUM
#define NART_RQ_QUORUM 8u
#endif

namespace nd {

// One environment knob: present at all (`set`, even when empty), and its number when not empty.
struct Knob {
    bool set = false, has = false;
    double v = 0.0;
    double or_(double def) const { return has ? v : def; }
};
// The test hooks of the path schedule (none changes an image): NART_PRIMARY_PACKET, NART_RQ_PRIO, _PAIRS,
// _HALF, _QUAD, _SETPRIO, _ORDER, _TOPF, NART_PROBE_SUB, NART_QUEUE_K.
struct SchedKnobs {
    Knob primary_packet, rq_prio, rq_pairs, rq_half, rq_quad, rq_setprio, rq_order, rq_topf, probe_sub, queue_k;
};

struct PathLaunchIn {
    uint32_t n_slots = 0;
    uint32_t resident_k = 1;   // resident 256-lane blocks of k_render on the device
    uint32_t resident_rq = 1;  // resident lanes / 256 of the ray-queue kernel (whole rq_block blocks), if rq
    uint32_t rq_block = 512;   // lanes of a ray-queue block (kernels.h RQ_BLOCK_OF)
    int wv = 2;                // waves per SIMD of the ray-queue build (3: the lean build)
    bool pr = true, env = false;  // the build has priority lanes; environment-light build
    bool rq = false;           // the ray-queue kernel runs (variant 0 and its LDS layout fits), else k_render
    bool specialized = false;  // a scene-specialised build
    bool has_prim = false;     // there is a camera-hit buffer to fill (and this is no cost probe)
};

enum class PathShape {
    Direct,             // one lane per pixel, slot order, no queue
    Groups,             // persistent ray-queue grid, waves take 64-slot groups (ghead / gorder)
    PixelQueue,         // cost probe, the k W costliest pixels dealt over the first round, refill
    WholeGroupsByCost,  // k = 64: one lane per pixel, the groups launched costliest first
};
enum class PathProbe { None, EveryPixel, Sampled };

struct PathSchedule {
    const char* error = nullptr;  // a broken invariant (nothing may be launched)
    PathShape shape = PathShape::Direct;
    bool primary = false;  // k_primary first, as wave packets if `packet`
    uint32_t packet = 0;
    uint32_t resident = 0, W = 0;  // resident blocks of 256 lanes of the kernel launched, its waves
    uint32_t queue_room = 0;       // entries the queue buffers must hold (0: no queue buffers needed)
    PathProbe probe = PathProbe::None;
    uint32_t probe_sub = 64, probe_blocks = 0;      // pixels probed per 64-slot group; the probe's launch
    uint32_t order = 0, E = 0;  // Groups: 0 slot order, 1 costliest first, 2 the E costliest groups first
    uint32_t k = 0, pairs = 0, half = 0, quad = 0;  // PixelQueue layout (queue_entry)
    uint32_t rq_prio = 0, rq_setprio = 0, rq_quorum = 0, qlen = 0, qbase = 0;
    uint32_t blocks = 0;  // final launch, in blocks of 256 lanes
    uint32_t sched = 0;   // NART_SCHED_* bits
};

// Rounds of resident waves a launch of n slots spans, given the resident blocks of 256 lanes.
inline double rounds_of(uint32_t n_slots, uint32_t resident) { return (double)n_slots / (64.0 * 4.0 * resident); }

// Groups.  Many rounds: the slot order (costly waves interleaved with cheap ones in time) measured
// faster than any reordering of pixels.  The ray-queue kernel runs it on a persistent grid whose waves
// take wave-sized slot groups (one wave per group, blocks retiring as a whole: 422 vs 407 ms,
// profiles/r02h_env_ab.log).
inline void plan_groups(PathSchedule& s, const PathLaunchIn& in, const SchedKnobs& kn, double R) {
    const uint32_t ng = (in.n_slots + 63u) / 64u;
    s.shape = PathShape::Groups;
    s.sched |= NART_SCHED_WAVE_GROUPS;
    s.blocks = std::min(s.blocks, s.resident);
    // group order (NART_RQ_ORDER): 0 slot order; 1 costliest group first (cost probe); 2 the NART_RQ_TOPF
    // % (default 10) costliest groups first, each class in slot order.  In slot order the costly groups
    // (behind the glass) taken last left a tail: at 90 % of the C3 launch only 25 of 2,048 waves were
    // still running (WAVEPROF timeline).  C3 frame 445 -> 407 ms (probe included; order 1: 408, top 20 /
    // 35 %: 408 / 408 ms).  The lean build's slower waves leave a longer tail behind the costly groups
    // taken late: fully cost-ordered groups (1) measured C3 227.5 vs 235-247 ms for the costliest 10 %
    // first (2), 250 / 245 / 260 ms for 5 / 20 / 35 %, slot order 299 (profiles/r06r_group_order_ab.log),
    // C2 75 vs 77 ms; C4's environment-light frame keeps 2 (4K/128: 609 vs 624 ms,
    // r06s_group_order_c4_c2.log).  The two-wave build's launches of 6-12 rounds (C3 1/2 shard,
    // chain-bound) also take 1: worst rank 183-184 -> 167-169 ms (profiles/r06x_mid_shards.log)
    const int order = (int)kn.rq_order.or_(!in.env ? 1.0 : 2.0);
    if (order != 1 && order != 2) return;
    s.order = (uint32_t)order;
    // cost probe: the first sample of NART_PROBE_SUB (default 8) evenly spaced pixels of every 64-slot
    // group (64: every pixel).  Only the group order depends on it (costliest NART_RQ_TOPF % first), and
    // that order is not sensitive to the estimate (TOPF 10 / 20 / 35 %: 407 / 408 / 408 ms).  Launches of
    // fewer than 12 rounds of resident waves probe every pixel: there a costly group the sample missed
    // and took late sets the tail (C4 1/8 shards, 8 rounds: worst rank 488-496 ms probing every pixel,
    // 552-556 ms sampled; profiles/r05ah_c4_probe_ab.log)
    uint32_t sub = (uint32_t)kn.probe_sub.or_(R >= 12.0 ? 8.0 : 64.0);
    if (sub != 1u && sub != 2u && sub != 4u && sub != 8u && sub != 16u && sub != 32u) sub = 64u;
    s.probe_sub = sub;
    s.probe = sub < 64u ? PathProbe::Sampled : PathProbe::EveryPixel;
    s.probe_blocks = sub < 64u ? (ng * sub + 255u) / 256u : (in.n_slots + 255u) / 256u;
    if (order == 2) s.E = (uint32_t)std::min<double>(ng, std::max(0.0, kn.rq_topf.or_(10.0)) * 0.01 * ng);
}

inline PathSchedule plan_path(const PathLaunchIn& in, const SchedKnobs& kn) {
    PathSchedule s;
    const uint32_t n = in.n_slots;
    const bool rq = in.rq;
    if (rq && in.specialized) s.sched |= NART_SCHED_SPECIALIZED;
    if (rq && in.wv == 3 && !in.pr) s.sched |= NART_SCHED_LEAN;
    // camera rays first, coherently (k_primary; leaving them to the path kernel measured C3 470 vs 407 ms
    // per frame, profiles/r02h_env_ab.log), as wave packets (path.h traverse_packet; C3 -1.7 ms, C4 -31 ms
    // per frame, profiles/r04_primary_packet_ab.log); NART_PRIMARY_PACKET=0: one ray per lane
    s.primary = rq && in.has_prim;
    s.packet = kn.primary_packet.or_(1.0) != 0.0 ? 1u : 0u;
    if (s.primary) s.sched |= NART_SCHED_PRIMARY;
    // rounds of resident waves (of k_render: the same figure for every build, so that the choice of the
    // lean build and this launch's thresholds agree)
    const double R = rounds_of(n, in.resident_k);
    // resident blocks of 256 lanes of the kernel this launch runs: the ray-queue kernel holds one 512- or
    // 768-lane block per CU, so its persistent grid and the waves the queue deals its first round over
    // are its own (the lean build has 1.5x k_render's resident lanes)
    s.resident = rq ? in.resident_rq : in.resident_k;
    const uint32_t W = s.W = s.resident * 4u;
    // rounds from which a launch counts as throughput-bound: traversal-phase quorum 8, no priority lanes
    // or speculative pairs.  Below, quorum 0 (every queued ray resolved before the path phase): the
    // costliest pixels' chains set a small shard's time (1/8 C3 shard: 100.5 -> 96.0 ms)
    const double q_rounds = 3.0;
    s.rq_quorum = R >= q_rounds ? NART_RQ_QUORUM : 0u;
    s.blocks = (n + 255u) / 256u;
    if (s.blocks <= s.resident) return s;  // every pixel has a resident lane

    // more pixels than resident lanes: persistent grid + queue, with room for the speculative groups'
    // duplicates: qlen = n + (Q - 1) * k * W with Q * k <= 64
    s.queue_room = n + 63u * W;
    // Priority lanes for the costly pixels in the ray-queue kernel (NART_RQ_PRIO=0: off, 2: also on
    // launches of >= 3 rounds), run as speculative lane groups of Q lanes (NART_RQ_PAIRS: 0 one lane per
    // pixel, 1 or 2 pairs, 4 groups of four).  Only small shards (< 3 rounds of resident waves), whose
    // time is their costliest pixels' chains: on throughput-bound launches the priority breaks and the
    // speculative duplicates cost throughput (1/2 C3 shard 238 -> 249 ms, C4 batches 3175 -> 3381 ms)
    const int prio_env = (int)kn.rq_prio.or_(1.0);
    const bool prio_on = prio_env == 2 || (prio_env == 1 && R < q_rounds);
    const int pe = (int)kn.rq_pairs.or_(NART_RQ_GROUP_LANES);
    const uint32_t Q = pe <= 0 ? 0u : (pe >= 4 ? 4u : 2u);
    // (the lean build has no priority lanes: it runs only where prio_on is false anyway)
    const bool prio = rq && prio_on && in.pr;
    // Half waves (default): the costly pixels only on the first 4 waves of each ray-queue block (8 or 12
    // waves), PB = 2 or 3 shares each -- one such wave per SIMD -- and those waves at a raised issue
    // priority (s_setprio 2, NART_RQ_SETPRIO) while they hold priority work, so the SIMD's other waves
    // fill their stalls instead of sharing issue with them.  C3 1/8 shard, every rank: mean 84.2 -> 80.9
    // ms, worst 87-92 -> 86.0 ms (profiles/r05h_chain_schedule_ab.log).  NART_RQ_HALF=0: every wave.
    const uint32_t BW = in.rq_block / 64u, PB = BW / 4u;
    // costly pixels per first-round wave: few when the shard is small (their serial chains bound the
    // frame), all 64 (packed, launched first) when there are many rounds.  C3 1/8 shard, mean of the 8
    // ranks with half waves at k = 4/6/8/12/14/16 per two-wave block share: 95.2/88.8/81.4/80.9/81.3/81.6
    // ms; three-wave blocks keep the same number of costly pixels (k W constant: 8 per share).  The half
    // layout is settled first, so a configuration it does not fit falls back to k = 8 dealt over every
    // wave.
    const uint32_t k_half = PB == 2u ? 12u : 8u;
    const bool half = prio && kn.rq_half.or_(1.0) != 0.0 && (W % BW) == 0u && R < 3.0 &&
                      PB * ((Q && Q * k_half <= 64u) ? Q : 1u) * k_half <= 64u;
    // ray-queue kernel: wave-group refill from 6 rounds of resident waves (C3 1/2 shard, 8 rounds: 241 ->
    // 235 ms; C4 batches, ~9 rounds: 1385 -> 1566 Msamples/s).  Below that a wave of costly groups
    // outlasts the rest (1/4 shard, 4 rounds: 146 -> 211 ms; with the groups cost-ordered still 156 vs
    // 114 ms), and the probe-ordered pixel queue with priority lanes stays.  The lean build (from 3 rounds
    // where it runs: scenes without glass) takes groups from there: C2 1/4 shard 32.2 -> 27.9 ms
    // (profiles/r06x_mid_shards.log).  k_render launches 12 rounds or more as they are, in slot order.
    const double g_rounds = in.wv == 3 ? 3.0 : 6.0;
    if (R >= (rq ? g_rounds : 12.0) && !kn.queue_k.set) {
        if (rq) plan_groups(s, in, kn, R);
        return s;
    }
    s.k = R >= 3.0 ? 32u : (half ? k_half : 8u);
    if (kn.queue_k.set) s.k = (uint32_t)std::max(1.0, std::min(64.0, kn.queue_k.or_(8.0)));
    const uint32_t k = s.k;
    s.probe = PathProbe::EveryPixel;  // the first sample of every pixel
    s.probe_blocks = s.blocks;
    s.shape = k == 64u ? PathShape::WholeGroupsByCost : PathShape::PixelQueue;
    if (k == 64u) return s;  // whole groups, costliest first (coherent waves, longest chains first)
    s.sched |= NART_SCHED_PROBE_QUEUE;
    s.pairs = (prio && Q && Q * k <= 64u) ? Q : 0u;
    const bool hw = half && PB * (s.pairs ? s.pairs : 1u) * k <= 64u;  // (again: NART_QUEUE_K may have changed k)
    // NART_RQ_QUAD (A/B): each first-round wave's costliest pixel gets four lanes
    s.quad = (prio && s.pairs == 2u && 2u * k + 2u <= 64u && kn.rq_quad.or_(0.0) != 0.0) ? 1u : 0u;
    s.half = hw && !s.quad ? BW : 0u;
    s.qlen = queue_length(n, W, k, s.pairs, s.quad);
    s.rq_prio = prio ? 1u : 0u;
    s.rq_setprio = prio ? (uint32_t)std::max(0.0, kn.rq_setprio.or_(hw ? 1.0 : 0.0)) : 0u;
    if (s.half) s.sched |= NART_SCHED_HALF_WAVES;
    if (prio) s.sched |= NART_SCHED_PRIORITY;
    if (s.pairs) s.sched |= NART_SCHED_SPEC_PAIRS;
    // whole ray-queue blocks, so that every first-round lane's entry lies below qbase
    const uint32_t per = rq ? in.rq_block / 256u : 1u;
    s.blocks = (s.resident + per - 1u) / per * per;
    s.qbase = s.blocks * 256u;
    // the size ensure_queue is called with must hold the queue
    if (s.qlen > s.queue_room) s.error = "pixel queue longer than its buffers (n + 63 W)";
    return s;
}

// ---------------------------------------------------------------- the volume integrator's launch
// k_render_volume_sm: lanes advance one tentative collision per iteration and start their next sample
// independently.  When the shard spans several rounds of resident waves, the costliest wave-sized pixel
// groups (cost probe: tentative collisions of 4 samples per pixel) are launched first.
struct VolumeIn {
    uint32_t n_slots = 0, spp = 0;
    uint32_t resident = 1;    // resident 256-lane blocks of the plain build, with the grid's LDS
    uint32_t grid_cells = 0;  // cells of the medium's density grid (0: no medium)
    bool counters = false;    // the counter pass
    Knob sparse, sparse_f, sparse_rounds;  // test hooks: NART_VOL_SPARSE, _F, _ROUNDS
};
enum class VolumeBuild { Counter, FourWave, Plain };  // k_render_volume_sm<true, 1>, <false, NART_VOL_WV>, <false, 1>
struct VolumePlan {
    uint32_t lds_nodes = 0;  // density-grid cells read from LDS
    VolumeBuild build = VolumeBuild::Plain;
    uint32_t blocks = 0;      // a lane per slot, in blocks of 256
    bool queue = false;       // cost probe, then the groups costliest first
    uint32_t queue_room = 0;  // entries the queue buffers must hold
    bool sparse = false;      // the sorted group keys are read back for sparse_hot_groups
    uint32_t S = 0, W = 0;    // pixels per sparse wave; resident waves
    double f = 0.0;           // a hot group costs >= f x the median group
    uint32_t sched = 0;       // NART_SCHED_* bits known before the readback
};

// small density grids (C5: 2x2x2) are read from LDS (1 % faster than L1-hitting global loads); the
// occupancy query behind VolumeIn::resident needs the figure first
inline uint32_t volume_lds_cells(uint32_t grid_cells) { return grid_cells <= 4096u ? grid_cells : 0u; }

inline VolumePlan plan_volume(const VolumeIn& in) {
    VolumePlan v;
    const uint32_t n = in.n_slots;
    v.lds_nodes = volume_lds_cells(in.grid_cells);
    v.blocks = (n + 255u) / 256u;
    // occupancy: launches of >= 8 rounds of resident waves use the 4-waves-per-SIMD build (C5 frame,
    // 10.5 rounds: 134 -> 122 ms); smaller ones keep the unconstrained build, whose lanes' serial
    // chains are shorter (C5 1/2, 1/4, 1/8 shards: 79 / 74 / 71 ms vs 83 / 80 / 76 with 4 waves;
    // profiles/r03h_vol_w4_ab.log).  (Whole blocks per resident block here and below for the sparse
    // waves; the queue's 12 rounds count slots, rounds_of.)
    const double block_rounds = (double)v.blocks / (double)in.resident;
    v.build = in.counters ? VolumeBuild::Counter : (block_rounds >= 8.0 ? VolumeBuild::FourWave : VolumeBuild::Plain);
    v.W = in.resident * 4u;  // resident waves
    v.queue = v.blocks > in.resident && rounds_of(n, in.resident) < 12.0 && in.spp > 4u;
    if (!v.queue) return v;
    v.queue_room = n + 63u * v.W;
    v.sched |= NART_SCHED_VOL_QUEUE;
    // Sparse waves on shards of < NART_VOL_SPARSE_ROUNDS (default 2) rounds of resident
    // waves: the costliest groups (probe cost >= NART_VOL_SPARSE_F (4) x the median group's)
    // spread NART_VOL_SPARSE (16) pixels per wave, the other lanes idle.  A wave executes
    // the union of its lanes' divergent chains, and a frame's costliest volume pixels
    // cluster: C5's centre pixels take 30 ms alone at 1,024 spp, 69 ms as a wave of 64.
    // C5 1/8 shard 73.7 -> 65.3 ms; on larger shards (2+ rounds) the mostly idle sparse
    // waves hold slots the other groups need (1/2 shard 78 -> 127 ms), and 1-8 pixels per
    // wave measured worse (profiles/r04h_c5_sparse.log).  Only the order of work changes.
    v.S = (uint32_t)std::max(1.0, std::min(64.0, in.sparse.or_(16.0)));
    v.f = in.sparse_f.or_(4.0);
    v.sparse = v.S < 64u && (64u % v.S) == 0u && block_rounds < in.sparse_rounds.or_(2.0);
    return v;
}

// The sparse part of the volume queue, from the cost-sorted group keys read back from the device
// (k_group_keys: 0xFFFFFFFE - cost, ascending; 0xFFFFFFFF for a partial last group, which is no
// candidate): the H costliest groups, those of at least f x the median group's cost, as many as the
// queue's room beyond n (63 W entries, VolumePlan::queue_room) lets spread S pixels per wave.
struct SparseGroups {
    uint32_t H = 0;     // hot groups (0: the dense queue stays)
    uint32_t qlen = 0;  // queue entries with them spread
    uint32_t grid = 0;  // blocks of 256 lanes of the launch
};
inline SparseGroups sparse_hot_groups(const uint32_t* keys, uint32_t ng, double f, uint32_t S, uint32_t W, uint32_t n) {
    SparseGroups g;
    g.grid = (n + 255u) / 256u;
    uint32_t full = 0;  // whole groups: their costs, 0xFFFFFFFE - key, descend
    while (full < ng && keys[full] != 0xFFFFFFFFu) ++full;
    if (!full) return g;
    const double med = 0xFFFFFFFEu - keys[full / 2u];
    while (g.H < full && (double)(0xFFFFFFFEu - keys[g.H]) >= f * med) ++g.H;
    g.H = std::min<uint32_t>(g.H, 63u * W / (64u / S * 64u));
    if (!g.H) return g;
    g.qlen = g.H * (64u / S) * 64u + (n - 64u * g.H);
    g.grid = (g.qlen + 255u) / 256u;
    return g;
}

}  // namespace nd
