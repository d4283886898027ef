// What one render produces, decided once from plain values (no HIP, no context): the entry points of
// render.hip state a FrameAsk, plan_frame turns it into an error or a FramePlan, and render_frame,
// render_multi, render_buckets_adaptive and render_buckets execute the plan.  tests/test_frame_plan.py
// compares plan_frame with a restatement of the rules over every combination that can be asked for.
#pragma once
#include <cstdint>
#include <string>

#include "../../../include/nart_hip.h"

namespace nd {

// device/cascade.h CASCADE_MAX_LAYERS; device/matte.h MATTE_MAX_PLANES (four ids a plane), MATTE_MAX_IDS
constexpr uint32_t FRAME_MAX_LAYERS = 8, FRAME_MAX_PLANES = 8, FRAME_MAX_MATTE_IDS = 4 * FRAME_MAX_PLANES;
// beauty, two first-hit AOVs, moment, layers, planes, two followed guides (a frame has layers or
// planes, and first-hit AOVs or followed guides: at most twelve; a light-group frame the beauty and
// its groups, a depth-cut frame the beauty and its cuts: at most nine; a half-buffer frame the beauty,
// two AOVs or guides and the two halves: five)
constexpr uint32_t FRAME_MAX_OUTPUTS = 4 + FRAME_MAX_LAYERS + FRAME_MAX_PLANES + 2;
constexpr uint32_t FRAME_MAX_LIGHT_GROUPS = 8;  // include/nart_hip.h NART_LIGHT_GROUPS_MAX
constexpr uint32_t FRAME_MAX_DEPTH_CUTS = 8;    // include/nart_hip.h NART_DEPTH_CUTS_MAX
constexpr uint32_t FRAME_MAX_FOLLOW = 10;  // include/nart_hip.h NART_GUIDE_MAX_FOLLOW

// The firefly cascade's levels (include/nart_hip.h, "Firefly cascade"): layer j takes the share of
// every Li_alpha record around brightness b[j] = start * base^j.  K = 0: no cascade.
struct CascadeLevels {
    uint32_t K = 0;
    float base = 0.f;
    float b[FRAME_MAX_LAYERS] = {};
};
// The ID mattes' coverage planes (include/nart_hip.h, "First-hit ID mattes"): plane q holds the
// indicator records of ids 4q .. 4q+3 of `kind` (NART_MATTE_MESH, NART_MATTE_MATERIAL).
struct MatteRequest {
    bool on = false;
    uint32_t kind = 0, n_ids = 0;
    uint32_t planes() const { return on ? (n_ids + 3) / 4 : 0; }
};

struct FrameAsk {  // what the caller asks for
    uint32_t integrator;           // nart_render_params::integrator: first-hit outputs need surfaces
    bool beauty = true;            // false: no path kernel runs
    bool aov[2] = {false, false};  // first-hit AOVs: AOV_ALBEDO, AOV_NORMAL (kernels.h)
    bool moment = false;           // the second-moment image of the beauty's samples
    bool adaptive = false;         // buckets refined level by level, not rendered once at p->spp
    CascadeLevels cascade;
    MatteRequest matte;
    bool guide[2] = {false, false};  // followed guides (include/nart_hip.h, "Followed guides"): albedo, normal
    uint32_t max_follow = 0;         // delta interfaces a guide chain follows, 0..FRAME_MAX_FOLLOW
    uint32_t light_groups = 0;       // G light groups (include/nart_hip.h, "Light groups"), 0: off
    uint32_t depth_cuts = 0;         // K depth cuts (include/nart_hip.h, "Depth cuts"), 0: off
    // the cost image (include/nart_hip.h, "Cost image"): a per-pixel grid of counts next to the beauty.
    // Not a tile image: no output of the list, no pass, no splat, combine or gather
    bool cost = false;
    // the half buffers (include/nart_hip.h, "Half buffers"): the beauty's samples of even and of odd
    // index, each into a tile image of its own
    bool halves = false;
    explicit FrameAsk(uint32_t integrator_) : integrator(integrator_) {}
};

// One tile buffer (and image) of a render; index: j of cascade layer j, q of matte plane q, g of light
// group g, j of depth cut j, else 0.  HalfA: the samples of even index, HalfB: of odd index.
enum class OutputKind : uint32_t {
    Beauty, Albedo, Normal, Moment, Layer, Plane, GuideAlbedo, GuideNormal, LightGroup, DepthCut, HalfA, HalfB
};
struct FrameOutput { OutputKind kind = OutputKind::Beauty; uint32_t index = 0; };

// The passes of a batch after the path kernel and the beauty's splat, in the order they must run.
// Each fills a record buffer once per output it feeds and splats it into that output's tiles:
//   PASS_CASCADE    reads the Li_alpha records in d_L before anything else touches them
//                   (k_cascade_split into a second record buffer, one layer at a time);
//   PASS_MOMENT     k_moment squares d_L in place: after the cascade, the last reader of Li_alpha;
//   PASS_FIRST_HIT  k_aov overwrites d_L from the camera-ray hits (d_prim), one AOV at a time;
//   PASS_MATTE      k_matte_ids overwrites d_L from the same hits, one plane at a time;
//   PASS_GUIDE      k_guide traces every sample's chain once: the albedo record overwrites d_L, the
//                   normal record goes to a second record buffer where both are asked for;
//   PASS_HALVES     reads the Li_alpha records in d_L like the cascade (k_half_split into a second
//                   record buffer, one half at a time).  It runs first among a frame's passes, though it
//                   has the largest value: N_PASSES is also pass_of's "no pass" and stays what it was,
//                   so the new pass takes the next value after it.
enum PassKind : uint32_t { PASS_CASCADE, PASS_MOMENT, PASS_FIRST_HIT, PASS_MATTE, PASS_GUIDE, N_PASSES, PASS_HALVES };
constexpr uint32_t PASS_SLOTS = PASS_HALVES + 1;  // what is indexed by PassKind has this many entries
// The pass that fills an output's records, by OutputKind; N_PASSES: the beauty, the light groups
// and the depth cuts, the path kernel's own.
constexpr PassKind PASS_OF[8] = {N_PASSES,     PASS_FIRST_HIT, PASS_FIRST_HIT, PASS_MOMENT,
                                 PASS_CASCADE, PASS_MATTE,     PASS_GUIDE,     PASS_GUIDE};
inline PassKind pass_of(OutputKind k) {
    if (k == OutputKind::HalfA || k == OutputKind::HalfB) return PASS_HALVES;
    return k == OutputKind::LightGroup || k == OutputKind::DepthCut ? N_PASSES : PASS_OF[(uint32_t)k];
}

struct FramePlan {
    int code = NART_OK;  // not NART_OK: the first broken rule and its message; nothing else is set
    std::string message;
    FrameAsk ask{NART_INTEGRATOR_PATH};
    // Tile buffers and images in delivery order: beauty, albedo, normal, moment, then the layers or
    // the planes ascending, then the followed guides; a light-group frame: the beauty, then the groups
    // ascending; a depth-cut frame: the beauty, then the cuts ascending; the two halves come after the
    // followed guides.  On-device delivery lays the images out back to back in this order.
    FrameOutput outputs[FRAME_MAX_OUTPUTS];
    uint32_t n_outputs = 0;
    PassKind passes[PASS_SLOTS] = {};  // the passes that run: the halves' first, the others ascending
    uint32_t n_passes = 0;
    bool path_kernel = false;   // false: camera rays only (first-hit outputs without the beauty)
    // per-sample record memory beyond d_L (batch_slot_limit): the cascade's buffer, the second guide
    // record's where both guides are asked for, one record per light group or depth cut, the cost
    // record, or the halves' buffer (free again when the guide pass runs: the two share the 16 bytes)
    uint32_t record_bytes = 0;

    int find(OutputKind kind, uint32_t index = 0) const {  // position in the list, or -1
        for (uint32_t i = 0; i < n_outputs; ++i)
            if (outputs[i].kind == kind && outputs[i].index == index) return (int)i;
        return -1;
    }
};

// Whose rules apply: a whole frame's (render_frame), or those of a bare bucket-list render (a level
// of an adaptive render, nart_hip_render_buckets_async), which is not told how its tiles are used.
enum class PlanRules { Frame, Buckets };

inline FramePlan plan_frame(const FrameAsk& a, PlanRules rules) {
    FramePlan plan;
    const bool frame = rules == PlanRules::Frame, first_hit = a.aov[0] || a.aov[1] || a.matte.on;
    const bool guides = a.guide[0] || a.guide[1];
    int code = NART_E_UNSUPPORTED;
    std::string why;
    if (a.moment && !a.beauty) {
        code = NART_E_INVALID;
        why = frame ? "the moment image needs the path kernel: it cannot be rendered without the beauty"
                    : "the moment image needs the path kernel (the beauty)";
    } else if (frame && a.cascade.K && (!a.beauty || a.adaptive)) {
        why = "the cascade layers need the beauty and a uniform render";
    } else if (frame && a.matte.on && (a.cascade.K || a.adaptive)) {
        why = "the matte planes need a uniform render without the cascade";
    } else if (frame && first_hit && a.integrator == NART_INTEGRATOR_VOLUME) {
        why = "first-hit AOVs need surfaces: the volume integrator has none";
    } else if (!frame && a.cascade.K && !a.beauty) {
        code = NART_E_INVALID;
        why = "the cascade layers need the path kernel (the beauty)";
    } else if (a.matte.on && a.matte.n_ids > FRAME_MAX_MATTE_IDS) {  // (what the list of outputs holds)
        why = "the scene has " + std::to_string(a.matte.n_ids) + " matte ids; at most 32 are supported";
    } else if (guides && a.integrator == NART_INTEGRATOR_VOLUME) {
        why = "followed guides need surfaces: the volume integrator has none";
    } else if (guides && (a.adaptive || a.cascade.K || a.matte.on)) {
        why = "followed guides need a uniform render without the cascade and the mattes";
    } else if (guides && (a.aov[0] || a.aov[1])) {
        why = "followed guides and first-hit AOVs are not rendered in one call";
    } else if (guides && a.max_follow > FRAME_MAX_FOLLOW) {
        code = NART_E_INVALID;
        why = "max_follow must be 0..10";
    } else if (a.light_groups > FRAME_MAX_LIGHT_GROUPS) {
        code = NART_E_INVALID;
        why = "at most 8 light groups are supported";
    } else if (a.light_groups && !a.beauty) {
        code = NART_E_INVALID;
        why = "light groups need the path kernel (the beauty)";
    } else if (a.light_groups && a.integrator == NART_INTEGRATOR_VOLUME) {
        why = "light groups need the path integrator: the volume integrator has no light-group build";
    } else if (a.light_groups && a.adaptive) {
        why = "light groups need a uniform render: not adaptive sampling";
    } else if (a.light_groups && (a.cascade.K || a.matte.on || a.aov[0] || a.aov[1] || guides || a.moment)) {
        why = "light groups are not rendered with the cascade, the mattes, AOVs, guides or the moment image in one call";
    } else if (a.depth_cuts > FRAME_MAX_DEPTH_CUTS) {
        code = NART_E_INVALID;
        why = "at most 8 depth cuts are supported";
    } else if (a.depth_cuts && !a.beauty) {
        code = NART_E_INVALID;
        why = "depth cuts need the path kernel (the beauty)";
    } else if (a.depth_cuts && a.integrator == NART_INTEGRATOR_VOLUME) {
        why = "depth cuts need the path integrator: the volume integrator has no depth-cut build";
    } else if (a.depth_cuts && a.adaptive) {
        why = "depth cuts need a uniform render: not adaptive sampling";
    } else if (a.depth_cuts &&
               (a.cascade.K || a.matte.on || a.aov[0] || a.aov[1] || guides || a.moment || a.light_groups)) {
        why = "depth cuts are not rendered with the cascade, the mattes, AOVs, guides, the moment image or light groups in "
              "one call";
    } else if (a.cost && !a.beauty) {
        code = NART_E_INVALID;
        why = "the cost image needs the path kernel (the beauty)";
    } else if (a.cost && a.integrator == NART_INTEGRATOR_VOLUME) {
        why = "the cost image needs the path integrator: the volume integrator has no cost build";
    } else if (a.cost && a.adaptive) {
        why = "the cost image needs a uniform render: not adaptive sampling";
    } else if (a.cost && (a.cascade.K || a.matte.on || a.aov[0] || a.aov[1] || guides || a.moment || a.light_groups ||
                          a.depth_cuts)) {
        why = "the cost image is not rendered with the cascade, the mattes, AOVs, guides, the moment image, light groups or "
              "depth cuts in one call";
    } else if (a.halves && !a.beauty) {
        code = NART_E_INVALID;
        why = "the half buffers need the path kernel (the beauty)";
    } else if (a.halves && a.adaptive) {
        why = "the half buffers need a uniform render: not adaptive sampling";
    } else if (a.halves && (a.moment || a.cascade.K || a.matte.on || a.light_groups || a.depth_cuts || a.cost)) {
        why = "the half buffers are not rendered with the moment image, the cascade, the mattes, light groups, depth cuts or "
              "the cost image in one call";
    }
    if (!why.empty()) {
        plan.code = code;
        plan.message = why;
        return plan;
    }
    plan.ask = a;
    auto add = [&plan](OutputKind kind, uint32_t index) { plan.outputs[plan.n_outputs++] = {kind, index}; };
    if (a.beauty) add(OutputKind::Beauty, 0);
    if (a.aov[0]) add(OutputKind::Albedo, 0);
    if (a.aov[1]) add(OutputKind::Normal, 0);
    if (a.moment) add(OutputKind::Moment, 0);
    for (uint32_t j = 0; j < a.cascade.K; ++j) add(OutputKind::Layer, j);
    for (uint32_t q = 0; q < a.matte.planes(); ++q) add(OutputKind::Plane, q);
    if (a.guide[0]) add(OutputKind::GuideAlbedo, 0);
    if (a.guide[1]) add(OutputKind::GuideNormal, 0);
    if (a.halves) add(OutputKind::HalfA, 0);
    if (a.halves) add(OutputKind::HalfB, 0);
    for (uint32_t g = 0; g < a.light_groups; ++g) add(OutputKind::LightGroup, g);
    for (uint32_t j = 0; j < a.depth_cuts; ++j) add(OutputKind::DepthCut, j);
    // An adaptive render estimates a bucket's error from its moment tiles: every level runs the moment
    // pass, wanted or not (adaptive_level_ask).
    bool runs[PASS_SLOTS] = {};
    runs[PASS_MOMENT] = a.adaptive;
    for (uint32_t i = 0; i < plan.n_outputs; ++i) runs[pass_of(plan.outputs[i].kind)] = true;
    if (runs[PASS_HALVES]) plan.passes[plan.n_passes++] = PASS_HALVES;  // before anything overwrites Li_alpha
    for (uint32_t k = 0; k < N_PASSES; ++k)
        if (runs[k]) plan.passes[plan.n_passes++] = (PassKind)k;
    plan.path_kernel = a.beauty;
    plan.record_bytes = (a.cascade.K || a.halves || (a.guide[0] && a.guide[1])) ? 16 : 0;  // one float4 per sample
    if (a.light_groups) plan.record_bytes = 16 * a.light_groups;              // and per group
    if (a.depth_cuts) plan.record_bytes = 16 * a.depth_cuts;                  // or per cut
    if (a.cost) plan.record_bytes = 16;                                       // one uint4 per sample
    return plan;
}

// What one level of an adaptive render asks of render_buckets: a uniform render of the beauty, the
// wanted AOVs and, always, the moment tiles.
inline FrameAsk adaptive_level_ask(FrameAsk a) { a.moment = true; a.adaptive = false; return a; }

}  // namespace nd
