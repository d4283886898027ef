// The parameter structs of the stages that work on whole images (include/nart_hip.h: denoiser,
// adaptive sampling, firefly cascade, ID mattes, followed guides), as far as they need no device: their
// defaults, their rules and what is computed from them alone (no HIP, no context).  Every X_params_error
// has one shape: `in` (null: the defaults) is copied into `out`, and the message of the first broken
// rule is returned, or null.  The entry points of render.hip raise the message as NART_E_INVALID.
// tests/test_stage_params.py compares all of this with a restatement of the rules.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../../include/nart_hip.h"
#include "denoise_passes.h"
#include "frame_plan.h"

namespace nd {

constexpr uint32_t STAGE_MAX_RANKS = 8;  // device/matte.h MATTE_MAX_RANKS

// The defaults, field by field in the structs' order, as include/nart_hip.h documents them.
constexpr nart_denoise_params DENOISE_DEFAULTS = {5, 5, 4.f, 1.f, 1e-3f, 0.05f, 0.01f};
constexpr nart_guide_params GUIDE_DEFAULTS = {8};
constexpr nart_adaptive_params ADAPTIVE_DEFAULTS = {16, 4, 0.1f, 0.01f};
constexpr nart_cascade_params CASCADE_DEFAULTS = {6, 1.f, 8.f, 2.f};
constexpr nart_matte_params MATTE_DEFAULTS = {NART_MATTE_MESH, 6};

// ---------------------------------------------------------------- denoiser
inline const char* denoise_params_error(const nart_denoise_params* in, nart_denoise_params& out) {
    out = in ? *in : DENOISE_DEFAULTS;
    static_assert(DN_MAX_ITERATIONS == 8, "the message below, and pass_ms[8] of the timing getters");
    if (out.iterations < 1 || out.iterations > DN_MAX_ITERATIONS) return "denoise iterations must be 1..8";
    if (out.normal_squarings > 16) return "denoise normal_squarings must be <= 16";
    if (!(out.sigma_color > 0.f) || !(out.sigma_depth > 0.f) || !(out.depth_eps > 0.f) || !(out.sigma_coverage > 0.f) ||
        !(out.albedo_floor > 0.f))
        return "denoise sigmas, depth_eps and albedo_floor must be > 0";
    return nullptr;
}

// ---------------------------------------------------------------- followed guides
inline const char* guide_params_error(const nart_guide_params* in, nart_guide_params& out) {
    out = in ? *in : GUIDE_DEFAULTS;
    if (out.max_follow > NART_GUIDE_MAX_FOLLOW) return "max_follow must be 0..10";
    return nullptr;
}

// ---------------------------------------------------------------- adaptive sampling
// spp: the render's sample count (nart_render_params::spp).
inline const char* adaptive_params_error(const nart_adaptive_params* in, nart_adaptive_params& out, uint32_t spp) {
    out = in ? *in : ADAPTIVE_DEFAULTS;
    if (out.min_spp < 2) return "adaptive min_spp must be >= 2 (one sample has no variance)";
    if (spp < 2) return "adaptive sampling needs spp >= 2 (one sample has no variance)";
    if (out.growth < 2 || out.growth > 16) return "adaptive growth must be in 2..16";
    if (!(out.threshold >= 0.f)) return "adaptive threshold must be >= 0 (+inf: nothing refines)";
    if (!(out.floor > 0.f) || !std::isfinite(out.floor)) return "adaptive floor must be finite and > 0";
    return nullptr;
}

// L_0 = min_spp, L_{i+1} = min(L_i * growth, spp), ending on spp; the one level spp if min_spp >= spp.
constexpr uint32_t ADAPTIVE_MAX_LEVELS = 32;
inline std::vector<uint32_t> adaptive_levels(const nart_adaptive_params& ap, uint32_t spp) {
    std::vector<uint32_t> levels;
    uint64_t L = ap.min_spp;
    while (L < spp && levels.size() + 1 < ADAPTIVE_MAX_LEVELS) {
        levels.push_back((uint32_t)L);
        L = std::min<uint64_t>(L * ap.growth, spp);
    }
    levels.push_back(spp);
    return levels;
}

// ---------------------------------------------------------------- firefly cascade
// Also the levels b[j] = start * base^j into lv, by repeated float multiplication.
inline const char* cascade_params_error(const nart_cascade_params* in, nart_cascade_params& out, CascadeLevels& lv) {
    out = in ? *in : CASCADE_DEFAULTS;
    if (out.layers < 2 || out.layers > FRAME_MAX_LAYERS) return "cascade layers must be in 2..8";
    if (!std::isfinite(out.start) || !(out.start > 0.f)) return "cascade start must be finite and > 0";
    if (!std::isfinite(out.base) || !(out.base > 1.f)) return "cascade base must be finite and > 1";
    if (!std::isfinite(out.kappa) || !(out.kappa > 0.f)) return "cascade kappa must be finite and > 0";
    lv.K = out.layers;
    lv.base = out.base;
    float b = out.start;
    for (uint32_t j = 0; j < lv.K; ++j) {
        if (!std::isfinite(b)) return "a cascade level is not finite";
        if (j > 0 && !(b > lv.b[j - 1])) return "the cascade levels do not increase (start too small for base)";
        lv.b[j] = b;
        b = b * out.base;
    }
    return nullptr;
}

// ---------------------------------------------------------------- first-hit ID mattes
inline const char* matte_params_error(const nart_matte_params* in, nart_matte_params& out) {
    out = in ? *in : MATTE_DEFAULTS;
    if (out.kind != NART_MATTE_MESH && out.kind != NART_MATTE_MATERIAL) return "unknown matte id kind";
    if (out.ranks < 2 || out.ranks > STAGE_MAX_RANKS || (out.ranks & 1u)) return "matte ranks must be even and in 2..8";
    return nullptr;
}

// ---------------------------------------------------------------- light groups
// The group map of a light-group render: group_of_light[n_lights], one entry per light of the scene
// (scene_lights), each below n_groups.
inline const char* light_groups_error(const uint32_t* group_of_light, uint32_t n_lights, uint32_t scene_lights,
                                      uint32_t n_groups) {
    if (n_groups < 1 || n_groups > NART_LIGHT_GROUPS_MAX) return "n_groups must be 1..8";
    if (!group_of_light) return "the light-group map is required";
    if (n_lights != scene_lights) return "the light-group map must have one entry per light of the scene";
    for (uint32_t l = 0; l < n_lights; ++l)
        if (group_of_light[l] >= n_groups) return "a light's group must be < n_groups";
    return nullptr;
}

// The mix of group images: gains[n_groups][3], finite.
inline const char* light_mix_error(uint32_t n_groups, const float* gains, const void* groups, const void* out) {
    if (n_groups < 1 || n_groups > NART_LIGHT_GROUPS_MAX) return "n_groups must be 1..8";
    if (!gains || !groups || !out) return "the gains, the group images and the mixed image are required";
    for (uint32_t i = 0; i < 3 * n_groups; ++i)
        if (!std::isfinite(gains[i])) return "light-mix gains must be finite";
    return nullptr;
}

// ---------------------------------------------------------------- depth cuts
// The cuts of a depth-cut render: cuts[n_cuts], strictly ascending, each in 1..bounces.
inline const char* depth_cuts_error(const uint32_t* cuts, uint32_t n_cuts, uint32_t bounces) {
    if (n_cuts < 1 || n_cuts > NART_DEPTH_CUTS_MAX) return "n_cuts must be 1..8";
    if (!cuts) return "the depth cuts are required";
    for (uint32_t j = 0; j < n_cuts; ++j) {
        if (cuts[j] < 1) return "a depth cut must be at least 1";
        if (cuts[j] > bounces) return "a depth cut must not exceed the bounce limit";
        if (j && cuts[j] <= cuts[j - 1]) return "depth cuts must be strictly ascending";
    }
    return nullptr;
}

// ---------------------------------------------------------------- denoised parts
// A parts denoise (include/nart_hip.h, "Denoised parts"): n_parts images in 1..9; images_given: every
// image the call requires is there; dp (null: the defaults) into d; follow (null: the first-hit AOVs are
// the guides) into g.  The rules in this order: the count, the images, the denoiser's, the guides'.
// The whole-frame calls check their group map or their cuts first (light_groups_error, depth_cuts_error)
// and hand in the number of parts those give.
inline const char* denoise_parts_error(uint32_t n_parts, bool images_given, const nart_denoise_params* dp,
                                       nart_denoise_params& d, const nart_guide_params* follow, nart_guide_params& g) {
    d = dp ? *dp : DENOISE_DEFAULTS;
    g = follow ? *follow : GUIDE_DEFAULTS;
    if (n_parts < 1 || n_parts > NART_DENOISE_PARTS_MAX) return "n_parts must be 1..9";
    if (!images_given) return "the part images, the guide images and the denoised images are required";
    if (const char* why = denoise_params_error(dp, d)) return why;
    return follow ? guide_params_error(follow, g) : nullptr;
}

// ---------------------------------------------------------------- what the stages need of p
// What the stages over whole images (denoiser, reweighting, ranking) need of p without check_params.
inline const char* check_image_size(const nart_render_params* p) {
    if (!p->image_width || !p->image_height || !(p->filter_width > 0.f))
        return "imageWidth, imageHeight and filterWidth must be > 0";
    return nullptr;
}

inline const char* check_sample_variance(const nart_render_params* p) {
    return p->spp < 2 ? "sample variance needs spp >= 2" : nullptr;
}

inline const char* check_cascade_frame(const nart_render_params* p) {
    if (const char* why = check_image_size(p)) return why;
    return p->spp < 1 ? "the cascade needs spp >= 1" : nullptr;
}

}  // namespace nd
