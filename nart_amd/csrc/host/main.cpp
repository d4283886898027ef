// `nart <scene file> <output path> [-w -h -b -s -o -f -r] [--gpus N | --devices a,b,...] [--device d]`
// -- drop-in for the reference CLI (src/core/main.cpp:12-61) with RenderSession::Render() served
// by the MI355X path.  The reference's flags are parsed by nart_parse_args exactly as
// ParseRenderParamArguments does (render.cpp:236-325); the device flags are this build's own and
// are taken out of argv first:
//   --gpus N        render every session over GPUs 0..N-1 (or d..d+N-1 with --device d); "all" = every
//                   visible GPU.  Buckets are sharded over the GPUs and gathered with RCCL
//                   (nart_hip_create_multi); the image is bit-identical for any N.
//   --devices a,b   an explicit device list (repeats allowed: a rehearsal on fewer GPUs)
//   --device d      first (or only) device; NART_DEVICE sets the default, which is 0
//   --aovs          also write the first-hit AOVs of every session (nart_hip_render_aovs) through the
//                   same EXR writer: <out>.albedo.exr (RGB albedo, A coverage) and <out>.normal.exr
//                   (RGB shading normal, filtered and not renormalised; A depth), in half precision;
//                   <out>_<n>.albedo.exr / <out>_<n>.normal.exr with several sessions
//   --denoise       also write every session's denoised image (nart_hip_render_denoised, default
//                   parameters; with --aovs nart_hip_denoise over the AOVs rendered anyway: the same
//                   image) to <out>.denoised.exr, through the same writer
//   --sample-variance  with --denoise: the denoiser takes each pixel's variance from the renderer's
//                   second-moment image (nart_hip_render_denoised_moment; with --aovs
//                   nart_hip_render_moment + nart_hip_denoise_moment: the same image) instead of the
//                   spatial estimate; without --denoise it is an error
//   --adaptive T    render every session adaptively (nart_hip_render_adaptive) with threshold T: a pilot
//                   pass, then more samples only for the buckets whose error exceeds T; -s is the
//                   maximum.  Also writes <out>.spp.exr (RGB = the sample count of the pixel's bucket,
//                   A = 1) and prints the levels, the buckets rendered per level and the samples
//                   taken.  With --aovs the AOVs are the adaptive call's; with --denoise the adaptive
//                   images go through nart_hip_denoise, with --sample-variance too through
//                   nart_hip_denoise_moment
//   --min-spp N     with --adaptive: the samples of the pilot pass (default 16); without it an error
//   --robust [KAPPA]  also write every session's firefly-robust image (nart_hip_render_cascade, default
//                   parameters; KAPPA, if the next argument is a number, replaces kappa) to
//                   <out>.robust.exr; <out>.exr is the same call's beauty.  Not offered together with
//                   --adaptive, --aovs or --denoise: an error
//   --mattes [mesh|material]  also write every session's first-hit ID mattes (nart_hip_render_mattes;
//                   ids are mesh indices by default) to <out>.matte.00.exr ... <out>.matte.0{R/2-1}.exr:
//                   image k holds (id, coverage) of ranks 2k and 2k+1 in RG and BA; <out>.exr is the
//                   same call's beauty.  With --aovs or --denoise the mattes are a matte-only call
//                   after the main one.  Not offered together with --adaptive or --robust: an error
//   --matte-ranks N with --mattes: the ranks kept per pixel, even and in 2..8 (default 6)
//   --matte-ids a,b,..  with --mattes: also write <out>.matte.exr, the summed coverage of that id set
//   --follow-specular [N]  with --aovs and/or --denoise: <out>.albedo.exr, <out>.normal.exr and
//                   <out>.denoised.exr come from the followed guides (nart_hip_render_guides,
//                   nart_hip_render_denoised_guides): the first surface behind perfect mirrors and smooth
//                   glass, at most N (0..10, default 8) interfaces deep.  Without --aovs or --denoise,
//                   or together with --adaptive, --robust or --mattes: an error
//   --light-groups each|a,b,c,..  also write every session's beauty split by light
//                   (nart_hip_render_light_groups) to <out>.light.00.exr ...: `each` gives every light a
//                   group of its own (at most 8 lights), the list the group of every light in scene
//                   order (groups 0..7); <out>.exr is the same call's beauty.  Not offered together with
//                   --adaptive, --robust, --mattes, --aovs, --denoise or --follow-specular: an error
//   --light-gains k0,k1,..  with --light-groups: one gain per group; also write <out>.mix.exr, the sum of
//                   the group images scaled by their gains (nart_hip_light_mix)
//   --depth-cuts d0,d1,..  also write every session's image at the bounce limits d0 < d1 < .. (at most 8,
//                   each in 1..bounces) from the one render (nart_hip_render_depth_cuts) to
//                   <out>.depth.NN.exr, NN the cut; <out>.exr is the same call's beauty.  Not offered
//                   together with --light-groups, --adaptive, --robust, --mattes, --aovs, --denoise or
//                   --follow-specular: an error
//   --depth-layers  with --depth-cuts: also write <out>.layer.00.exr ... <out>.layer.0K.exr, the light each
//                   range of bounces added (nart_hip_depth_layers): the first cut, the differences of
//                   neighbouring cuts, the beauty minus the last cut
//   --denoise-parts  with --light-groups or --depth-cuts: also denoise the group images or the depth layers
//                   one by one with shared guides (default parameters) and write them to
//                   <out>.light.NN.denoised.exr or <out>.layer.NN.denoised.exr, and their sum to
//                   <out>.denoised.exr; with --light-gains also <out>.mix.denoised.exr, the denoised groups
//                   through nart_hip_light_mix.  The light groups take one call
//                   (nart_hip_render_denoised_light_groups); the depth cuts, whose cut images are written
//                   too, nart_hip_render_depth_cuts, nart_hip_depth_layers, a guides-only render and
//                   nart_hip_denoise_parts: the same images.  The noisy layers are written only with
//                   --depth-layers.  --follow-specular [N] next to it selects the followed guides.  Without
//                   --light-groups or --depth-cuts: an error
//   --cost          also write every session's cost image (nart_hip_render_cost, nart_hip_cost_image) to
//                   <out>.cost.exr: RGBA the per-sample means of extension rays, shadow rays, shaded hits
//                   and traversal steps (BVH node visits plus triangle tests) of every pixel of the
//                   cropped window, in half precision -- a mean above 65504 is written as inf -- and
//                   print the four totals; <out>.exr is the same call's beauty.  Not offered together
//                   with --depth-cuts, --light-groups, --adaptive, --robust, --mattes, --aovs, --denoise
//                   or --follow-specular: an error
//   --halves        also write every session's half buffers (nart_hip_render_halves) to <out>.half.0.exr and
//                   <out>.half.1.exr: the samples of even and of odd index, each divided by the beauty's
//                   filter weight sum, so that the two files add up to <out>.exr, the same call's beauty.
//                   With --aovs (and --follow-specular [N]) the AOVs or followed guides are the same
//                   call's.  Not offered together with --denoise, --denoise-parts, --adaptive, --robust,
//                   --mattes, --light-groups, --depth-cuts or --cost: an error
//   --denoise-cross  also write every session's cross-filtered denoised image and its error image
//                   (nart_hip_render_denoised_cross, default parameters) to <out>.denoised.exr and
//                   <out>.error.exr: the two half buffers of the render, each filtered with colour weights
//                   from the other, averaged; the error is the squared half difference of the two.  With
//                   --halves and/or --aovs the half buffers and AOVs are rendered anyway and go through
//                   nart_hip_denoise_cross: the same images.  --follow-specular [N] next to it selects the
//                   followed guides.  Needs -s >= 2.  Not offered together with --denoise, --denoise-parts,
//                   --sample-variance, --adaptive, --robust, --mattes, --light-groups, --depth-cuts or
//                   --cost: an error
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/nart_hip.h"

namespace {

bool parse_int(const char* s, int& v) {
    char* end = nullptr;
    long x = std::strtol(s, &end, 10);
    if (!s[0] || *end) return false;
    v = (int)x;
    return true;
}

// Removes the device flags from argv (kept: everything the reference CLI parses).
bool take_device_flags(std::vector<char*>& args, std::vector<int>& devices) {
    int first = 0, gpus = 1;
    bool all = false;
    if (const char* e = std::getenv("NART_DEVICE")) parse_int(e, first);
    std::vector<int> list;
    std::vector<char*> kept;
    for (size_t i = 0; i < args.size(); ++i) {
        const char* a = args[i];
        const bool dev = !std::strcmp(a, "--device"), g = !std::strcmp(a, "--gpus"), l = !std::strcmp(a, "--devices");
        if (!dev && !g && !l) {
            kept.push_back(args[i]);
            continue;
        }
        if (i + 1 >= args.size()) {
            std::fprintf(stderr, "Error: %s needs a value\n", a);
            return false;
        }
        const char* v = args[++i];
        if (dev && !parse_int(v, first)) {
            std::fprintf(stderr, "Error: --device %s\n", v);
            return false;
        }
        if (g) {
            if (!std::strcmp(v, "all")) all = true;
            else if (!parse_int(v, gpus) || gpus < 1) {
                std::fprintf(stderr, "Error: --gpus %s\n", v);
                return false;
            }
        }
        if (l) {
            std::string s(v);
            size_t pos = 0;
            while (pos <= s.size()) {
                size_t c = s.find(',', pos);
                if (c == std::string::npos) c = s.size();
                int d = 0;
                if (!parse_int(s.substr(pos, c - pos).c_str(), d)) {
                    std::fprintf(stderr, "Error: --devices %s\n", v);
                    return false;
                }
                list.push_back(d);
                pos = c + 1;
            }
        }
    }
    args = kept;
    if (!list.empty()) {
        devices = list;
        return true;
    }
    if (all) {
        int n = 0;
        if (nart_hip_device_count(&n) != NART_OK || n < 1) {
            std::fprintf(stderr, "Error: no HIP devices\n");
            return false;
        }
        gpus = n - first;
    }
    for (int d = 0; d < gpus; ++d) devices.push_back(first + d);
    return true;
}

// Removes every `flag` (--aovs, --denoise, --sample-variance) from argv; true if it was there.
bool take_flag(std::vector<char*>& args, const char* flag) {
    std::vector<char*> kept;
    for (char* a : args)
        if (std::strcmp(a, flag)) kept.push_back(a);
    const bool found = kept.size() != args.size();
    args = kept;
    return found;
}

// Removes every `flag <value>` pair from argv; the last value into `value`.  False (after a
// message) if a flag lacks its value.
bool take_value_flag(std::vector<char*>& args, const char* flag, const char*& value) {
    std::vector<char*> kept;
    for (size_t i = 0; i < args.size(); ++i) {
        if (std::strcmp(args[i], flag)) {
            kept.push_back(args[i]);
            continue;
        }
        if (i + 1 >= args.size()) {
            std::fprintf(stderr, "Error: %s needs a value\n", flag);
            return false;
        }
        value = args[++i];
    }
    args = kept;
    return true;
}

// Removes every `flag [number]` from argv; true if it was there.  The argument after the flag is
// its value only if all of it parses as a number (the last value into `value`).
bool take_optional_value_flag(std::vector<char*>& args, const char* flag, float& value) {
    std::vector<char*> kept;
    bool found = false;
    for (size_t i = 0; i < args.size(); ++i) {
        if (std::strcmp(args[i], flag)) {
            kept.push_back(args[i]);
            continue;
        }
        found = true;
        if (i + 1 < args.size() && args[i + 1][0]) {
            char* end = nullptr;
            const float v = std::strtof(args[i + 1], &end);
            if (!*end) {
                value = v;
                ++i;
            }
        }
    }
    args = kept;
    return found;
}

// Removes every `flag [word]` from argv, where word is one of `words`; true if the flag was there
// (the last word into `value`).
bool take_optional_word_flag(std::vector<char*>& args, const char* flag, const std::vector<const char*>& words,
                             const char*& value) {
    std::vector<char*> kept;
    bool found = false;
    for (size_t i = 0; i < args.size(); ++i) {
        if (std::strcmp(args[i], flag)) {
            kept.push_back(args[i]);
            continue;
        }
        found = true;
        if (i + 1 < args.size())
            for (const char* w : words)
                if (!std::strcmp(args[i + 1], w)) {
                    value = w;
                    ++i;
                    break;
                }
    }
    args = kept;
    return found;
}

}  // namespace

int main(int argc, char* argv[]) {
    std::vector<char*> args(argv, argv + argc);
    std::vector<int> devices;
    const bool aovs = take_flag(args, "--aovs");
    const bool denoise = take_flag(args, "--denoise");
    const bool sample_variance = take_flag(args, "--sample-variance");
    const bool denoise_parts = take_flag(args, "--denoise-parts");
    const bool denoise_cross = take_flag(args, "--denoise-cross");
    const char* const cross_alone = "Error: --denoise-cross is not offered together with --denoise, --denoise-parts, "
                                    "--sample-variance, --adaptive, --robust, --mattes, --light-groups, --depth-cuts or --cost\n";
    if (denoise_cross && (denoise || denoise_parts || sample_variance)) {
        std::fputs(cross_alone, stderr);
        return EXIT_FAILURE;
    }
    if (sample_variance && !denoise) {
        std::fprintf(stderr, "Error: --sample-variance selects the denoiser's variance input and needs --denoise\n");
        return EXIT_FAILURE;
    }
    const char *adaptive_arg = nullptr, *min_spp_arg = nullptr;
    if (!take_value_flag(args, "--adaptive", adaptive_arg) || !take_value_flag(args, "--min-spp", min_spp_arg))
        return EXIT_FAILURE;
    if (min_spp_arg && !adaptive_arg) {
        std::fprintf(stderr, "Error: --min-spp sets the pilot pass of adaptive sampling and needs --adaptive\n");
        return EXIT_FAILURE;
    }
    const bool adaptive = adaptive_arg != nullptr;
    nart_cascade_params cp;
    nart_hip_cascade_defaults(&cp);
    const bool robust = take_optional_value_flag(args, "--robust", cp.kappa);
    if (robust && (adaptive || aovs || denoise)) {
        std::fprintf(stderr, "Error: --robust is not offered together with --adaptive, --aovs or --denoise\n");
        return EXIT_FAILURE;
    }
    uint32_t n_levels = 0;
    if (robust && nart_hip_cascade_levels(&cp, nullptr, &n_levels) != NART_OK) {
        std::fprintf(stderr, "Error: --robust %g: kappa must be finite and > 0\n", cp.kappa);
        return EXIT_FAILURE;
    }
    nart_matte_params mp;
    nart_hip_matte_defaults(&mp);
    const char *matte_kind = nullptr, *matte_ranks_arg = nullptr, *matte_ids_arg = nullptr;
    const bool mattes = take_optional_word_flag(args, "--mattes", {"mesh", "material"}, matte_kind);
    if (!take_value_flag(args, "--matte-ranks", matte_ranks_arg) || !take_value_flag(args, "--matte-ids", matte_ids_arg))
        return EXIT_FAILURE;
    if ((matte_ranks_arg || matte_ids_arg) && !mattes) {
        std::fprintf(stderr, "Error: --matte-ranks and --matte-ids belong to the ID mattes and need --mattes\n");
        return EXIT_FAILURE;
    }
    if (mattes && (adaptive || robust)) {
        std::fprintf(stderr, "Error: --mattes is not offered together with --adaptive or --robust\n");
        return EXIT_FAILURE;
    }
    uint64_t matte_mask = 0;
    if (mattes) {
        if (matte_kind && !std::strcmp(matte_kind, "material")) mp.kind = NART_MATTE_MATERIAL;
        int v = 0;
        if (matte_ranks_arg && (!parse_int(matte_ranks_arg, v) || v < 2 || v > 8 || (v & 1))) {
            std::fprintf(stderr, "Error: --matte-ranks %s: the ranks must be even and in 2..8\n", matte_ranks_arg);
            return EXIT_FAILURE;
        }
        if (matte_ranks_arg) mp.ranks = (uint32_t)v;
        if (matte_ids_arg) {
            const std::string s(matte_ids_arg);
            size_t pos = 0;
            while (pos <= s.size()) {
                size_t c = s.find(',', pos);
                if (c == std::string::npos) c = s.size();
                int id = 0;
                if (!parse_int(s.substr(pos, c - pos).c_str(), id) || id < 0 || id > 31) {
                    std::fprintf(stderr, "Error: --matte-ids %s: a comma-separated list of ids in 0..31\n", matte_ids_arg);
                    return EXIT_FAILURE;
                }
                matte_mask |= 1ull << id;
                pos = c + 1;
            }
        }
    }
    // --follow-specular [N]: the AOVs and the denoiser's guides follow mirrors and smooth glass
    nart_guide_params gp;
    nart_hip_guide_defaults(&gp);
    float follow_arg = (float)gp.max_follow;
    const bool follow = take_optional_value_flag(args, "--follow-specular", follow_arg);
    if (follow && !aovs && !denoise && !denoise_parts && !denoise_cross) {
        std::fprintf(stderr, "Error: --follow-specular selects the guides of --aovs and --denoise and needs one of them\n");
        return EXIT_FAILURE;
    }
    if (follow && (adaptive || robust || mattes)) {
        std::fprintf(stderr, "Error: --follow-specular is not offered together with --adaptive, --robust or --mattes\n");
        return EXIT_FAILURE;
    }
    if (follow && !(follow_arg >= 0.f && follow_arg <= (float)NART_GUIDE_MAX_FOLLOW && follow_arg == (float)(int)follow_arg)) {
        std::fprintf(stderr, "Error: --follow-specular %g: a whole number in 0..10\n", follow_arg);
        return EXIT_FAILURE;
    }
    if (follow) gp.max_follow = (uint32_t)follow_arg;
    // --light-groups each|a,b,..  and  --light-gains k0,k1,..
    const char *groups_arg = nullptr, *gains_arg = nullptr;
    if (!take_value_flag(args, "--light-groups", groups_arg) || !take_value_flag(args, "--light-gains", gains_arg))
        return EXIT_FAILURE;
    const bool light_groups = groups_arg != nullptr;
    if (gains_arg && !light_groups) {
        std::fprintf(stderr, "Error: --light-gains scales the light groups and needs --light-groups\n");
        return EXIT_FAILURE;
    }
    if (light_groups && (adaptive_arg || robust || mattes || aovs || denoise || (follow && !denoise_parts))) {
        std::fprintf(stderr, "Error: --light-groups is not offered together with --adaptive, --robust, --mattes, --aovs, "
                             "--denoise or --follow-specular\n");
        return EXIT_FAILURE;
    }
    std::vector<uint32_t> group_of_light;  // empty: one group per light
    std::vector<float> light_gains;        // [G][3], once the group count is known
    std::vector<float> gain_list;
    if (light_groups && std::strcmp(groups_arg, "each")) {
        const std::string s(groups_arg);
        for (size_t pos = 0; pos <= s.size();) {
            size_t c = s.find(',', pos);
            if (c == std::string::npos) c = s.size();
            int v = 0;
            if (!parse_int(s.substr(pos, c - pos).c_str(), v) || v < 0 || v >= (int)NART_LIGHT_GROUPS_MAX) {
                std::fprintf(stderr, "Error: --light-groups %s: `each`, or a comma-separated list of groups in 0..7\n", groups_arg);
                return EXIT_FAILURE;
            }
            group_of_light.push_back((uint32_t)v);
            pos = c + 1;
        }
    }
    if (gains_arg) {
        const std::string s(gains_arg);
        for (size_t pos = 0; pos <= s.size();) {
            size_t c = s.find(',', pos);
            if (c == std::string::npos) c = s.size();
            const std::string t = s.substr(pos, c - pos);
            char* end = nullptr;
            const float v = std::strtof(t.c_str(), &end);
            if (t.empty() || *end || !(v - v == 0.f)) {
                std::fprintf(stderr, "Error: --light-gains %s: a comma-separated list of finite numbers\n", gains_arg);
                return EXIT_FAILURE;
            }
            gain_list.push_back(v);
            pos = c + 1;
        }
    }
    // --depth-cuts d0,d1,..  and  --depth-layers
    const char* cuts_arg = nullptr;
    if (!take_value_flag(args, "--depth-cuts", cuts_arg)) return EXIT_FAILURE;
    const bool depth_layers = take_flag(args, "--depth-layers");
    const bool depth_cuts = cuts_arg != nullptr;
    if (depth_layers && !depth_cuts) {
        std::fprintf(stderr, "Error: --depth-layers subtracts the depth cuts and needs --depth-cuts\n");
        return EXIT_FAILURE;
    }
    if (depth_cuts && (light_groups || adaptive_arg || robust || mattes || aovs || denoise || (follow && !denoise_parts))) {
        std::fprintf(stderr, "Error: --depth-cuts is not offered together with --light-groups, --adaptive, --robust, --mattes, "
                             "--aovs, --denoise or --follow-specular\n");
        return EXIT_FAILURE;
    }
    std::vector<uint32_t> cuts;
    if (depth_cuts) {
        const std::string s(cuts_arg);
        for (size_t pos = 0; pos <= s.size();) {
            size_t c = s.find(',', pos);
            if (c == std::string::npos) c = s.size();
            int v = 0;
            if (!parse_int(s.substr(pos, c - pos).c_str(), v) || v < 1 || (!cuts.empty() && (uint32_t)v <= cuts.back()) ||
                cuts.size() == NART_DEPTH_CUTS_MAX) {
                std::fprintf(stderr, "Error: --depth-cuts %s: a comma-separated, strictly ascending list of at most 8 bounce "
                                     "limits, each at least 1\n", cuts_arg);
                return EXIT_FAILURE;
            }
            cuts.push_back((uint32_t)v);
            pos = c + 1;
        }
    }
    if (denoise_parts && !light_groups && !depth_cuts) {
        std::fprintf(stderr, "Error: --denoise-parts denoises the light groups or the depth layers and needs --light-groups or "
                             "--depth-cuts\n");
        return EXIT_FAILURE;
    }
    // --cost
    const bool cost = take_flag(args, "--cost");
    if (cost && (depth_cuts || light_groups || adaptive_arg || robust || mattes || aovs || denoise || follow)) {
        std::fprintf(stderr, "Error: --cost is not offered together with --depth-cuts, --light-groups, --adaptive, --robust, "
                             "--mattes, --aovs, --denoise or --follow-specular\n");
        return EXIT_FAILURE;
    }
    if (denoise_cross && (adaptive || robust || mattes || light_groups || depth_cuts || cost)) {
        std::fputs(cross_alone, stderr);
        return EXIT_FAILURE;
    }
    // --halves
    const bool halves = take_flag(args, "--halves");
    if (halves && (denoise || denoise_parts || adaptive || robust || mattes || light_groups || depth_cuts || cost)) {
        std::fprintf(stderr, "Error: --halves is not offered together with --denoise, --denoise-parts, --adaptive, --robust, "
                             "--mattes, --light-groups, --depth-cuts or --cost\n");
        return EXIT_FAILURE;
    }
    nart_adaptive_params ap;
    nart_hip_adaptive_params_init(&ap);
    if (adaptive) {
        char* end = nullptr;
        ap.threshold = std::strtof(adaptive_arg, &end);
        if (!adaptive_arg[0] || *end) {
            std::fprintf(stderr, "Error: --adaptive %s\n", adaptive_arg);
            return EXIT_FAILURE;
        }
        int v = 0;
        if (min_spp_arg && (!parse_int(min_spp_arg, v) || v < 0)) {
            std::fprintf(stderr, "Error: --min-spp %s\n", min_spp_arg);
            return EXIT_FAILURE;
        }
        if (min_spp_arg) ap.min_spp = (uint32_t)v;
    }
    if (!take_device_flags(args, devices)) return EXIT_FAILURE;
    if (args.size() < 3) {
        std::fprintf(stderr, "Too few arguments given.\nUsage example: %s <scene file> <output path>\n", argv[0]);
        return EXIT_FAILURE;
    }
    nart_render_params params;
    nart_render_params_init(&params);
    if (nart_parse_args((int)args.size(), args.data(), &params) != NART_OK) {
        std::fprintf(stderr, "%s\n", nart_scene_last_error());
        return EXIT_FAILURE;
    }
    std::printf("Loading %s...\n", args[1]);
    nart_scene* scene = nullptr;
    if (nart_scene_load(args[1], &scene) != NART_OK) {
        std::fprintf(stderr, "%s\nAborting.\n", nart_scene_last_error());
        return EXIT_FAILURE;
    }
    int n = nart_load_sessions(args[1], &params, nullptr, 0);
    if (n <= 0) {
        std::fprintf(stderr, "Failed to load sessions from %s\n", args[1]);
        return EXIT_FAILURE;
    }
    std::vector<nart_render_params> sessions(n);
    nart_load_sessions(args[1], &params, sessions.data(), n);
    for (const nart_render_params& p : sessions)
        if (depth_cuts && cuts.back() > p.bounces) {
            std::fprintf(stderr, "Error: --depth-cuts %s: a session's bounce limit is %u\n", cuts_arg, p.bounces);
            return EXIT_FAILURE;
        }
    nart_ctx* ctx = nullptr;
    int rc = nart_hip_create_multi(nart_scene_blob_of(scene), devices.data(), (int)devices.size(), &ctx);
    if (rc != NART_OK) {
        std::fprintf(stderr, "Error: cannot create the HIP render context on %zu device(s) (%d)\n", devices.size(), rc);
        return EXIT_FAILURE;
    }
    uint32_t n_groups = 0;
    if (light_groups) {
        const uint32_t n_lights = nart_scene_blob_of(scene)->num_lights;
        if (group_of_light.empty()) {
            if (n_lights > NART_LIGHT_GROUPS_MAX) {
                std::fprintf(stderr, "Error: --light-groups each: the scene has %u lights, at most 8 groups are supported\n", n_lights);
                return EXIT_FAILURE;
            }
            for (uint32_t l = 0; l < n_lights; ++l) group_of_light.push_back(l);
        }
        if (group_of_light.size() != n_lights) {
            std::fprintf(stderr, "Error: --light-groups lists %zu lights, the scene has %u\n", group_of_light.size(), n_lights);
            return EXIT_FAILURE;
        }
        for (uint32_t v : group_of_light) n_groups = std::max(n_groups, v + 1);
        if (gains_arg && gain_list.size() != n_groups) {
            std::fprintf(stderr, "Error: --light-gains lists %zu gains for %u groups\n", gain_list.size(), n_groups);
            return EXIT_FAILURE;
        }
        for (float v : gain_list) light_gains.insert(light_gains.end(), 3, v);
    }
    int k = 0;
    for (const nart_render_params& p : sessions) {
        auto start = std::chrono::high_resolution_clock::now();
        std::printf("Rendering...\n");
        nart_session_geometry g;
        nart_session_geometry_of(&p, &g);
        std::vector<nart_pixel> image((size_t)g.total_width * g.total_height);
        std::vector<nart_pixel> albedo, normal, denoised, moment, robust_img, matte_ranks, matte_img;
        if (mattes) matte_ranks.resize((size_t)(mp.ranks / 2) * image.size());
        // alone, the matte call renders the beauty too; next to AOVs or the denoiser it follows their call
        const bool mattes_after = mattes && (aovs || denoise);
        if (denoise) denoised.resize(image.size());
        std::vector<uint32_t> bucket_spp;
        std::vector<nart_pixel> group_imgs, mix_img, cut_imgs, layer_imgs, cost_img, part_imgs, parts_sum, parts_mix;
        const nart_guide_params* parts_gp = follow ? &gp : nullptr;
        std::vector<nart_pixel> half_imgs, error_img;
        if (denoise_cross) {
            denoised.resize(image.size());
            error_img.resize(image.size());
        }
        if (denoise_cross && !halves && !aovs) {
            rc = nart_hip_render_denoised_cross(ctx, &p, nullptr, follow ? &gp : nullptr, denoised.data(), error_img.data(),
                                                image.data(), nullptr, nullptr);
        } else if (denoise_cross) {
            // the half buffers and the AOVs are rendered for their files anyway: the filter over them
            half_imgs.resize(2 * image.size());
            albedo.resize(image.size());
            normal.resize(image.size());
            nart_pixel* const half_b = half_imgs.data() + image.size();
            rc = nart_hip_render_halves(ctx, &p, NART_AOV_ALBEDO | NART_AOV_NORMAL, follow ? &gp : nullptr, image.data(),
                                        albedo.data(), normal.data(), half_imgs.data(), half_b, nullptr, nullptr);
            if (rc == NART_OK)
                rc = nart_hip_denoise_cross(ctx, &p, nullptr, half_imgs.data(), half_b, image.data(), albedo.data(),
                                            normal.data(), denoised.data(), error_img.data(), nullptr);
        } else if (halves) {
            half_imgs.resize(2 * image.size());
            if (aovs) {
                albedo.resize(image.size());
                normal.resize(image.size());
            }
            rc = nart_hip_render_halves(ctx, &p, aovs ? NART_AOV_ALBEDO | NART_AOV_NORMAL : 0u, follow ? &gp : nullptr,
                                        image.data(), aovs ? albedo.data() : nullptr, aovs ? normal.data() : nullptr,
                                        half_imgs.data(), half_imgs.data() + image.size(), nullptr, nullptr);
        } else if (cost) {
            uint32_t gw = 0, gh = 0;
            rc = nart_hip_cost_grid(&p, &gw, &gh);
            std::vector<nart_cost_pixel> grid((size_t)gw * gh);
            if (rc == NART_OK) rc = nart_hip_render_cost(ctx, &p, grid.data(), image.data(), nullptr);
            if (rc == NART_OK) {
                cost_img.resize(image.size());
                rc = nart_hip_cost_image(ctx, &p, grid.data(), cost_img.data());
            }
            if (rc == NART_OK) {
                unsigned long long t[4] = {0, 0, 0, 0};
                for (const nart_cost_pixel& c : grid) {
                    t[0] += c.rays_extend;
                    t[1] += c.rays_shadow;
                    t[2] += c.hits;
                    t[3] += c.steps;
                }
                std::printf("Cost: %llu extension rays, %llu shadow rays, %llu shaded hits, %llu traversal steps\n", t[0], t[1],
                            t[2], t[3]);
            }
        } else if (depth_cuts) {
            cut_imgs.resize(cuts.size() * image.size());
            rc = nart_hip_render_depth_cuts(ctx, &p, cuts.data(), (uint32_t)cuts.size(), cut_imgs.data(), image.data(), nullptr);
            if (rc == NART_OK && (depth_layers || denoise_parts)) {
                layer_imgs.resize((cuts.size() + 1) * image.size());
                rc = nart_hip_depth_layers(ctx, &p, (uint32_t)cuts.size(), cut_imgs.data(), image.data(), layer_imgs.data());
            }
            if (rc == NART_OK && denoise_parts) {
                // the guides alone (camera rays only), then the layers through the parts denoise
                albedo.resize(image.size());
                normal.resize(image.size());
                rc = follow ? nart_hip_render_guides(ctx, &p, &gp, NART_AOV_ALBEDO | NART_AOV_NORMAL, nullptr, albedo.data(),
                                                     normal.data(), nullptr, nullptr, nullptr)
                            : nart_hip_render_aovs(ctx, &p, NART_AOV_ALBEDO | NART_AOV_NORMAL, nullptr, albedo.data(),
                                                   normal.data(), nullptr, nullptr);
                part_imgs.resize(layer_imgs.size());
                parts_sum.resize(image.size());
                if (rc == NART_OK)
                    rc = nart_hip_denoise_parts(ctx, &p, nullptr, (uint32_t)cuts.size() + 1, layer_imgs.data(), albedo.data(),
                                                normal.data(), part_imgs.data(), parts_sum.data(), nullptr);
            }
        } else if (light_groups) {
            group_imgs.resize((size_t)n_groups * image.size());
            if (denoise_parts) {
                part_imgs.resize(group_imgs.size());
                parts_sum.resize(image.size());
                rc = nart_hip_render_denoised_light_groups(ctx, &p, nullptr, parts_gp, group_of_light.data(),
                                                           (uint32_t)group_of_light.size(), n_groups, part_imgs.data(),
                                                           parts_sum.data(), group_imgs.data(), image.data(), nullptr, nullptr);
                if (rc == NART_OK && gains_arg) {
                    parts_mix.resize(image.size());
                    rc = nart_hip_light_mix(ctx, &p, n_groups, light_gains.data(), part_imgs.data(), parts_mix.data());
                }
            } else {
                rc = nart_hip_render_light_groups(ctx, &p, group_of_light.data(), (uint32_t)group_of_light.size(), n_groups,
                                                  group_imgs.data(), image.data(), nullptr);
            }
            if (rc == NART_OK && gains_arg) {
                mix_img.resize(image.size());
                rc = nart_hip_light_mix(ctx, &p, n_groups, light_gains.data(), group_imgs.data(), mix_img.data());
            }
        } else if (robust) {
            robust_img.resize(image.size());
            rc = nart_hip_render_cascade(ctx, &p, &cp, robust_img.data(), image.data(), nullptr, nullptr);
        } else if (mattes && !mattes_after) {
            rc = nart_hip_render_mattes(ctx, &p, &mp, matte_ranks.data(), image.data(), nullptr, nullptr);
        } else if (adaptive) {
            // the adaptive call renders what the flags need; the denoiser then runs over its images
            const bool guides = aovs || denoise;
            if (guides) {
                albedo.resize(image.size());
                normal.resize(image.size());
            }
            if (sample_variance) moment.resize(image.size());
            bucket_spp.resize((size_t)g.n_buckets_x * g.n_buckets_y);
            nart_render_stats st;
            std::memset(&st, 0, sizeof(st));
            rc = nart_hip_render_adaptive(ctx, &p, &ap, guides ? NART_AOV_ALBEDO | NART_AOV_NORMAL : 0u, image.data(),
                                          guides ? albedo.data() : nullptr, guides ? normal.data() : nullptr,
                                          sample_variance ? moment.data() : nullptr, bucket_spp.data(), nullptr, &st,
                                          nullptr);
            if (rc == NART_OK && sample_variance)
                rc = nart_hip_denoise_moment(ctx, &p, nullptr, image.data(), albedo.data(), normal.data(), moment.data(),
                                             denoised.data(), nullptr);
            else if (rc == NART_OK && denoise)
                rc = nart_hip_denoise(ctx, &p, nullptr, image.data(), albedo.data(), normal.data(), denoised.data(),
                                      nullptr);
            uint32_t levels[32], nl = 0;
            if (rc == NART_OK && nart_hip_adaptive_levels(&ap, p.spp, levels, &nl) == NART_OK) {
                // a bucket was rendered at every level up to the one it ended on
                std::printf("Adaptive: levels");
                for (uint32_t l = 0; l < nl; ++l) {
                    size_t cnt = 0;
                    for (uint32_t s : bucket_spp) cnt += s >= levels[l];
                    std::printf(" %u spp x %zu buckets%s", levels[l], cnt, l + 1 < nl ? "," : ";");
                }
                std::printf(" %llu of %llu samples\n", (unsigned long long)st.samples,
                            (unsigned long long)p.image_width * p.image_height * p.spp);
            }
        } else if (follow && aovs) {
            albedo.resize(image.size());
            normal.resize(image.size());
            if (sample_variance) moment.resize(image.size());
            rc = nart_hip_render_guides(ctx, &p, &gp, NART_AOV_ALBEDO | NART_AOV_NORMAL, image.data(), albedo.data(),
                                        normal.data(), sample_variance ? moment.data() : nullptr, nullptr, nullptr);
            if (rc == NART_OK && sample_variance)
                rc = nart_hip_denoise_moment(ctx, &p, nullptr, image.data(), albedo.data(), normal.data(), moment.data(),
                                             denoised.data(), nullptr);
            else if (rc == NART_OK && denoise)
                rc = nart_hip_denoise(ctx, &p, nullptr, image.data(), albedo.data(), normal.data(), denoised.data(),
                                      nullptr);
        } else if (follow) {
            rc = nart_hip_render_denoised_guides(ctx, &p, nullptr, &gp, sample_variance ? 1 : 0, image.data(),
                                                 denoised.data(), nullptr, nullptr);
        } else if (aovs && sample_variance) {
            albedo.resize(image.size());
            normal.resize(image.size());
            moment.resize(image.size());
            rc = nart_hip_render_moment(ctx, &p, NART_AOV_ALBEDO | NART_AOV_NORMAL, image.data(), albedo.data(),
                                        normal.data(), moment.data(), nullptr, nullptr, nullptr);
            if (rc == NART_OK)
                rc = nart_hip_denoise_moment(ctx, &p, nullptr, image.data(), albedo.data(), normal.data(), moment.data(),
                                             denoised.data(), nullptr);
        } else if (aovs) {
            albedo.resize(image.size());
            normal.resize(image.size());
            rc = nart_hip_render_aovs(ctx, &p, NART_AOV_ALBEDO | NART_AOV_NORMAL, image.data(), albedo.data(),
                                      normal.data(), nullptr, nullptr);
            if (rc == NART_OK && denoise)
                rc = nart_hip_denoise(ctx, &p, nullptr, image.data(), albedo.data(), normal.data(), denoised.data(),
                                      nullptr);
        } else if (sample_variance) {
            rc = nart_hip_render_denoised_moment(ctx, &p, nullptr, image.data(), denoised.data(), nullptr, nullptr);
        } else if (denoise) {
            rc = nart_hip_render_denoised(ctx, &p, nullptr, image.data(), denoised.data(), nullptr, nullptr);
        } else {
            rc = nart_hip_render(ctx, &p, image.data(), nullptr);
        }
        if (rc == NART_OK && mattes_after)
            rc = nart_hip_render_mattes(ctx, &p, &mp, matte_ranks.data(), nullptr, nullptr, nullptr);
        if (rc == NART_OK && mattes && matte_ids_arg) {
            matte_img.resize(image.size());
            rc = nart_hip_matte_extract(ctx, &p, &mp, matte_ranks.data(), matte_mask, matte_img.data());
        }
        if (rc != NART_OK) {
            std::fprintf(stderr, "Error: render failed (%d): %s\n", rc, nart_hip_last_error(ctx));
            return EXIT_FAILURE;
        }
        // main.cpp:44-49: <out>.exr for one session, <out>_<n>.exr for several
        const std::string stem = std::string(args[2]) + (n == 1 ? std::string() : "_" + std::to_string(k++));
        std::string path = stem + ".exr";
        std::printf("Writing to %s...\n", path.c_str());
        if (nart_write_exr(path.c_str(), &p, image.data(), 3) != NART_OK) {
            std::fprintf(stderr, "%s\n", nart_scene_last_error());
            return EXIT_FAILURE;
        }
        std::vector<std::pair<std::string, const nart_pixel*>> extra;
        if (aovs) {
            extra.push_back({".albedo.exr", albedo.data()});
            extra.push_back({".normal.exr", normal.data()});
        }
        if (denoise || denoise_cross) extra.push_back({".denoised.exr", denoised.data()});
        if (denoise_cross) extra.push_back({".error.exr", error_img.data()});
        if (robust) extra.push_back({".robust.exr", robust_img.data()});
        for (uint32_t i = 0; mattes && i < mp.ranks / 2; ++i)
            extra.push_back({".matte.0" + std::to_string(i) + ".exr", matte_ranks.data() + (size_t)i * image.size()});
        if (mattes && matte_ids_arg) extra.push_back({".matte.exr", matte_img.data()});
        for (uint32_t i = 0; i < (light_groups ? n_groups : 0u); ++i)
            extra.push_back({".light.0" + std::to_string(i) + ".exr", group_imgs.data() + (size_t)i * image.size()});
        if (light_groups && gains_arg) extra.push_back({".mix.exr", mix_img.data()});
        auto two = [](uint32_t v) { return (v < 10 ? "0" : "") + std::to_string(v); };
        for (size_t i = 0; depth_cuts && i < cuts.size(); ++i)
            extra.push_back({".depth." + two(cuts[i]) + ".exr", cut_imgs.data() + i * image.size()});
        for (size_t i = 0; depth_layers && i <= cuts.size(); ++i)
            extra.push_back({".layer." + two((uint32_t)i) + ".exr", layer_imgs.data() + i * image.size()});
        if (denoise_parts) {
            const size_t n_parts = light_groups ? n_groups : cuts.size() + 1;
            for (size_t i = 0; i < n_parts; ++i)
                extra.push_back({std::string(light_groups ? ".light." : ".layer.") + two((uint32_t)i) + ".denoised.exr",
                                 part_imgs.data() + i * image.size()});
            extra.push_back({".denoised.exr", parts_sum.data()});
            if (light_groups && gains_arg) extra.push_back({".mix.denoised.exr", parts_mix.data()});
        }
        if (cost) extra.push_back({".cost.exr", cost_img.data()});
        for (size_t h = 0; halves && h < 2; ++h)
            extra.push_back({".half." + std::to_string(h) + ".exr", half_imgs.data() + h * image.size()});
        std::vector<nart_pixel> spp_img;
        if (adaptive) {
            // pixel (x, y) of the cropped image was traced by bucket (x / B, y / B)
            spp_img.assign(image.size(), nart_pixel{{0.f, 0.f, 0.f, 0.f}, 0.f});
            for (uint32_t y = 0; y < p.image_height; ++y)
                for (uint32_t x = 0; x < p.image_width; ++x) {
                    const float s = (float)bucket_spp[(size_t)(y / p.bucket_size) * g.n_buckets_x + x / p.bucket_size];
                    spp_img[(size_t)(y + g.filter_bounds) * g.total_width + x + g.filter_bounds] =
                        nart_pixel{{s, s, s, 1.f}, 1.f};
                }
            extra.push_back({".spp.exr", spp_img.data()});
        }
        for (const auto& e : extra) {
            path = stem + e.first;
            std::printf("Writing to %s...\n", path.c_str());
            if (nart_write_exr(path.c_str(), &p, e.second, 3) != NART_OK) {
                std::fprintf(stderr, "%s\n", nart_scene_last_error());
                return EXIT_FAILURE;
            }
        }
        std::chrono::duration<float> d = std::chrono::high_resolution_clock::now() - start;
        std::printf("Completed in %gs\n", d.count());
        std::fflush(stdout);
    }
    nart_hip_destroy(ctx);
    nart_scene_free(scene);
    return 0;
}
