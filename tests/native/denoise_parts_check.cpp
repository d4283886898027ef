// Prints the decisions of host/denoise_parts_plan.h and of denoise_parts_error (host/stage_params.h) for
// tests/test_denoise_parts_plan.py and tests/test_denoise_parts_params.py.  One case per line of standard
// input, floats as strtof reads them:
//   plan   K knob
//       -> n_chunks|first:size first:size ...
//   error  n_parts images_given dp gp
//       dp: "null", or iterations normal_squarings sigma_color sigma_depth depth_eps sigma_coverage albedo_floor
//       gp: "null", or max_follow
//       -> message|the denoise fields after the call|max_follow after the call
//   max
//       -> NART_DENOISE_PARTS_MAX PARTS_MAX PARTS_CHUNK_MAX
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../nart_amd/csrc/host/denoise_parts_plan.h"
#include "../../nart_amd/csrc/host/stage_params.h"

using namespace nd;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string what, t;
        is >> what;
        std::vector<std::string> tok;
        while (is >> t) tok.push_back(t);
        size_t at = 0;
        auto u = [&]() { return (uint32_t)std::strtoull(tok.at(at++).c_str(), nullptr, 10); };
        auto f = [&]() { return std::strtof(tok.at(at++).c_str(), nullptr); };
        try {
            if (what == "plan") {
                const uint32_t K = u(), knob = u();
                const PartsPlan plan = plan_denoise_parts(K, knob);
                std::printf("%u|", plan.n_chunks);
                for (uint32_t j = 0; j < plan.n_chunks; ++j) std::printf("%s%u:%u", j ? " " : "", plan.first[j], plan.size[j]);
            } else if (what == "error") {
                const uint32_t n_parts = u();
                const bool given = u() != 0;
                nart_denoise_params dp = {}, d = {};
                nart_guide_params gp = {}, g = {};
                const bool dp_null = tok.at(at) == "null";
                if (dp_null) ++at;
                else dp = {u(), u(), f(), f(), f(), f(), f()};
                const bool gp_null = tok.at(at) == "null";
                if (gp_null) ++at;
                else gp = {u()};
                const char* why = denoise_parts_error(n_parts, given, dp_null ? nullptr : &dp, d, gp_null ? nullptr : &gp, g);
                std::printf("%s|%u %u %a %a %a %a %a|%u", why ? why : "", d.iterations, d.normal_squarings, d.sigma_color,
                            d.sigma_depth, d.depth_eps, d.sigma_coverage, d.albedo_floor, g.max_follow);
            } else if (what == "max") {
                std::printf("%u %u %u", NART_DENOISE_PARTS_MAX, PARTS_MAX, PARTS_CHUNK_MAX);
            } else {
                throw std::out_of_range(what);
            }
        } catch (const std::out_of_range&) {
            std::fprintf(stderr, "bad case: %s\n", line.c_str());
            return 1;
        }
        std::printf("\n");
    }
    return 0;
}
