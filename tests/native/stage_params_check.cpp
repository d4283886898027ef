// Prints the decisions of host/stage_params.h for tests/test_stage_params.py.  One case per line of
// standard input, floats as strtof reads them (hexadecimal floats, inf, nan); "null" in the fields'
// place passes a null pointer (the defaults):
//   defaults
//   denoise   iterations normal_squarings sigma_color sigma_depth depth_eps sigma_coverage albedo_floor
//   guide     max_follow
//   adaptive  spp min_spp growth threshold floor          (spp also before "null")
//   cascade   layers start base kappa
//   matte     kind ranks
//   image     image_width image_height filter_width       (check_image_size)
//   variance  spp                                         (check_sample_variance)
//   cascade_frame image_width image_height filter_width spp
// One answer per line: message|the struct's fields after the call|levels, fields and levels separated
// by spaces, floats as %a.  "defaults" answers the five structs' defaults, separated by '|'.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../nart_amd/csrc/host/stage_params.h"

using namespace nd;

namespace {

struct Fields {
    std::vector<std::string> tok;
    size_t at = 0;
    bool null() const { return tok.size() == 1 && tok[0] == "null"; }
    uint32_t u() { return (uint32_t)std::strtoull(tok.at(at++).c_str(), nullptr, 10); }
    float f() { return std::strtof(tok.at(at++).c_str(), nullptr); }
};

void print(const nart_denoise_params& d) {
    std::printf("%u %u %a %a %a %a %a", d.iterations, d.normal_squarings, d.sigma_color, d.sigma_depth, d.depth_eps,
                d.sigma_coverage, d.albedo_floor);
}
void print(const nart_guide_params& g) { std::printf("%u", g.max_follow); }
void print(const nart_adaptive_params& a) { std::printf("%u %u %a %a", a.min_spp, a.growth, a.threshold, a.floor); }
void print(const nart_cascade_params& c) { std::printf("%u %a %a %a", c.layers, c.start, c.base, c.kappa); }
void print(const nart_matte_params& m) { std::printf("%u %u", m.kind, m.ranks); }

void message(const char* why) { std::printf("%s|", why ? why : ""); }

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string what, t;
        is >> what;
        Fields in;
        while (is >> t) in.tok.push_back(t);
        try {
            if (what == "defaults") {
                const nart_denoise_params d = DENOISE_DEFAULTS;
                const nart_guide_params g = GUIDE_DEFAULTS;
                const nart_adaptive_params a = ADAPTIVE_DEFAULTS;
                const nart_cascade_params c = CASCADE_DEFAULTS;
                const nart_matte_params m = MATTE_DEFAULTS;
                print(d), std::printf("|"), print(g), std::printf("|"), print(a), std::printf("|"), print(c), std::printf("|"), print(m);
            } else if (what == "denoise") {
                nart_denoise_params v = {}, out = {};
                if (!in.null()) v = {in.u(), in.u(), in.f(), in.f(), in.f(), in.f(), in.f()};
                message(denoise_params_error(in.null() ? nullptr : &v, out));
                print(out), std::printf("|");
            } else if (what == "guide") {
                nart_guide_params v = {}, out = {};
                if (!in.null()) v = {in.u()};
                message(guide_params_error(in.null() ? nullptr : &v, out));
                print(out), std::printf("|");
            } else if (what == "adaptive") {
                const uint32_t spp = in.u();
                in.tok.erase(in.tok.begin()), in.at = 0;
                nart_adaptive_params v = {}, out = {};
                if (!in.null()) v = {in.u(), in.u(), in.f(), in.f()};
                const char* why = adaptive_params_error(in.null() ? nullptr : &v, out, spp);
                message(why);
                print(out), std::printf("|");
                if (!why) {
                    const std::vector<uint32_t> l = adaptive_levels(out, spp);
                    for (size_t i = 0; i < l.size(); ++i) std::printf("%s%u", i ? " " : "", l[i]);
                }
            } else if (what == "cascade") {
                nart_cascade_params v = {}, out = {};
                CascadeLevels lv;
                if (!in.null()) v = {in.u(), in.f(), in.f(), in.f()};
                const char* why = cascade_params_error(in.null() ? nullptr : &v, out, lv);
                message(why);
                print(out), std::printf("|");
                if (!why) {
                    if (lv.base != out.base) return 2;
                    for (uint32_t j = 0; j < lv.K; ++j) std::printf("%s%a", j ? " " : "", lv.b[j]);
                }
            } else if (what == "matte") {
                nart_matte_params v = {}, out = {};
                if (!in.null()) v = {in.u(), in.u()};
                message(matte_params_error(in.null() ? nullptr : &v, out));
                print(out), std::printf("|");
            } else if (what == "image" || what == "cascade_frame" || what == "variance") {
                nart_render_params p = {};
                if (what == "variance") {
                    p.spp = in.u();
                } else {
                    p.image_width = in.u(), p.image_height = in.u(), p.filter_width = in.f();
                    if (what == "cascade_frame") p.spp = in.u();
                }
                message(what == "image" ? check_image_size(&p) : what == "variance" ? check_sample_variance(&p) : check_cascade_frame(&p));
                std::printf("|");
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
