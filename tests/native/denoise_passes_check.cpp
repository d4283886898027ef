// Prints the decisions of host/denoise_passes.h for tests/test_denoise_passes.py.  One case per line of
// standard input:
//   passes iterations variance_kernel
//   parts  K knob iterations sum
//       -> n|kind:halo:slot:in:out:chunk:step ...     (kind: prepare variance atrous finalize sum)
//   work   plain|cross|parts [K] npx
//       -> bytes per pixel|total bytes|offset:bytes:element-size ...|float4 planes by name|float planes by name
//          (offsets: the float4 planes, then the float planes; by name: indices into each group)
//   limits
//       -> DN_MAX_ITERATIONS DN_SLOTS DN_MAX_LAUNCHES DN_EVENT_BUDGET
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../nart_amd/csrc/host/denoise_passes.h"

using namespace nd;

static void print(const DnSequence& s) {
    static const char* names[] = {"prepare", "variance", "atrous", "finalize", "sum"};
    std::printf("%u|", s.n);
    for (uint32_t k = 0; k < s.n; ++k) {
        const DnLaunch& l = s.launch[k];
        std::printf("%s%s:%u:%u:%d:%d:%u:%u", k ? " " : "", names[(int)l.kind], l.halo, l.slot, l.in, l.out, l.chunk, l.step);
    }
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string what, t;
        is >> what;
        std::vector<std::string> tok;
        while (is >> t) tok.push_back(t);
        size_t at = 0;
        auto u = [&]() { return std::strtoull(tok.at(at++).c_str(), nullptr, 10); };
        try {
            if (what == "passes") {
                const uint32_t it = (uint32_t)u();
                print(plan_denoise_passes(it, u() != 0));
            } else if (what == "parts") {
                const uint32_t K = (uint32_t)u(), knob = (uint32_t)u(), it = (uint32_t)u();
                print(plan_denoise_parts_passes(plan_denoise_parts(K, knob), it, u() != 0));
            } else if (what == "work") {
                const std::string family = tok.at(at++);
                const DnWorkLayout w = family == "plain"   ? DN_WORK_PLAIN
                                       : family == "cross" ? DN_WORK_CROSS
                                                           : dn_work_parts((uint32_t)u());
                const size_t npx = u();
                std::printf("%zu|%zu|", w.bytes_per_pixel(), w.bytes_per_pixel() * npx);
                for (uint32_t p = 0; p < w.n4(); ++p) std::printf("%s%zu:%zu:16", p ? " " : "", w.off4(p, npx), 16 * npx);
                for (uint32_t p = 0; p < w.n1(); ++p) std::printf(" %zu:%zu:4", w.off1(p, npx), 4 * npx);
                // the planes by name: guide, centre, signals [ping-pong][c] | cov, slope, alphas
                std::printf("|%u %u", w.guide(), w.centre());
                for (uint32_t pp = 0; pp < 2; ++pp)
                    for (uint32_t c = 0; c < w.n_sig; ++c) std::printf(" %u", w.sig(pp, c));
                std::printf("|%u %u", w.cov(), w.slope());
                for (uint32_t k = 0; k < w.n_alpha; ++k) std::printf(" %u", w.alpha(k));
            } else if (what == "limits") {
                std::printf("%u %u %u %u", DN_MAX_ITERATIONS, DN_SLOTS, DN_MAX_LAUNCHES, DN_EVENT_BUDGET);
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
