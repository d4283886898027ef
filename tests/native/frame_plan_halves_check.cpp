// Prints the decisions of host/frame_plan.h for tests/test_frame_plan_halves.py: frame_plan_cost_check's
// request with the halves flag appended.  One request per line of standard input:
//   rules beauty aov_bits moment adaptive K matte n_ids integrator guide_bits max_follow light_groups depth_cuts cost halves
//        (halves: 1 the half buffers, 0 off; the rest as tests/native/frame_plan_cost_check.cpp)
// One answer per line, in frame_plan_check's form:
//   code|message|kind:index,...|pass,...|path_kernel|record_bytes
// With the argument "constants": one line, OutputKind::DepthCut, HalfA and HalfB, PASS_GUIDE, N_PASSES,
// PASS_HALVES, PASS_SLOTS, pass_of(HalfA), pass_of(HalfB), FRAME_MAX_OUTPUTS and the size of PASS_OF.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "../../nart_amd/csrc/host/frame_plan.h"

using namespace nd;

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "constants")) {
        std::printf("%u %u %u %u %u %u %u %u %u %u %u\n", (unsigned)OutputKind::DepthCut, (unsigned)OutputKind::HalfA,
                    (unsigned)OutputKind::HalfB, (unsigned)PASS_GUIDE, (unsigned)N_PASSES, (unsigned)PASS_HALVES,
                    (unsigned)PASS_SLOTS, (unsigned)pass_of(OutputKind::HalfA), (unsigned)pass_of(OutputKind::HalfB),
                    (unsigned)FRAME_MAX_OUTPUTS, (unsigned)(sizeof(PASS_OF) / sizeof(PASS_OF[0])));
        return 0;
    }
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string rules;
        unsigned beauty = 0, bits = 0, moment = 0, adaptive = 0, K = 0, matte = 0, n_ids = 0, integrator = 0, gbits = 0,
                 max_follow = 0, groups = 0, cuts = 0, cost = 0, halves = 0;
        is >> rules >> beauty >> bits >> moment >> adaptive >> K >> matte >> n_ids >> integrator >> gbits >> max_follow >> groups >>
            cuts >> cost >> halves;
        if (!is || (rules != "frame" && rules != "buckets")) {
            std::fprintf(stderr, "bad request: %s\n", line.c_str());
            return 1;
        }
        FrameAsk a(integrator);
        a.beauty = beauty != 0;
        a.aov[0] = (bits & 1u) != 0;
        a.aov[1] = (bits & 2u) != 0;
        a.moment = moment != 0;
        a.adaptive = adaptive != 0;
        a.cascade.K = K;
        a.matte.on = matte != 0;
        a.matte.n_ids = n_ids;
        a.guide[0] = (gbits & 1u) != 0;
        a.guide[1] = (gbits & 2u) != 0;
        a.max_follow = max_follow;
        a.light_groups = groups;
        a.depth_cuts = cuts;
        a.cost = cost != 0;
        a.halves = halves != 0;
        const FramePlan plan = plan_frame(a, rules == "frame" ? PlanRules::Frame : PlanRules::Buckets);
        std::printf("%d|%s|", plan.code, plan.message.c_str());
        for (uint32_t i = 0; i < plan.n_outputs; ++i)
            std::printf("%s%u:%u", i ? "," : "", (unsigned)plan.outputs[i].kind, plan.outputs[i].index);
        std::printf("|");
        for (uint32_t i = 0; i < plan.n_passes; ++i) std::printf("%s%u", i ? "," : "", (unsigned)plan.passes[i]);
        std::printf("|%d|%u\n", plan.path_kernel ? 1 : 0, plan.record_bytes);
    }
    return 0;
}
