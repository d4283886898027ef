// Prints the decisions of host/path_build.h (plan_build) with the cost image for
// tests/test_path_build_cost.py: path_build_depth_check's "build" request with cost appended.
//   build features has_env specialize counters bounces variant stack_depth num_nodes n_slots resident_k
//         rq_blocks has_prim  NART_RQ_LDS_LIMIT NART_LEAN_STACK NART_LEAN_ROUNDS  depth_cuts cost
// The answer is path_build_depth_check's with cs= added after dc=.  A cost launch has no camera-hit
// buffer to fill (render.hip launch_render passes has_prim = false for it).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "../../nart_amd/csrc/host/path_build.h"

using namespace nd;

static Knob knob(std::istream& is) {
    std::string t;
    is >> t;
    if (t == "-") return Knob{};
    if (t == "=") return Knob{true, false, 0.0};
    return Knob{true, true, std::atof(t.c_str())};
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string what;
        is >> what;
        if (what != "build") return 1;
        PathBuildIn in;
        int env, spec, counters, has_prim, dc, cs;
        uint32_t rq_blocks;
        is >> in.features >> env >> spec >> counters >> in.bounces >> in.variant >> in.stack_depth >> in.num_nodes >>
            in.n_slots >> in.resident_k >> rq_blocks >> has_prim;
        in.has_env = env, in.counters = counters;
        in.specialize = spec == 0 ? Specialize::Off : (spec == 1 ? Specialize::On : Specialize::Lean);
        in.rq_lds_limit = knob(is), in.lean_stack = knob(is), in.lean_rounds = knob(is);
        is >> dc >> cs;
        if (!is) return 1;
        in.depth_cuts = dc != 0;
        in.cost = cs != 0;
        const PathBuild b = plan_build(in);
        std::printf("error=%s ext=%d count=%d env=%d fm=%u wv=%d pr=%d rq=%d rq_block=%u stack_lds=%u k_nodes=%u "
                    "k_lds=%zu rq_nodes=%u rq_lds=%zu fm_used=%u lg=%d dc=%d cs=%d unsupported=%d",
                    b.error ? "1" : "0", b.id.ext, b.id.count, b.id.env, b.id.fm, b.id.wv, b.id.pr, b.rq, b.rq_block,
                    b.stack_lds, b.k_render.nodes, b.k_render.bytes, b.rq_lds.nodes, b.rq_lds.bytes, b.fm_used, b.id.lg,
                    b.id.dc, b.id.cs, b.unsupported);
        // the launch as render.hip launch_render states it
        const PathLaunchIn li{in.n_slots, in.resident_k, rq_blocks * (b.rq_block / 256), b.rq_block, b.id.wv, b.id.pr,
                              b.id.env, b.rq, b.id.fm != FT_ALL, has_prim != 0 && !b.id.cs};
        const PathSchedule s = plan_path(li, SchedKnobs{});
        std::printf(" p_error=%d p_shape=%d p_k=%u p_pairs=%u p_half=%u p_quad=%u p_rq_prio=%u p_blocks=%u p_sched=%u # %s\n",
                    s.error ? 1 : 0, (int)s.shape, s.k, s.pairs, s.half, s.quad, s.rq_prio, s.blocks, s.sched, b.error ? b.error : "");
    }
    return 0;
}
