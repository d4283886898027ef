// Prints the decisions of host/path_schedule.h and device/queue_layout.h for
// tests/test_path_schedule.py.  One query per line of standard input:
//   plan n_slots resident_k resident_rq rq_block wv pr env rq specialized has_prim  K*10
//        (knobs in SchedKnobs order: primary_packet rq_prio rq_pairs rq_half rq_quad rq_setprio
//         rq_order rq_topf probe_sub queue_k; "-" = unset)
//   queue n W k prio pairs half quad
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "../../nart_amd/csrc/host/path_schedule.h"

using namespace nd;

static Knob knob(const std::string& t) {
    if (t == "-") return Knob{};
    return Knob{true, !t.empty(), std::atof(t.c_str())};
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string what;
        is >> what;
        if (what == "plan") {
            PathLaunchIn in;
            int pr, env, rq, sp, hp;
            is >> in.n_slots >> in.resident_k >> in.resident_rq >> in.rq_block >> in.wv >> pr >> env >> rq >> sp >> hp;
            in.pr = pr, in.env = env, in.rq = rq, in.specialized = sp, in.has_prim = hp;
            std::string t[10];
            for (auto& x : t) is >> x;
            SchedKnobs k;
            Knob* dst[10] = {&k.primary_packet, &k.rq_prio,  &k.rq_pairs, &k.rq_half,   &k.rq_quad,
                             &k.rq_setprio,     &k.rq_order, &k.rq_topf,  &k.probe_sub, &k.queue_k};
            for (int i = 0; i < 10; ++i) *dst[i] = knob(t[i]);
            const PathSchedule s = plan_path(in, k);
            std::printf("error=%d shape=%d primary=%d packet=%u resident=%u W=%u queue_room=%u probe=%d probe_sub=%u "
                        "probe_blocks=%u order=%u E=%u k=%u pairs=%u half=%u quad=%u rq_prio=%u rq_setprio=%u "
                        "rq_quorum=%u qlen=%u qbase=%u blocks=%u sched=%u\n",
                        s.error ? 1 : 0, (int)s.shape, s.primary ? 1 : 0, s.packet, s.resident, s.W, s.queue_room,
                        (int)s.probe, s.probe_sub, s.probe_blocks, s.order, s.E, s.k, s.pairs, s.half, s.quad, s.rq_prio,
                        s.rq_setprio, s.rq_quorum, s.qlen, s.qbase, s.blocks, s.sched);
        } else if (what == "queue") {
            uint32_t n, W, k, prio, pairs, half, quad;
            is >> n >> W >> k >> prio >> pairs >> half >> quad;
            const uint32_t len = queue_length(n, W, k, pairs, quad);
            std::printf("%u", len);
            for (uint32_t p = 0; p < len; ++p) {
                const QueueEntry e = queue_entry(p, n, W, k, prio, pairs, half, quad);
                std::printf(" %u %u %u", e.top, e.index, e.flags);
            }
            std::printf("\n");
        }
    }
    return 0;
}
