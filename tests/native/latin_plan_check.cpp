// Prints host/latin_plan.h plan_latin for tests/test_latin_plan.py.  One query per line of standard input:
//   n_slots spp sample_capacity_bytes
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../../nart_amd/csrc/host/latin_plan.h"

using namespace nd;

static void grid(const char* name, const Grid& g) {
    std::printf(" %s_blocks=%u %s_threads=%u %s_lds=%zu", name, g.blocks, name, g.threads, name, g.lds);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        uint32_t n_slots, spp;
        size_t capacity;
        if (!(is >> n_slots >> spp >> capacity)) continue;
        const LatinPlan p = plan_latin(n_slots, spp, capacity);
        std::printf("form=%d n2=%u words=%zu stw=%zu cx=%zu cy=%zu sx=%zu sy=%zu st=%zu perm_block=%u", (int)p.form, p.n2,
                    p.words, p.stw, p.cx, p.cy, p.sx, p.sy, p.st, p.perm_block);
        grid("draws", p.draws), grid("perm", p.perm), grid("emit", p.emit), grid("one", p.one);
        std::printf("\n");
    }
    return 0;
}
