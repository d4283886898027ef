// Prints the messages of host/stage_params.h depth_cuts_error for tests/test_depth_cut_params.py.
// One request per line of standard input:
//   cuts n_cuts bounces null  value*          (null 1: the cuts pointer is null)
// One answer per line: the message, or "ok".
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../nart_amd/csrc/host/stage_params.h"

using namespace nd;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string what;
        is >> what;
        if (what != "cuts") return 1;
        uint32_t K, bounces, null_cuts, v;
        is >> K >> bounces >> null_cuts;
        std::vector<uint32_t> cuts;
        while (is >> v) cuts.push_back(v);
        cuts.resize(K > 16 ? 16 : (K > cuts.size() ? K : cuts.size()) + 1);
        const char* why = depth_cuts_error(null_cuts ? nullptr : cuts.data(), K, bounces);
        std::printf("%s\n", why ? why : "ok");
    }
    return 0;
}
