// Prints the messages of host/stage_params.h light_groups_error and light_mix_error for
// tests/test_light_group_params.py.  One request per line of standard input:
//   groups n_groups n_lights scene_lights null_map  value*          (null_map 1: the map pointer is null)
//   mix    n_groups null_bits  gain*     (null_bits: 1 gains, 2 groups, 4 out null; gains as strtof reads them)
// One answer per line: the message, or "ok".
#include <cstdio>
#include <cstdlib>
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
        const char* why = nullptr;
        if (what == "groups") {
            uint32_t G, n, scene, null_map, v;
            is >> G >> n >> scene >> null_map;
            std::vector<uint32_t> map;
            while (is >> v) map.push_back(v);
            map.resize(n + 1);
            why = light_groups_error(null_map ? nullptr : map.data(), n, scene, G);
        } else if (what == "mix") {
            uint32_t G, nulls;
            is >> G >> nulls;
            std::vector<float> gains;
            std::string t;
            while (is >> t) gains.push_back(std::strtof(t.c_str(), nullptr));
            gains.resize(3 * 9);
            int some = 0;
            why = light_mix_error(G, (nulls & 1u) ? nullptr : gains.data(), (nulls & 2u) ? nullptr : &some,
                                  (nulls & 4u) ? nullptr : &some);
        } else {
            return 1;
        }
        std::printf("%s\n", why ? why : "ok");
    }
    return 0;
}
