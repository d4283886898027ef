// Prints the decisions of host/splat_plan.h for tests/test_splat_plan.py.  One query per line of standard
// input; a knob is a number, an empty-valued "=" or "-" (unset):
//   choice mode volume B fb tile n_buckets n_cus lut_ok small_col4  NART_SKEW_BANDS
//   launch mode skew rows bands fb tile thr_ok invB_ok lut_cells nbk
//   scalars fw B
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "../../nart_amd/csrc/host/splat_plan.h"

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
        if (what == "choice") {
            SplatIn in;
            int volume, lut_ok, small;
            is >> in.mode >> volume >> in.B >> in.fb >> in.tile >> in.n_buckets >> in.n_cus >> lut_ok >> small;
            in.volume = volume, in.lut_ok = lut_ok, in.small_col4 = small;
            in.skew_bands = knob(is);
            const SplatChoice c = plan_splat(in);
            std::printf("mode=%d skew=%d rows=%d bands=%u\n", c.mode, c.skew, c.rows, c.bands);
        } else if (what == "launch") {
            SplatChoice c;
            int skew, rows, thr_ok, invB_ok;
            uint32_t fb, tile, lut_cells, nbk;
            is >> c.mode >> skew >> rows >> c.bands >> fb >> tile >> thr_ok >> invB_ok >> lut_cells >> nbk;
            c.skew = skew, c.rows = rows;
            const SplatLaunch l = splat_launch(c, fb, tile, thr_ok, invB_ok, lut_cells, nbk);
            std::printf("kernel=%d fb=%u bands=%u lut=%d thr=%d per_block=%u blocks=%u threads=%u lds=%zu sched=%u\n",
                        (int)l.kernel, l.fb, l.bands, l.lut, l.thr, l.per_block, l.blocks, l.threads, l.lds, l.sched);
        } else if (what == "scalars") {
            float fw;
            uint32_t B;
            is >> fw >> B;
            const SplatScalars s = splat_scalars(fw, 4, B, 2, B + 4, 3, 100, 80, 7, 9);
            std::printf("idx_scale=%.9g invB=%.9g invFw=%.9g\n", s.idx_scale, s.invB, s.invFw);
        }
    }
    return 0;
}
