// Cuts a bucket list into batches with host/bucket_batch.h gather_batch, as render.hip render_buckets does, for
// tests/test_bucket_batch.py.  One list per line of standard input:
//   B n_buckets_x total_width total_height image_width image_height limit  id*
// and one line of output per list, its batches separated by " ; ", each
//   b1 counted(so far) base,... xy,...
// A line "rect x0 y0 w h" prints append_rect's pixels.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../nart_amd/csrc/host/bucket_batch.h"

using namespace nd;

static void list(const std::vector<uint32_t>& v) {
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%u", i ? "," : "", v[i]);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::vector<uint32_t> xy, base;
        if (line.compare(0, 5, "rect ") == 0) {
            std::string word;
            uint32_t x0, y0, w, h;
            is >> word >> x0 >> y0 >> w >> h;
            append_rect(xy, x0, y0, w, h);
            list(xy);
            std::printf("\n");
            continue;
        }
        BucketGrid g;
        size_t limit;
        is >> g.B >> g.n_buckets_x >> g.total_width >> g.total_height >> g.image_width >> g.image_height >> limit;
        std::vector<uint32_t> ids;
        for (uint32_t id; is >> id;) ids.push_back(id);
        const uint32_t n = (uint32_t)ids.size();
        uint64_t counted = 0;
        for (uint32_t b0 = 0, b1; b0 < n; b0 = b1) {
            b1 = gather_batch(g, ids.data(), b0, n, limit, xy, base, counted);
            std::printf("%s%u %llu ", b0 ? " ; " : "", b1, (unsigned long long)counted);
            list(base);
            std::printf(" ");
            list(xy);
            if (b1 <= b0) return 1;  // (a batch always takes a bucket)
        }
        std::printf("\n");
    }
    return 0;
}
