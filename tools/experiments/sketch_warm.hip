// sketch_warm.hip -- how long a warm-up kp_occ_sketch_kernel's chunks need (profiles/occ_cut.md), through kp_sketch.h itself.
//
// Host only, no GPU: for sequences of 700 bases (random, unit repeats of period 1, 2, 3, 7 and 12, N runs) and every chunk
// start s0 of a grid, the seeds that start at or behind s0 are emitted once by a state that ran from the sequence's first base
// and once by a fresh state that starts `warm` bases before s0, with the kernel's own loop: reset, step, filter on the start,
// kp_sketch_final at the sequence's end.  Prints, per warm-up length, the number of chunk starts at which the two lists differ.
//
//   hipcc -O2 -std=c++17 --offload-arch=gfx950 -I kaptive_amd/csrc tools/experiments/sketch_warm.hip -o sketch_warm && ./sketch_warm
#include <cstdio>
#include <random>
#include <tuple>
#include <vector>

#include "kp_sketch.h"

using Seeds = std::vector<std::tuple<int64_t, uint32_t, uint32_t>>;

static Seeds sketch_from(const std::vector<uint8_t> &c, int64_t from, int64_t s0) {
    Seeds out;
    auto emit = [&](int64_t t, uint32_t z, uint32_t x) { if (t >= s0) out.emplace_back(t, z, x); };
    KpSketchState st;
    kp_sketch_reset(st);
    const int64_t n = (int64_t)c.size();
    for (int64_t i = from; i < n; ++i) kp_sketch_step(st, i, c[i], emit);
    kp_sketch_final(st, n - 1, emit);
    return out;
}

int main() {
    std::mt19937 rng(5);
    std::vector<std::vector<uint8_t>> seqs;
    auto random_seq = [&]() { std::vector<uint8_t> c(700); for (auto &b : c) b = rng() & 3u; return c; };
    for (int i = 0; i < 30; ++i) seqs.push_back(random_seq());
    const std::vector<std::vector<uint8_t>> units = {{0}, {0, 1}, {0, 1, 2}, {0, 1, 2, 3, 3, 2, 0}, {0, 1, 2, 2, 3, 1, 0, 3, 3, 2, 1, 0}};
    for (const auto &u : units) {
        auto c = random_seq();
        for (int at : {100, 300, 500}) {
            const int len = 20 + (int)(rng() % 180);
            for (int j = 0; j < len; ++j) c[at + j] = u[j % u.size()];
        }
        seqs.push_back(c);
    }
    for (int i = 0; i < 30; ++i) {
        auto c = random_seq();
        for (int r = 0; r < 6; ++r) {
            const int at = (int)(rng() % 690), len = 1 + (int)(rng() % 11);
            for (int j = 0; j < len && at + j < 700; ++j) c[at + j] = 4;
        }
        seqs.push_back(c);
    }
    for (int warm : {0, 5, 8, 9, 10, 14, 15, 24, 25, 98}) {
        int bad = 0, total = 0;
        for (const auto &c : seqs)
            for (int64_t s0 = 1; s0 < 650; s0 += 7) {
                const int64_t from = s0 > warm ? s0 - warm : 0;
                ++total;
                bad += sketch_from(c, 0, s0) != sketch_from(c, from, s0);
            }
        std::printf("warm %2d: %d of %d chunk starts differ\n", warm, bad, total);
    }
    return 0;
}
