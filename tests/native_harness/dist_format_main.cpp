// dist_format_main.cpp -- a stand-alone program around kaptive_amd/csrc/kp_dist.h and kp_format_distances, for a run under the host
// sanitizers (no GPU, nothing loaded into an interpreter):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -o dist_format_main
//       tests/native_harness/dist_format_main.cpp kaptive_amd/csrc/kp_rows.cpp && ./dist_format_main
// Every table is a heap block of exactly the size the call may read or write: an access past an end stops the program.  It makes
// locus rows of 1 to 70 blocks -- short last plane words included -- from random codes, compares the counts of every pair, summed
// plane word by plane word, with a walk column by column; checks the padding mask of every length and the tile of every index of
// small grids and of the grids of 4097, 16385 and 2^18 rows; then formats a table twice (sizing call with cap 0, then into a buffer of exactly the size returned) and checks
// every refusal.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kaptive_amd.h"
#include "../../kaptive_amd/csrc/kp_dist.h"

template <class T>
struct Exact {  // a heap block of exactly n items (std::vector may round its capacity up)
    T *p;
    size_t n;
    explicit Exact(const std::vector<T> &v) : p((T *)std::malloc(v.size() * sizeof(T) + (v.empty() ? 1 : 0))), n(v.size()) {
        if (!v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T));
    }
    ~Exact() { std::free(p); }
    Exact(const Exact &) = delete;
};

static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #x); ++fails; } } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) {  // xorshift64*: [0, n)
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)(((rng_state * 0x2545f4914f6cdd1dull) >> 33) % n);
}

// codes 0..3, 4 = N, 5 = GAP -> blocks
static std::vector<uint64_t> pack(const std::vector<uint8_t> &codes) {
    std::vector<uint64_t> b(codes.size() / 16, 0);
    for (size_t c = 0; c < codes.size(); ++c) {
        const int j = (int)(c & 15);
        if (codes[c] < 4) b[c / 16] |= (uint64_t)codes[c] << (2 * j);
        else if (codes[c] == 4) b[c / 16] |= 1ull << (32 + j);
        else b[c / 16] |= 1ull << (48 + j);
    }
    return b;
}

static void counts_case(int nb) {
    std::vector<uint8_t> ca((size_t)16 * nb), cb((size_t)16 * nb);
    for (auto *v : {&ca, &cb})
        for (auto &c : *v) { const uint32_t r = rnd(20); c = r < 16 ? (uint8_t)(r & 3) : (r < 17 ? 4 : 5); }
    const Exact<uint64_t> a(pack(ca)), b(pack(cb));
    int32_t got[3] = {0, 0, 0}, want[3] = {0, 0, 0};
    for (int64_t w = 0; w < kp_dist_words(nb); ++w) {
        const KpDistWord x = kp_dist_word_planes(a.p, nb, w), y = kp_dist_word_planes(b.p, nb, w);
        kp_dist_word_counts(x.lo, x.hi, x.valid, x.present, y.lo, y.hi, y.valid, y.present, &got[0], &got[1], &got[2]);
    }
    for (size_t c = 0; c < ca.size(); ++c) {
        if (ca[c] < 4 && cb[c] < 4) { ++want[0]; want[1] += ca[c] != cb[c]; }
        want[2] += (ca[c] == 5) != (cb[c] == 5);
    }
    CHECK(got[0] == want[0] && got[1] == want[1] && got[2] == want[2]);
}

int main() {
    for (int nb = 1; nb <= 70; ++nb)
        for (int rep = 0; rep < 4; ++rep) counts_case(nb);
    for (int L = 1; L <= 200; ++L) {
        uint64_t want = 0;
        for (int c = L % 16; L % 16 && c < 16; ++c) want |= 1ull << (48 + c);
        CHECK(kp_dist_pad_mask(L) == want);
    }
    CHECK(kp_dist_pad_mask(65535) == 0x8000ull << 48 && kp_dist_pad_mask(65536) == 0);
    CHECK(kp_dist_listed(5, 3, 3, 5) && !kp_dist_listed(5, 4, 3, 5) && !kp_dist_listed(4, 3, 3, 5) && kp_dist_listed(0, 0, 0x7fffffff, 0));
    for (int nt = 1; nt <= 40; ++nt) {
        int64_t t = 0;
        for (int i = 0; i < nt; ++i)
            for (int j = i; j < nt; ++j, ++t) {
                int32_t ti, tj;
                kp_dist_tile_of(t, nt, &ti, &tj);
                CHECK(ti == i && tj == j);
            }
        CHECK(t == kp_dist_tiles(nt));
    }
    // every tile of the grids of 4097 rows, of 16385 rows and of KP_DIST_MAX_ROWS rows (8 390 656 tiles: the square root of
    // kp_dist_tile_of at its largest argument) against two nested counters
    for (const int64_t nt : {(int64_t)65, (int64_t)257, (int64_t)4096}) {
        int64_t t = 0, wrong = 0;
        for (int64_t i = 0; i < nt; ++i) {
            CHECK(kp_dist_tile_row_first(i, nt) == t);
            for (int64_t j = i; j < nt; ++j, ++t) {
                int32_t ti = -1, tj = -1;
                kp_dist_tile_of(t, nt, &ti, &tj);
                wrong += !(ti == i && tj == j);
            }
        }
        CHECK(wrong == 0);
        CHECK(t == kp_dist_tiles(nt));
        std::printf("tiles of nt %lld: %lld walked\n", (long long)nt, (long long)t);
    }
    {   // the known answers of the specification
        const Exact<uint64_t> a({0xf0c3010000900e40ull, 0x000f000000000000ull | kp_dist_pad_mask(20)}), b({0xf0c3002000e40390ull, 0x000f000000000000ull | kp_dist_pad_mask(20)});
        const Exact<uint64_t> g({0xffffull << 48, 0xffffull << 48});
        CHECK(a.p[1] >> 48 == 0xffff);
        int32_t c[3] = {0, 0, 0};
        KpDistWord x = kp_dist_word_planes(a.p, 2, 0), y = kp_dist_word_planes(b.p, 2, 0), z = kp_dist_word_planes(g.p, 2, 0);
        kp_dist_word_counts(x.lo, x.hi, x.valid, x.present, y.lo, y.hi, y.valid, y.present, &c[0], &c[1], &c[2]);
        CHECK(c[0] == 6 && c[1] == 6 && c[2] == 0);
        c[0] = c[1] = c[2] = 0;
        kp_dist_word_counts(x.lo, x.hi, x.valid, x.present, z.lo, z.hi, z.valid, z.present, &c[0], &c[1], &c[2]);
        CHECK(c[0] == 0 && c[1] == 0 && c[2] == 8);
        kp_dist_pair rec;
        kp_dist_pair_store(&rec, 1, 2, 3, 4, 5);
        CHECK(rec.a == 1 && rec.b == 2 && rec.compared == 3 && rec.differences == 4 && rec.unshared == 5 && rec.pad_ == 0);
    }
    {   // the formatter: size, then fill exactly
        const std::string names_s = "iso_1" "b" "" "a third name";
        const Exact<char> names(std::vector<char>(names_s.begin(), names_s.end()));
        const Exact<int64_t> off({0, 5, 6, 6, 18});
        const Exact<kp_dist_pair> pairs({{0, 1, 25000, 3, 17, 0}, {0, 3, 2147483647, 2147483647, 2147483647, 0}, {2, 3, 0, 0, 0, 0}});
        const Exact<char> locus(std::vector<char>{'K', 'L', '1'});
        const std::string want = "KL1\tiso_1\tb\t25123\t25000\t3\t17\nKL1\tiso_1\ta third name\t25123\t2147483647\t2147483647\t2147483647\nKL1\t\ta third name\t25123\t0\t0\t0\n";
        const int64_t need = kp_format_distances(locus.p, 3, 25123, names.p, off.p, 4, pairs.p, 3, nullptr, 0);
        CHECK(need == (int64_t)want.size());
        const Exact<char> out(std::vector<char>((size_t)need, '?'));
        CHECK(kp_format_distances(locus.p, 3, 25123, names.p, off.p, 4, pairs.p, 3, out.p, need) == need);
        CHECK(std::memcmp(out.p, want.data(), want.size()) == 0);
        const Exact<char> small(std::vector<char>(10, '?'));  // too small: counted, nothing stored past its end
        CHECK(kp_format_distances(locus.p, 3, 25123, names.p, off.p, 4, pairs.p, 3, small.p, 10) == need);
        CHECK(kp_format_distances(locus.p, 3, 25123, names.p, off.p, 4, pairs.p, 0, nullptr, 0) == 0);
        CHECK(kp_format_distances(nullptr, 0, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, 0) == 0);
        CHECK(kp_format_distances(locus.p, 3, 25123, names.p, off.p, 3, pairs.p, 3, nullptr, 0) == KP_EINVAL);  // a pair names row 3 of 3
        CHECK(kp_format_distances(locus.p, 3, 25123, names.p, nullptr, 4, pairs.p, 3, nullptr, 0) == KP_EINVAL);
        CHECK(kp_format_distances(locus.p, 3, 25123, names.p, off.p, 4, nullptr, 3, nullptr, 0) == KP_EINVAL);
        CHECK(kp_format_distances(locus.p, 3, 25123, names.p, off.p, 4, pairs.p, 3, nullptr, 5) == KP_EINVAL);
        CHECK(kp_format_distances(locus.p, -1, 25123, names.p, off.p, 4, pairs.p, 3, nullptr, 0) == KP_EINVAL);
        CHECK(kp_format_distances(locus.p, 3, -1, names.p, off.p, 4, pairs.p, 3, nullptr, 0) == KP_EINVAL);
        const Exact<kp_dist_pair> neg({{-1, 1, 0, 0, 0, 0}});
        CHECK(kp_format_distances(locus.p, 3, 1, names.p, off.p, 4, neg.p, 1, nullptr, 0) == KP_EINVAL);
    }
    std::printf(fails ? "FAILED: %d checks\n" : "dist_format_main: all checks passed\n", fails);
    return fails ? 1 : 0;
}
