// clust_format_main.cpp -- a stand-alone program around kaptive_amd/csrc/kp_clust.h and kp_format_clusters, for a run under the host
// sanitizers (no GPU, nothing loaded into an interpreter):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -o clust_format_main
//       tests/native_harness/clust_format_main.cpp kaptive_amd/csrc/kp_rows.cpp && ./clust_format_main
// Every table is a heap block of exactly the size the call may read or write: an access past an end stops the program.  It checks
// the first level of a pair at every edge of a level list, the nearest key's order, find / unite on random edge lists in three
// orders against a flood fill (parent[x] <= x after every call), the cluster numbers, the specification's known answers, and the
// formatter: sized with cap 0, filled into a buffer of exactly the size returned, K = 0, 1 and 8, a row without a neighbour, and
// every refusal.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kaptive_amd.h"
#include "../../kaptive_amd/csrc/kp_clust.h"

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

static KpClustLevels levels_of(const std::vector<int32_t> &t) {
    KpClustLevels L{};
    for (int k = 0; k < KP_CLUST_MAX_LEVELS; ++k) L.t[k] = k < (int)t.size() ? t[k] : INT32_MAX;
    L.n = (int32_t)t.size();
    return L;
}

struct Edge { int32_t a, b, d; };

// the labels of R rows under `edges`, united in the order given; parent[x] <= x after every call
static std::vector<int32_t> labels_of(int32_t R, const std::vector<Edge> &edges, const std::vector<int32_t> &t) {
    const KpClustLevels L = levels_of(t);
    const int32_t K = L.n;
    std::vector<int32_t> seed((size_t)K * R);
    for (size_t e = 0; e < seed.size(); ++e) seed[e] = (int32_t)(e % (size_t)R);
    const Exact<int32_t> parent(seed);
    const auto ok = [&]() {
        for (size_t e = 0; e < parent.n; ++e)
            if (parent.p[e] < 0 || parent.p[e] > (int32_t)(e % (size_t)R)) return false;
        return true;
    };
    for (const Edge &e : edges) {
        kp_clust_edge(parent.p, R, K, kp_clust_first_level(L, e.d), e.a, e.b);
        CHECK(ok());
    }
    std::vector<int32_t> out((size_t)K * R);
    for (int32_t k = 0; k < K; ++k)
        for (int32_t x = 0; x < R; ++x) out[(size_t)k * R + x] = kp_clust_find(parent.p + (size_t)k * R, x);
    CHECK(ok());
    return out;
}

// the same by flood fill: label = the smallest row reachable over edges of at most t[k] differences
static std::vector<int32_t> flood(int32_t R, const std::vector<Edge> &edges, const std::vector<int32_t> &t) {
    std::vector<int32_t> out(t.size() * (size_t)R);
    for (size_t k = 0; k < t.size(); ++k) {
        int32_t *lab = out.data() + k * (size_t)R;
        for (int32_t x = 0; x < R; ++x) lab[x] = x;
        for (bool moved = true; moved;) {
            moved = false;
            for (const Edge &e : edges)
                if (e.d <= t[k] && lab[e.a] != lab[e.b]) { lab[e.a] = lab[e.b] = std::min(lab[e.a], lab[e.b]); moved = true; }
        }
    }
    return out;
}

int main() {
    {   // the first level of a pair, at every edge
        const std::vector<int32_t> t{0, 1, 2, 5, 10};
        const KpClustLevels L = levels_of(t);
        for (int k = 0; k < 5; ++k) {
            CHECK(kp_clust_first_level(L, t[k]) == k);
            CHECK(kp_clust_first_level(L, t[k] + 1) == k + 1);
        }
        CHECK(kp_clust_first_level(L, 3) == 3 && kp_clust_first_level(L, 11) == 5 && kp_clust_first_level(L, INT32_MAX) == 5);
        CHECK(kp_clust_first_level(levels_of({}), 0) == 0 && kp_clust_first_level(levels_of({}), INT32_MAX) == 0);
        const KpClustLevels top = levels_of({0, 1, 2, 3, 4, 5, 6, INT32_MAX});
        CHECK(kp_clust_first_level(top, INT32_MAX) == 7 && kp_clust_first_level(top, 7) == 7 && kp_clust_first_level(top, 6) == 6);
        const Exact<int32_t> good({0, 1, 2, 5, 10}), same({0, 1, 1}), down({3, 2}), neg({-1, 0}), nine({0, 1, 2, 3, 4, 5, 6, 7, 8});
        CHECK(kp_clust_levels_valid(good.p, 5) && kp_clust_levels_valid(nullptr, 0) && kp_clust_levels_valid(nine.p, 8));
        CHECK(!kp_clust_levels_valid(same.p, 3) && !kp_clust_levels_valid(down.p, 2) && !kp_clust_levels_valid(neg.p, 2));
        CHECK(!kp_clust_levels_valid(nine.p, 9) && !kp_clust_levels_valid(nullptr, 1) && !kp_clust_levels_valid(good.p, -1));
    }
    {   // the nearest key
        CHECK(kp_clust_key(0, 5) < kp_clust_key(1, 0) && kp_clust_key(3, 4) < kp_clust_key(3, 5) && kp_clust_key(INT32_MAX, (1 << 18) - 1) < KP_CLUST_KEY_NONE);
        CHECK(kp_clust_key_row(kp_clust_key(7, 9)) == 9 && kp_clust_key_differences(kp_clust_key(7, 9)) == 7);
        CHECK(kp_clust_key_row(KP_CLUST_KEY_NONE) == -1 && kp_clust_key_differences(KP_CLUST_KEY_NONE) == 0);
        CHECK(kp_clust_key_differences(kp_clust_key(INT32_MAX, 0)) == INT32_MAX);
    }
    for (int rep = 0; rep < 40; ++rep) {  // find / unite: random edge lists, three orders, against a flood fill
        const int32_t R = 1 + (int32_t)rnd(90);
        std::vector<Edge> edges;
        for (uint32_t i = 0, n = rnd(3 * R); i < n && R > 1; ++i) {
            const int32_t a = (int32_t)rnd(R), b = (int32_t)rnd(R);
            if (a != b) edges.push_back({std::min(a, b), std::max(a, b), (int32_t)rnd(8)});
        }
        const std::vector<int32_t> t{0, 2, 3, 6};
        const std::vector<int32_t> want = flood(R, edges, t);
        CHECK(labels_of(R, edges, t) == want);
        std::vector<Edge> back(edges.rbegin(), edges.rend()), mixed(edges);
        for (size_t i = mixed.size(); i > 1; --i) std::swap(mixed[i - 1], mixed[rnd((uint32_t)i)]);
        CHECK(labels_of(R, back, t) == want && labels_of(R, mixed, t) == want);
        for (size_t k = 0; k < t.size(); ++k) {  // the cluster numbers: ranks of the roots
            const std::vector<int32_t> level(want.begin() + k * R, want.begin() + (k + 1) * R), room((size_t)R, 0);
            const Exact<int32_t> lab(level), rank(room), num(room);
            CHECK(kp_clust_numbers(lab.p, R, rank.p, num.p));
            int32_t roots = 0;
            for (int32_t x = 0; x < R; ++x) {
                if (lab.p[x] == x) ++roots;
                CHECK(num.p[x] == num.p[lab.p[x]] && (lab.p[x] != x || num.p[x] == roots));
            }
        }
    }
    {   // a chain hooked from its far end: the deepest tree the rule can make, then found from the bottom
        const int32_t R = 300;
        std::vector<Edge> chain;
        for (int32_t x = R - 1; x > 0; --x) chain.push_back({x - 1, x, 1});
        const std::vector<int32_t> got = labels_of(R, chain, {0, 1});
        for (int32_t x = 0; x < R; ++x) CHECK(got[x] == x && got[R + x] == 0);
    }
    {   // the known answers of the specification: rows A, B and the all-GAP row, levels (0, 6)
        const Exact<uint64_t> m({0xf0c3010000900e40ull, 0x000f000000000000ull | kp_dist_pad_mask(20), 0xf0c3002000e40390ull, 0x000f000000000000ull | kp_dist_pad_mask(20),
                                 0xffffull << 48, 0xffffull << 48});
        for (int32_t mc = 0; mc <= 1; ++mc) {
            const KpClustLevels L = levels_of({0, 6});
            const Exact<int32_t> parent({0, 1, 2, 0, 1, 2});
            uint64_t best[3] = {KP_CLUST_KEY_NONE, KP_CLUST_KEY_NONE, KP_CLUST_KEY_NONE};
            int32_t cnt[3][3][3] = {};
            for (int32_t a = 0; a < 3; ++a)
                for (int32_t b = a + 1; b < 3; ++b) {
                    int32_t *c = cnt[a][b];
                    const KpDistWord x = kp_dist_word_planes(m.p + 2 * a, 2, 0), y = kp_dist_word_planes(m.p + 2 * b, 2, 0);
                    kp_dist_word_counts(x.lo, x.hi, x.valid, x.present, y.lo, y.hi, y.valid, y.present, &c[0], &c[1], &c[2]);
                    if (c[0] < mc) continue;
                    best[a] = std::min(best[a], kp_clust_key(c[1], b));
                    best[b] = std::min(best[b], kp_clust_key(c[1], a));
                    kp_clust_edge(parent.p, 3, 2, kp_clust_first_level(L, c[1]), a, b);
                }
            int32_t lab[6];
            for (int k = 0; k < 2; ++k)
                for (int x = 0; x < 3; ++x) lab[3 * k + x] = kp_clust_find(parent.p + 3 * k, x);
            if (mc == 1) {
                CHECK(lab[0] == 0 && lab[1] == 1 && lab[2] == 2 && lab[3] == 0 && lab[4] == 0 && lab[5] == 2);
                CHECK(kp_clust_key_row(best[0]) == 1 && kp_clust_key_row(best[1]) == 0 && kp_clust_key_row(best[2]) == -1);
                CHECK(cnt[0][1][0] == 6 && cnt[0][1][1] == 6 && cnt[0][1][2] == 0);
            } else {
                for (int e = 0; e < 6; ++e) CHECK(lab[e] == 0);
                CHECK(kp_clust_key_row(best[0]) == 2 && kp_clust_key_row(best[1]) == 2 && kp_clust_key_row(best[2]) == 0);
                CHECK(cnt[0][2][0] == 0 && cnt[0][2][1] == 0 && cnt[0][2][2] == 8 && cnt[1][2][2] == 8);
            }
        }
        kp_dist_nearest rec;
        kp_dist_nearest_store(&rec, 1, 2, 3, 4);
        CHECK(rec.row == 1 && rec.compared == 2 && rec.differences == 3 && rec.unshared == 4);
    }
    {   // the formatter: size, then fill exactly
        const std::string names_s = "iso_1" "b" "" "a third name";
        const Exact<char> names(std::vector<char>(names_s.begin(), names_s.end()));
        const Exact<int64_t> off({0, 5, 6, 6, 18});
        const Exact<int32_t> labels({0, 1, 2, 3, 0, 0, 2, 2});  // two levels of four rows
        const Exact<kp_dist_nearest> near({{1, 25000, 3, 17}, {0, 25000, 3, 17}, {3, 2147483647, 2147483647, 2147483647}, {-1, 0, 0, 0}});
        const Exact<char> locus(std::vector<char>{'K', 'L', '1'});
        const std::string want = "KL1\tiso_1\t1\t1\tb\t3\t25000\t17\nKL1\tb\t2\t1\tiso_1\t3\t25000\t17\n"
                                 "KL1\t\t3\t2\ta third name\t2147483647\t2147483647\t2147483647\nKL1\ta third name\t4\t2\t.\t.\t.\t.\n";
        const int64_t need = kp_format_clusters(locus.p, 3, names.p, off.p, 4, nullptr, 2, labels.p, near.p, nullptr, 0);
        CHECK(need == (int64_t)want.size());
        const Exact<char> out(std::vector<char>((size_t)std::max<int64_t>(need, 1), '?'));
        CHECK(kp_format_clusters(locus.p, 3, names.p, off.p, 4, nullptr, 2, labels.p, near.p, out.p, need) == need);
        CHECK(need == (int64_t)want.size() && std::memcmp(out.p, want.data(), want.size()) == 0);
        const Exact<char> small(std::vector<char>(10, '?'));  // too small: counted, nothing stored past its end
        CHECK(kp_format_clusters(locus.p, 3, names.p, off.p, 4, nullptr, 2, labels.p, near.p, small.p, 10) == need);
        const Exact<int32_t> ident({0, 1, 2, 3}), swapped({1, 0, 2, 3});
        CHECK(kp_format_clusters(locus.p, 3, names.p, off.p, 4, ident.p, 2, labels.p, near.p, out.p, need) == need && std::memcmp(out.p, want.data(), want.size()) == 0);
        CHECK(kp_format_clusters(locus.p, 3, names.p, off.p, 4, swapped.p, 2, labels.p, near.p, out.p, need) == need && std::memcmp(out.p, "KL1\tb\t1\t1\tiso_1\t", 16) == 0);
        // K = 0: no cluster column; K = 8
        const std::string want0 = "KL1\tiso_1\tb\t3\t25000\t17\nKL1\tb\tiso_1\t3\t25000\t17\nKL1\t\ta third name\t2147483647\t2147483647\t2147483647\nKL1\ta third name\t.\t.\t.\t.\n";
        CHECK(kp_format_clusters(locus.p, 3, names.p, off.p, 4, nullptr, 0, nullptr, near.p, nullptr, 0) == (int64_t)want0.size());
        const Exact<int32_t> eight(std::vector<int32_t>(32, 0));
        const Exact<kp_dist_nearest> nobody({{-1, 0, 0, 0}, {-1, 0, 0, 0}, {-1, 0, 0, 0}, {-1, 0, 0, 0}});
        CHECK(kp_format_clusters(nullptr, 0, names.p, off.p, 4, nullptr, 8, eight.p, nobody.p, nullptr, 0) == (int64_t)(4 * (1 + 16 + 8) + 18 + 4));
        CHECK(kp_format_clusters(nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, 0) == 0);
        // refusals
        CHECK(kp_format_clusters(locus.p, 3, names.p, off.p, 4, nullptr, 9, labels.p, near.p, nullptr, 0) == KP_EINVAL);
        CHECK(kp_format_clusters(locus.p, 3, names.p, off.p, 4, nullptr, -1, labels.p, near.p, nullptr, 0) == KP_EINVAL);
        CHECK(kp_format_clusters(locus.p, -1, names.p, off.p, 4, nullptr, 2, labels.p, near.p, nullptr, 0) == KP_EINVAL);
        CHECK(kp_format_clusters(nullptr, 3, names.p, off.p, 4, nullptr, 2, labels.p, near.p, nullptr, 0) == KP_EINVAL);
        CHECK(kp_format_clusters(locus.p, 3, names.p, nullptr, 4, nullptr, 2, labels.p, near.p, nullptr, 0) == KP_EINVAL);
        CHECK(kp_format_clusters(locus.p, 3, names.p, off.p, 4, nullptr, 2, nullptr, near.p, nullptr, 0) == KP_EINVAL);
        CHECK(kp_format_clusters(locus.p, 3, names.p, off.p, 4, nullptr, 2, labels.p, nullptr, nullptr, 0) == KP_EINVAL);
        CHECK(kp_format_clusters(locus.p, 3, names.p, off.p, 4, nullptr, 2, labels.p, near.p, nullptr, 5) == KP_EINVAL);
        CHECK(kp_format_clusters(locus.p, 3, names.p, off.p, -1, nullptr, 2, labels.p, near.p, nullptr, 0) == KP_EINVAL);
        const Exact<int32_t> above({0, 2, 2, 3, 0, 0, 2, 2}), outside({0, 1, 2, 4, 0, 0, 2, 2}), negative({0, -1, 2, 3, 0, 0, 2, 2}), no_root({0, 1, 1, 2, 0, 0, 2, 2});
        for (const Exact<int32_t> *bad : {&above, &outside, &negative, &no_root})  // a label above its row, outside the table, negative, not a root
            CHECK(kp_format_clusters(locus.p, 3, names.p, off.p, 4, nullptr, 2, bad->p, near.p, nullptr, 0) == KP_EINVAL);
        const Exact<kp_dist_nearest> far({{4, 1, 1, 1}, {0, 1, 1, 1}, {0, 1, 1, 1}, {0, 1, 1, 1}}), low({{-2, 1, 1, 1}, {0, 1, 1, 1}, {0, 1, 1, 1}, {0, 1, 1, 1}});
        CHECK(kp_format_clusters(locus.p, 3, names.p, off.p, 4, nullptr, 2, labels.p, far.p, nullptr, 0) == KP_EINVAL);
        CHECK(kp_format_clusters(locus.p, 3, names.p, off.p, 4, nullptr, 2, labels.p, low.p, nullptr, 0) == KP_EINVAL);
        const Exact<int32_t> bad_rows({0, 1, 2, 4});
        CHECK(kp_format_clusters(locus.p, 3, names.p, off.p, 4, bad_rows.p, 2, labels.p, near.p, nullptr, 0) == KP_EINVAL);
    }
    std::printf(fails ? "FAILED: %d checks\n" : "clust_format_main: all checks passed\n", fails);
    return fails ? 1 : 0;
}
