// clust_harness.cpp -- test infrastructure for tests/test_clusters_cpu.py (g++, no GPU): the functions of kaptive_amd/csrc/kp_clust.h --
// the ones the cluster kernel calls, in their host bodies -- on host arrays.
//   * kpy_clust_layout: the record's size and the constants the Python side mirrors.
//   * kpy_clust_levels_valid, kpy_clust_first_level: the level list's rule and the first level of a pair.
//   * kpy_clust_key, kpy_clust_key_none, kpy_clust_key_row, kpy_clust_key_differences: the nearest key.
//   * kpy_clust_labels: an edge list united in the order given; parent[x] <= x checked after every call.
//   * kpy_clust_numbers: the cluster numbers of one level's labels.
//   * kpy_clust_matrix: labels and nearest records of a matrix of blocks, pair by pair as a lane of the kernel meets them.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../kaptive_amd/csrc/kp_caps.h"
#include "../../kaptive_amd/csrc/kp_clust.h"

static KpClustLevels levels_of(const int32_t *levels, int32_t n) {
    KpClustLevels L{};
    for (int32_t k = 0; k < KP_CLUST_MAX_LEVELS; ++k) L.t[k] = k < n ? levels[k] : INT32_MAX;
    L.n = n;
    return L;
}

extern "C" {

void kpy_clust_layout(int32_t *out4) {
    out4[0] = (int32_t)sizeof(kp_dist_nearest); out4[1] = KP_CLUST_MAX_LEVELS; out4[2] = (int32_t)sizeof(KpClustLevels); out4[3] = KP_CLUST_HALVE;
}

int kpy_clust_levels_valid(const int32_t *levels, int32_t n) { return kp_clust_levels_valid(levels, n) ? 1 : 0; }
int32_t kpy_clust_first_level(const int32_t *levels, int32_t n, int32_t differences) { return kp_clust_first_level(levels_of(levels, n), differences); }

uint64_t kpy_clust_key(int32_t differences, int32_t s) { return kp_clust_key(differences, s); }
uint64_t kpy_clust_key_none(void) { return KP_CLUST_KEY_NONE; }
int32_t kpy_clust_key_row(uint64_t key) { return kp_clust_key_row(key); }
int32_t kpy_clust_key_differences(uint64_t key) { return kp_clust_key_differences(key); }

// edges [n][3]: a, b, differences.  out [K][R].  -1 when parent[x] <= x broke after some call (checked only on request: it costs R a call).
int kpy_clust_labels(int32_t R, const int32_t *edges, int64_t n, const int32_t *levels, int32_t K, int32_t check, int32_t *out) {
    const KpClustLevels L = levels_of(levels, K);
    std::vector<int32_t> parent((size_t)K * (size_t)R);
    for (size_t e = 0; e < parent.size(); ++e) parent[e] = (int32_t)(e % (size_t)R);
    const auto ok = [&]() {
        for (int32_t k = 0; k < K; ++k)
            for (int32_t x = 0; x < R; ++x)
                if (parent[(size_t)k * R + x] < 0 || parent[(size_t)k * R + x] > x) return false;
        return true;
    };
    for (int64_t i = 0; i < n; ++i) {
        kp_clust_edge(parent.data(), R, K, kp_clust_first_level(L, edges[3 * i + 2]), edges[3 * i], edges[3 * i + 1]);
        if (check && !ok()) return -1;
    }
    for (int32_t k = 0; k < K; ++k)
        for (int32_t x = 0; x < R; ++x) {
            out[(size_t)k * R + x] = kp_clust_find(parent.data() + (size_t)k * R, x);
            if (check && !ok()) return -1;
        }
    return 0;
}

int kpy_clust_numbers(const int32_t *label, int32_t R, int32_t *number) {
    std::vector<int32_t> rank((size_t)R);
    return kp_clust_numbers(label, R, rank.data(), number) ? 1 : 0;
}

int kpy_clust_matrix(const uint64_t *blocks, int32_t R, int64_t nb, const int32_t *levels, int32_t K, int32_t min_compared, int32_t *labels, kp_dist_nearest *nearest) {
    const KpClustLevels L = levels_of(levels, K);
    std::vector<int32_t> parent((size_t)K * (size_t)R);
    for (size_t e = 0; e < parent.size(); ++e) parent[e] = (int32_t)(e % (size_t)R);
    std::vector<uint64_t> best((size_t)R, KP_CLUST_KEY_NONE);
    const auto counts = [&](int32_t a, int32_t b) { return kp_dist_row_counts(blocks + (size_t)a * nb, blocks + (size_t)b * nb, nb); };
    for (int32_t a = 0; a < R; ++a)
        for (int32_t b = a + 1; b < R; ++b) {
            const KpDistCounts c = counts(a, b);
            if (c.compared < min_compared) continue;
            if (kp_clust_key(c.differences, b) < best[a]) best[a] = kp_clust_key(c.differences, b);
            if (kp_clust_key(c.differences, a) < best[b]) best[b] = kp_clust_key(c.differences, a);
            kp_clust_edge(parent.data(), R, K, kp_clust_first_level(L, c.differences), a, b);
        }
    for (int32_t k = 0; k < K; ++k)
        for (int32_t x = 0; x < R; ++x) labels[(size_t)k * R + x] = kp_clust_find(parent.data() + (size_t)k * R, x);
    for (int32_t r = 0; r < R; ++r) {
        const int32_t s = kp_clust_key_row(best[r]);
        KpDistCounts c{0, 0, 0};
        if (s >= 0) c = counts(r, s);
        if (s >= 0 && c.differences != kp_clust_key_differences(best[r])) return -1;
        kp_dist_nearest_store(nearest + r, s, c.compared, c.differences, c.unshared);
    }
    return 0;
}

}  // extern "C"
