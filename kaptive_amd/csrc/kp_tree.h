// kp_tree.h -- the minimum spanning forest of locus rows (kp_spec.h, TREE), written once as plain functions: the packed edge key, the
// predicate for a matrix that fits it, the bound on Boruvka's rounds, and a serial host
// Boruvka over a matrix of blocks.  The tree kernels of kp_dist_graph.hip and their host share them.  No HIP header:
// tests/native_harness compiles it with g++.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "kp_caps.h"
#include "kp_clust.h"

// PACKED KEY of the edge (a, b), a < b, at `differences`: a smaller key is a lighter edge -- fewer differences, then the smaller a,
// then the smaller b.  Strictly ordered as the tuple, because every field stays inside its bits (kp_tree_fits; rows < 2^18).
#define KP_TREE_KEY_NONE KP_DIST_KEY_NONE /* no edge: loses to every key (a < b keeps a at 2^18 - 2 or less: no key is all ones) */
KP_HD uint64_t kp_tree_key(int32_t differences, int32_t a, int32_t b) {
    return ((uint64_t)(uint32_t)differences << (2 * KP_TREE_ROW_BITS)) | ((uint64_t)(uint32_t)a << KP_TREE_ROW_BITS) | (uint64_t)(uint32_t)b;
}
KP_HD int32_t kp_tree_key_differences(uint64_t key) { return (int32_t)(key >> (2 * KP_TREE_ROW_BITS)); }
KP_HD int32_t kp_tree_key_a(uint64_t key) { return (int32_t)((key >> KP_TREE_ROW_BITS) & ((1u << KP_TREE_ROW_BITS) - 1u)); }
KP_HD int32_t kp_tree_key_b(uint64_t key) { return (int32_t)(key & ((1u << KP_TREE_ROW_BITS) - 1u)); }

// A matrix of n_blocks blocks a row fits the key: no pair can differ in 2^28 columns or more.
KP_HD bool kp_tree_fits(int64_t n_blocks) { return n_blocks >= 0 && 16 * n_blocks < KP_TREE_MAX_COLUMNS; }

// ROUNDS.  Every round of Boruvka hooks each component that has an edge to another one, so the components that still have one at
// least halve: after ceil(log2 n) rounds none is left, and one more round finds no edge and ends the loop.
KP_HD int32_t kp_tree_max_rounds(int64_t n_rows) {
    const int64_t n = n_rows < 2 ? 2 : n_rows;
    int32_t lg = 0;
    while (((int64_t)1 << lg) < n) ++lg;
    return lg + 1;
}
// (the union that names the root it moved, under the name the harness sources know: kp_clust.h has the loop)
KP_HD int32_t kp_tree_unite(int32_t *parent, int32_t a, int32_t b) { return kp_clust_unite_root(parent, a, b); }

// The forest of a matrix of blocks, serially, by the rounds the device runs: every component's lightest outgoing edge under the
// packed key, then one union per chosen edge.  edges [max(R - 1, 0)] ascend by key, component [R] is the smallest row of every
// row's tree.  Returns the number of edges, or -1 when the round bound was reached with edges still arriving.  `rounds`, if given,
// receives the rounds taken, the empty last one included.
inline int64_t kp_tree_host(const uint64_t *blocks, int32_t R, int64_t nb, int32_t min_compared, kp_dist_pair *edges, int32_t *component, int32_t *rounds = nullptr) {
    if (rounds) *rounds = 0;
    if (R <= 0) return 0;
    const auto counts = [&](int32_t a, int32_t b) { return kp_dist_row_counts(blocks + (size_t)a * (size_t)nb, blocks + (size_t)b * (size_t)nb, nb); };
    std::vector<int32_t> parent((size_t)R), label((size_t)R);
    for (int32_t r = 0; r < R; ++r) parent[r] = label[r] = r;
    std::vector<uint64_t> cbest((size_t)R), chosen;
    bool ended = false;
    for (int32_t round = 0; round < kp_tree_max_rounds(R) && !ended; ++round) {
        std::fill(cbest.begin(), cbest.end(), KP_TREE_KEY_NONE);
        for (int32_t a = 0; a < R; ++a)
            for (int32_t b = a + 1; b < R; ++b) {
                if (label[a] == label[b]) continue;
                const KpDistCounts c = counts(a, b);
                if (c.compared < min_compared) continue;
                const uint64_t k = kp_tree_key(c.differences, a, b);
                cbest[label[a]] = std::min(cbest[label[a]], k);
                cbest[label[b]] = std::min(cbest[label[b]], k);
            }
        int64_t fresh = 0;
        for (int32_t r = 0; r < R; ++r)
            if (label[r] == r && cbest[r] != KP_TREE_KEY_NONE && kp_clust_unite(parent.data(), kp_tree_key_a(cbest[r]), kp_tree_key_b(cbest[r]))) {
                chosen.push_back(cbest[r]);
                ++fresh;
            }
        for (int32_t r = 0; r < R; ++r) label[r] = kp_clust_find(parent.data(), r);
        if (rounds) *rounds = round + 1;
        ended = fresh == 0;
    }
    if (!ended) return -1;
    std::sort(chosen.begin(), chosen.end());
    for (size_t e = 0; e < chosen.size(); ++e) {
        const KpDistCounts c = counts(kp_tree_key_a(chosen[e]), kp_tree_key_b(chosen[e]));
        kp_dist_pair_store(edges + e, kp_tree_key_a(chosen[e]), kp_tree_key_b(chosen[e]), c.compared, c.differences, c.unshared);
    }
    for (int32_t r = 0; r < R; ++r) component[r] = label[r];
    return (int64_t)chosen.size();
}
