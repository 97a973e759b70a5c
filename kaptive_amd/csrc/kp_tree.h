// kp_tree.h -- the minimum spanning forest of locus rows (kp_spec.h, TREE), written once as plain functions: the packed edge key, the
// predicate for a matrix that fits it, the bound on Boruvka's rounds, the union that names the root it moved, and a serial host
// Boruvka over a matrix of blocks.  The tree kernels of kp_dist.hip and their host share them.  No HIP header:
// tests/native_harness compiles it with g++.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "kp_caps.h"
#include "kp_clust.h"

// PACKED KEY of the edge (a, b), a < b, at `differences`: a smaller key is a lighter edge -- fewer differences, then the smaller a,
// then the smaller b.  Strictly ordered as the tuple, because every field stays inside its bits (kp_tree_fits; rows < 2^18).
#define KP_TREE_KEY_NONE 0xffffffffffffffffull /* no edge: loses to every key (a < b keeps a at 2^18 - 2 or less: no key is all ones) */
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

// kp_clust_unite that names the root it moved: the larger root of a's and b's components goes under the smaller one and is
// returned; -1 when they were one component already.  A root is moved at most once in its life -- a cell that has left its root
// state never returns to it (kp_clust.h) --, so the returned row is a slot no other union of the run is given.
KP_HD int32_t kp_tree_unite(int32_t *parent, int32_t a, int32_t b) {
    for (;;) {
        a = kp_clust_find(parent, a);
        b = kp_clust_find(parent, b);
        if (a == b) return -1;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        if (kp_clust_hook(parent + hi, hi, lo)) return hi;
    }
}

// The forest of a matrix of blocks, serially, by the rounds the device runs: every component's lightest outgoing edge under the
// packed key, then one union per chosen edge.  edges [max(R - 1, 0)] ascend by key, component [R] is the smallest row of every
// row's tree.  Returns the number of edges, or -1 when the round bound was reached with edges still arriving.  `rounds`, if given,
// receives the rounds taken, the empty last one included.
inline int64_t kp_tree_host(const uint64_t *blocks, int32_t R, int64_t nb, int32_t min_compared, kp_dist_pair *edges, int32_t *component, int32_t *rounds = nullptr) {
    if (rounds) *rounds = 0;
    if (R <= 0) return 0;
    const int64_t NW = kp_dist_words(nb);
    std::vector<KpDistWord> words((size_t)R * (size_t)NW);
    for (int32_t r = 0; r < R; ++r)
        for (int64_t w = 0; w < NW; ++w) words[(size_t)r * NW + w] = kp_dist_word_planes(blocks + (size_t)r * (size_t)nb, nb, w);
    const auto counts = [&](int32_t a, int32_t b, int32_t *c) {
        c[0] = c[1] = c[2] = 0;
        for (int64_t w = 0; w < NW; ++w) {
            const KpDistWord &x = words[(size_t)a * NW + w], &y = words[(size_t)b * NW + w];
            kp_dist_word_counts(x.lo, x.hi, x.valid, x.present, y.lo, y.hi, y.valid, y.present, &c[0], &c[1], &c[2]);
        }
    };
    std::vector<int32_t> parent((size_t)R), label((size_t)R);
    for (int32_t r = 0; r < R; ++r) parent[r] = label[r] = r;
    std::vector<uint64_t> cbest((size_t)R), chosen;
    bool ended = false;
    for (int32_t round = 0; round < kp_tree_max_rounds(R) && !ended; ++round) {
        std::fill(cbest.begin(), cbest.end(), KP_TREE_KEY_NONE);
        for (int32_t a = 0; a < R; ++a)
            for (int32_t b = a + 1; b < R; ++b) {
                if (label[a] == label[b]) continue;
                int32_t c[3];
                counts(a, b, c);
                if (c[0] < min_compared) continue;
                const uint64_t k = kp_tree_key(c[1], a, b);
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
        int32_t c[3];
        counts(kp_tree_key_a(chosen[e]), kp_tree_key_b(chosen[e]), c);
        kp_dist_pair_store(edges + e, kp_tree_key_a(chosen[e]), kp_tree_key_b(chosen[e]), c[0], c[1], c[2]);
    }
    for (int32_t r = 0; r < R; ++r) component[r] = label[r];
    return (int64_t)chosen.size();
}
