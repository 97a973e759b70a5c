// kp_clust.h -- single-linkage clusters and nearest neighbours of locus rows (kp_spec.h, CLUSTERS), written once as plain functions:
// the first level of a pair, the nearest key, find / unite over a parent array, and the cluster number of a label.  The cluster
// kernel of kp_dist_graph.hip and its host share them.  No HIP header: tests/native_harness compiles it with g++.
#pragma once

#include <stdint.h>

#include "kp_dist.h"

// LEVELS, as the kernel takes them: by value, so that no lane indexes memory for them.  t[k] for k >= n is never read as a level.
struct KpClustLevels { int32_t t[KP_CLUST_MAX_LEVELS]; int32_t n; };

// kp_dist_clusters' rule for a level list: 0 <= n <= KP_CLUST_MAX_LEVELS, every level >= 0, strictly ascending
KP_HD bool kp_clust_levels_valid(const int32_t *levels, int32_t n) {
    if (n < 0 || n > KP_CLUST_MAX_LEVELS || (n > 0 && !levels)) return false;
    for (int32_t k = 0; k < n; ++k)
        if (levels[k] < 0 || (k > 0 && levels[k] <= levels[k - 1])) return false;
    return true;
}

// FIRST LEVEL of a pair: the smallest k with differences <= T_k, or n.  The levels ascend, so it is the number of levels below
// `differences`; the loop has a fixed length and constant indices (the levels stay in scalar registers on the device).
KP_HD int32_t kp_clust_first_level(const KpClustLevels &L, int32_t differences) {
    int32_t k = 0;
    for (int32_t l = 0; l < KP_CLUST_MAX_LEVELS; ++l) k += (l < L.n && differences > L.t[l]) ? 1 : 0;
    return k;
}

// NEAREST KEY of a partner s at `differences`: a smaller key is a better partner -- fewer differences, then the smaller row.
#define KP_CLUST_KEY_NONE KP_DIST_KEY_NONE /* no partner: loses to every key */
KP_HD uint64_t kp_clust_key(int32_t differences, int32_t s) { return ((uint64_t)(uint32_t)differences << 32) | (uint64_t)(uint32_t)s; }
KP_HD int32_t kp_clust_key_row(uint64_t key) { return key == KP_CLUST_KEY_NONE ? -1 : (int32_t)(uint32_t)key; }
KP_HD int32_t kp_clust_key_differences(uint64_t key) { return key == KP_CLUST_KEY_NONE ? 0 : (int32_t)(uint32_t)(key >> 32); }

// ---- union-find over parent[], parent[x] <= x; a root has parent[x] == x ---------------------------------------------------------------
// The device build reads and writes a cell with relaxed device-scope atomics (a plain load may be kept in a register by the
// compiler and never see another lane's hook); the host build with plain loads and stores.
KP_HD int32_t kp_clust_load(const int32_t *cell) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return *cell;
#endif
}
KP_HD void kp_clust_store(int32_t *cell, int32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    __hip_atomic_store(cell, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    *cell = v;
#endif
}
// parent[x]: x -> v if it still holds x; false when another union hooked x first
KP_HD bool kp_clust_hook(int32_t *cell, int32_t x, int32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    int32_t expect = x;
    return __hip_atomic_compare_exchange_strong(cell, &expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    if (*cell != x) return false;
    *cell = v;
    return true;
#endif
}

#ifndef KP_CLUST_HALVE
#define KP_CLUST_HALVE 1 /* find stores the grandparent into every second cell it passes (path halving) */
#endif

// The root of x.  Every step descends strictly (parent[x] <= x holds for every value any lane ever stores), so the walk ends after
// at most x steps whatever it reads.  A value read late is still an ancestor of x: a cell that has left its root state only ever
// moves to another ancestor.  Path halving stores a grandparent into a cell that was read as a non-root; such a cell never
// becomes a root again, so the store cannot undo a hook.
KP_HD int32_t kp_clust_find(int32_t *parent, int32_t x) {
    for (;;) {
        const int32_t p = kp_clust_load(parent + x);
        if (p == x) return x;
        const int32_t g = kp_clust_load(parent + p);
        if (g == p) return p;
#if KP_CLUST_HALVE
        kp_clust_store(parent + x, g);
#endif
        x = g;
    }
}

// Joins the components of a and b: the larger root goes under the smaller one and is returned; -1 when they were one component
// already.  The loop runs again only when the hook lost to another union -- another lane has made progress; nothing waits for a
// lane.  A root is moved at most once in its life -- a cell that has left its root state never returns to it --, so the returned
// row is a slot no other union of the run is given (the tree's hook kernel keeps its edge there).
KP_HD int32_t kp_clust_unite_root(int32_t *parent, int32_t a, int32_t b) {
    for (;;) {
        a = kp_clust_find(parent, a);
        b = kp_clust_find(parent, b);
        if (a == b) return -1;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        if (kp_clust_hook(parent + hi, hi, lo)) return hi;
    }
}
// False when a and b were one component already.
KP_HD bool kp_clust_unite(int32_t *parent, int32_t a, int32_t b) { return kp_clust_unite_root(parent, a, b) >= 0; }

// An edge of first level k into the parent arrays parent[K][R] of levels k .. K - 1.  Levels nest, and every edge walks its levels
// upwards: where the two rows are one component at a level already, the edges that joined them there go on to join them at every
// level above, so this edge may stop.
KP_HD void kp_clust_edge(int32_t *parent, int64_t R, int32_t K, int32_t k, int32_t a, int32_t b) {
    for (; k < K; ++k)
        if (!kp_clust_unite(parent + (size_t)k * (size_t)R, a, b)) return;
}

// CLUSTER NUMBER.  number[r] = the 1-based rank of label[r] among the roots (label[x] == x) of one level's R labels, ascending.
// False for a label outside [0, r] or one that is not a root.  `rank` is scratch of R cells.
KP_HD bool kp_clust_numbers(const int32_t *label, int32_t R, int32_t *rank, int32_t *number) {
    int32_t n = 0;
    for (int32_t r = 0; r < R; ++r) {
        if (label[r] < 0 || label[r] > r) return false;
        rank[r] = label[r] == r ? ++n : 0;
    }
    for (int32_t r = 0; r < R; ++r) {
        if (rank[label[r]] == 0) return false;
        number[r] = rank[label[r]];
    }
    return true;
}

// two 8-byte words, like every record the device stores
static_assert(sizeof(kp_dist_nearest) == 16, "a nearest record is two 8-byte words");
KP_HD void kp_dist_nearest_store(kp_dist_nearest *p, int32_t row, int32_t compared, int32_t differences, int32_t unshared) {
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned long long *d = reinterpret_cast<unsigned long long *>(p);
    d[0] = (uint64_t)(uint32_t)row | ((uint64_t)(uint32_t)compared << 32);
    d[1] = (uint64_t)(uint32_t)differences | ((uint64_t)(uint32_t)unshared << 32);
#else
    p->row = row; p->compared = compared; p->differences = differences; p->unshared = unshared;
#endif
}
