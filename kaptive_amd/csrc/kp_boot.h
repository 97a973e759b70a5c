// kp_boot.h -- bootstrap support of the neighbour-joining tree (kp_spec.h, BOOTSTRAP), written once as plain functions: the mixer, the
// draws of a replicate and their clamp, the weight planes of a plane word, the weighted counts of one plane word of a pair and of a
// whole pair, the key of a set of taxa, the side of a split that is compared, and the walk over a tree's records that makes its
// splits.  The kernels of kp_dist_boot.hip and their host share them.  No HIP header: tests/native_harness compiles it with g++.
#pragma once

#include <stdint.h>

#include <vector>

#include "kp_caps.h"
#include "kp_dist.h"
#include "kp_nj.h"

#define KP_BOOT_PLANES 8       /* bit planes of a weight: weights are 0 .. 255 */
#define KP_BOOT_MAX_WEIGHT 255 /* the clamp */

// MIX.  All of it mod 2^64.
KP_HD uint64_t kp_boot_mix(uint64_t x) {
    uint64_t z = x + 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// the high 64 bits of the 128-bit product
KP_HD uint64_t kp_boot_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * (unsigned __int128)b) >> 64);
#endif
}

// DRAWS.  Replicate r of a seed has a stream; draw t of the stream is a column of the W block columns, padding included.
KP_HD uint64_t kp_boot_stream(uint64_t seed, uint64_t r) { return kp_boot_mix(kp_boot_mix(seed) + r); }
KP_HD int64_t kp_boot_draw(uint64_t stream, uint64_t t, int64_t W) { return (int64_t)kp_boot_mulhi64(kp_boot_mix(stream + t), (uint64_t)W); }
// the weight of a column that was drawn `count` times
KP_HD uint32_t kp_boot_weight(uint32_t count) { return count < KP_BOOT_MAX_WEIGHT ? count : KP_BOOT_MAX_WEIGHT; }

// weight[c] of every column c < W of replicate r, serially
inline void kp_boot_weights_host(uint64_t seed, int64_t r, int64_t W, uint8_t *weight) {
    std::vector<uint32_t> count((size_t)W, 0u);
    const uint64_t stream = kp_boot_stream(seed, (uint64_t)r);
    for (int64_t t = 0; t < W; ++t) ++count[(size_t)kp_boot_draw(stream, (uint64_t)t, W)];
    for (int64_t c = 0; c < W; ++c) weight[c] = (uint8_t)kp_boot_weight(count[(size_t)c]);
}

// WEIGHT PLANES of plane word w: M[k] holds bit k of the weights of columns 64 w .. 64 w + 63 (columns at or beyond W weigh 0).
// Returns one more than the highest k with M[k] != 0, 0 for none.
inline int kp_boot_word_planes(const uint8_t *weight, int64_t W, int64_t w, uint64_t (&M)[KP_BOOT_PLANES]) {
    int top = 0;
    for (int k = 0; k < KP_BOOT_PLANES; ++k) M[k] = 0;
    for (int b = 0; b < 64; ++b) {
        const int64_t c = 64 * w + b;
        if (c >= W) break;
        for (int k = 0; k < KP_BOOT_PLANES; ++k)
            if ((weight[c] >> k) & 1) { M[k] |= 1ull << b; if (k + 1 > top) top = k + 1; }
    }
    return top;
}

// WEIGHTED COUNTS of one plane word of a pair, added to the pair's two counters, over the weight planes k < TOP
template <int TOP>
KP_HD void kp_boot_word_counts(uint64_t la, uint64_t ha, uint64_t va, uint64_t lb, uint64_t hb, uint64_t vb, const uint64_t (&M)[KP_BOOT_PLANES],
                               int32_t *compared, int32_t *differences) {
    const uint64_t v = va & vb;
    const uint64_t d = ((la ^ lb) | (ha ^ hb)) & v;
#if defined(__clang__)
#pragma unroll
#endif
    for (int k = 0; k < TOP; ++k) {
        *compared += __builtin_popcountll(v & M[k]) << k;
        *differences += __builtin_popcountll(d & M[k]) << k;
    }
}

// The same of two rows of nb blocks each under weight[16 nb], for the host restatements.
inline KpDistCounts kp_boot_row_counts(const uint64_t *a, const uint64_t *b, int64_t nb, const uint8_t *weight) {
    KpDistCounts n{0, 0, 0};
    for (int64_t w = 0; w < kp_dist_words(nb); ++w) {
        const KpDistWord x = kp_dist_word_planes(a, nb, w), y = kp_dist_word_planes(b, nb, w);
        uint64_t M[KP_BOOT_PLANES];
        kp_boot_word_planes(weight, 16 * nb, w, M);
        kp_boot_word_counts<KP_BOOT_PLANES>(x.lo, x.hi, x.valid, y.lo, y.hi, y.valid, M, &n.compared, &n.differences);
    }
    return n;
}

// SPLITS.  The key of a set of taxa is the sum mod 2^64 of kp_boot_mix(k + 1) over its taxa k; kp_boot_total_key(n) is the key of
// all n taxa.
KP_HD uint64_t kp_boot_taxon_key(int32_t k) { return kp_boot_mix((uint64_t)(int64_t)k + 1); }
KP_HD uint64_t kp_boot_total_key(int32_t n) {
    uint64_t s = 0;
    for (int32_t k = 0; k < n; ++k) s += kp_boot_taxon_key(k);
    return s;
}

// A split as the device compares it: the side without taxon 0.  has0 remembers which side of the node below it that is.
struct KpBootSplit { uint64_t key; int32_t size, has0; };
static_assert(sizeof(KpBootSplit) == 16, "a split is two 8-byte words");
KP_HD bool kp_boot_split_less(const KpBootSplit &x, const KpBootSplit &y) { return x.size < y.size || (x.size == y.size && x.key < y.key); }
KP_HD bool kp_boot_split_same(const KpBootSplit &x, const KpBootSplit &y) { return x.size == y.size && x.key == y.key; }
KP_HD void kp_boot_split_store(KpBootSplit *p, uint64_t key, int32_t size, int32_t has0) {
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned long long *w = reinterpret_cast<unsigned long long *>(p);
    w[0] = key;
    w[1] = (uint64_t)(uint32_t)size | ((uint64_t)(uint32_t)has0 << 32);
#else
    p->key = key; p->size = size; p->has0 = has0;
#endif
}

// How many inner edges -- records with a split -- the tree of n taxa has.
KP_HD int64_t kp_boot_splits(int64_t n) { return n >= 4 ? n - 3 : 0; }

// The splits of the tree of n >= 4 taxa whose records are rec [n - 2]: out[t], t < n - 3, is the split of the node record t made,
// on the side without taxon 0.  The walk is serial: record t reads the splits of the inner nodes made before it from out itself,
// and turns them back to the side below the node by has0.  A child id outside the nodes made before its record -- no tree the join
// loop makes has one -- counts as the empty set.
KP_HD void kp_boot_walk(const kp_nj_node *rec, int32_t n, uint64_t total, KpBootSplit *out) {
    const int64_t S = kp_boot_splits(n);
    for (int64_t t = 0; t < S; ++t) {
        const int32_t child[2] = {rec[t].a, rec[t].b};
        uint64_t key = 0;
        int32_t size = 0, has0 = 0;
        for (int c = 0; c < 2; ++c) {
            const int32_t id = child[c];
            if (id >= 0 && id < n) {
                key += kp_boot_taxon_key(id); size += 1; has0 |= id == 0 ? 1 : 0;
            } else if (id >= n && (int64_t)id - n < t) {
                const KpBootSplit s = out[id - n];
                key += s.has0 ? total - s.key : s.key;
                size += s.has0 ? n - s.size : s.size;
                has0 |= s.has0;
            }
        }
        kp_boot_split_store(out + t, has0 ? total - key : key, has0 ? n - size : size, has0);
    }
}

// BATCH.  The replicates whose matrices are on the device at once: the most whose n x n doubles fit KP_BOOT_MATRIX_BYTES, at least
// one, no more than there are replicates or than a grid has rows, and no more than the caller's own limit (0: none).
KP_HD int32_t kp_boot_batch(int64_t n, int64_t replicates, int64_t max_batch) {
    int64_t b = n > 0 ? KP_BOOT_MATRIX_BYTES / (n * n * 8) : replicates;
    if (b > replicates) b = replicates;
    if (b > KP_BOOT_MAX_BATCH) b = KP_BOOT_MAX_BATCH;
    if (max_batch > 0 && b > max_batch) b = max_batch;
    return (int32_t)(b < 1 ? 1 : b);
}
