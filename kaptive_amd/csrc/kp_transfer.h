// kp_transfer.h -- transfer bootstrap of the neighbour-joining tree (kp_spec.h, TRANSFER), written once as plain functions: the depth
// of a split, the distance of two splits from their sizes and their overlap, the recurrence of a record over what lies below its
// children, the label's thousandths, and a serial restatement of one replicate's transfer distances.  The kernels of
// kp_dist_transfer.hip, the formatter (kp_rows.cpp) and the g++ harness share them.  No HIP header.
#pragma once

#include <stdint.h>

#include <vector>

#include "kp_boot.h"
#include "kp_caps.h"
#include "kp_nj.h"

// DEPTH of a split with s taxa on one side, of n: the taxa of its light side.
KP_HD int32_t kp_transfer_depth(int32_t s, int32_t n) { return s < n - s ? s : n - s; }

// DISTANCE of a split with s taxa and one with z taxa that share c taxa, of n: H = |A xor B|, and the lesser of H and n - H -- what
// it is from B's other side.  The same from either side of either split.
KP_HD int32_t kp_transfer_delta(int32_t s, int32_t z, int32_t c, int32_t n) {
    const int32_t h = s + z - 2 * c;
    return h < n - h ? h : n - h;
}

// RECURRENCE.  What lies below the node record u of a tree of n taxa made: the sum of what lies below its two children.  leaf(k) is
// the value of taxon k -- 1 for a size, k's membership of a set for a count --, node(v) the value record v < u left.  A child id
// outside the nodes made before the record -- no tree the join loop makes has one -- counts nothing.
template <class Leaf, class Node>
KP_HD int32_t kp_transfer_below(const kp_nj_node &rec, int32_t n, int64_t u, Leaf leaf, Node node) {
    const int32_t child[2] = {rec.a, rec.b};
    int32_t sum = 0;
    for (int c = 0; c < 2; ++c) {
        const int32_t id = child[c];
        if (id >= 0 && id < n) sum += leaf(id);
        else if (id >= n && (int64_t)id - n < u) sum += node(id - n);
    }
    return sum;
}

// LABEL.  K = floor((2000 (D - transfer) + D) / (2 D)), D = replicates * (depth - 1) >= 1: the thousandths of 1 - transfer / D,
// halves rounded up.  0 <= transfer <= D; D is below 2^27 and the numerator below 2^39.
KP_HD int64_t kp_transfer_label(int64_t transfer, int64_t replicates, int64_t depth) {
    const int64_t D = replicates * (depth - 1);
    return (2000 * (D - transfer) + D) / (2 * D);
}

// The taxa below the node of every record with an inner edge: size[t], t < n - 3.
inline void kp_transfer_sizes(const kp_nj_node *rec, int32_t n, int32_t *size) {
    for (int64_t t = 0; t < kp_boot_splits(n); ++t)
        size[t] = kp_transfer_below(rec[t], n, t, [](int32_t) { return 1; }, [size](int32_t v) { return size[v]; });
}

// phi[t], t < n - 3, of one replicate's tree against the supported tree `ref`, both [n - 2] records of n >= 4 taxa, serially: sets as
// rows of bytes, the side without taxon 0 of the supported tree, the side below the node of the replicate's.
inline void kp_transfer_host(const kp_nj_node *ref, const kp_nj_node *replicate, int32_t n, int32_t *phi) {
    const int64_t S = kp_boot_splits(n);
    if (S == 0) return;
    std::vector<std::vector<uint8_t>> in((size_t)S, std::vector<uint8_t>((size_t)n, 0));  // in[t][k]: taxon k in A_t
    std::vector<int32_t> s((size_t)S), z((size_t)S);
    for (int64_t t = 0; t < S; ++t) {
        for (int32_t k = 0; k < n; ++k)
            in[(size_t)t][(size_t)k] = (uint8_t)kp_transfer_below(ref[t], n, t, [k](int32_t id) { return id == k ? 1 : 0; },
                                                                  [&in, k](int32_t v) { return (int32_t)in[(size_t)v][(size_t)k]; });
    }
    for (int64_t t = 0; t < S; ++t) {  // (after the whole walk: a record reads the side below its children)
        if (in[(size_t)t][0])
            for (int32_t k = 0; k < n; ++k) in[(size_t)t][(size_t)k] ^= 1;
        s[(size_t)t] = 0;
        for (int32_t k = 0; k < n; ++k) s[(size_t)t] += in[(size_t)t][(size_t)k];
    }
    kp_transfer_sizes(replicate, n, z.data());
    std::vector<int32_t> cnt((size_t)S);
    for (int64_t t = 0; t < S; ++t) {
        const std::vector<uint8_t> &A = in[(size_t)t];
        int32_t best = kp_transfer_depth(s[(size_t)t], n) - 1;
        for (int64_t u = 0; u < S; ++u) {
            cnt[(size_t)u] = kp_transfer_below(replicate[u], n, u, [&A](int32_t k) { return (int32_t)A[(size_t)k]; }, [&cnt](int32_t v) { return cnt[(size_t)v]; });
            const int32_t d = kp_transfer_delta(s[(size_t)t], z[(size_t)u], cnt[(size_t)u], n);
            if (d < best) best = d;
        }
        phi[t] = best;
    }
}
