// kp_sites.h -- variable sites of a matrix of locus rows (kp_spec.h, SITES), written once as plain functions: the five class masks of a
// plane word, the bit-sliced vertical counter a lane of the profile kernel adds them into, the bit-matrix transposition that turns
// the counters of a wave's 64 lanes into per-column counts, the site predicate with its flag, ALLELES / MAJOR / INFORMATIVE, the
// mapping from a matrix column to its gene, the codes of a site row's block, the record store, and the geometry the kernels
// (kp_dist_sites.hip) and their host share.  No HIP header: tests/native_harness compiles it with g++.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "kp_dist.h"

#define KP_SITES_THREADS 256 /* lanes of a workgroup of the profile kernel */
#define KP_SITES_PLANES 4    /* P: bit planes of a lane's counter */
#define KP_SITES_LANE_ROWS ((1 << KP_SITES_PLANES) - 1)           /* rows a lane may add before its P planes would carry out: 2^P - 1 */
#define KP_SITES_SLAB (KP_SITES_THREADS * KP_SITES_LANE_ROWS)     /* rows of one workgroup: every lane its full share */
#define KP_SITES_CLASSES 5   /* what a column of a row can count as: a, c, g, t, N (GAP is the rest) */
#define KP_SITES_CLASS_N 4   /* the class of an N */
#define KP_SITES_BLOCK 16    /* sites of one block of a site row */
#define KP_SITES_FLAGS KP_SITES_CORE /* every flag bit kp_dist_sites_count knows */

// CLASS MASKS of one plane word of one row (kp_dist.h, PLANES): bit j of m[k] says column j of the word holds class k.  lo and hi
// are already cut to valid; present minus valid is N.  What no mask holds is GAP.
struct KpSiteMasks { uint64_t m[KP_SITES_CLASSES]; };
KP_HD KpSiteMasks kp_sites_masks(uint64_t lo, uint64_t hi, uint64_t valid, uint64_t present) {
    KpSiteMasks q;
    q.m[0] = valid & ~lo & ~hi;
    q.m[1] = valid & lo & ~hi;
    q.m[2] = valid & ~lo & hi;
    q.m[3] = valid & lo & hi;
    q.m[KP_SITES_CLASS_N] = present & ~valid;
    return q;
}

// COUNTER.  64 counters of P bits each, bit-sliced: bit j of p[b] is bit b of column j's count.  Adding a mask is a ripple of half
// adders over the planes; after more than KP_SITES_LANE_ROWS adds of a set bit the carry out of the last plane would be lost.
struct KpSiteCounter { uint64_t p[KP_SITES_PLANES]; };
KP_HD void kp_sites_counter_add(KpSiteCounter *c, uint64_t mask) {
    uint64_t carry = mask;
    for (int b = 0; b < KP_SITES_PLANES; ++b) {
        const uint64_t t = c->p[b] & carry;
        c->p[b] ^= carry;
        carry = t;
    }
}
KP_HD int32_t kp_sites_counter_get(const KpSiteCounter *c, int j) {
    int32_t n = 0;
    for (int b = 0; b < KP_SITES_PLANES; ++b) n |= (int32_t)((c->p[b] >> j) & 1ull) << b;
    return n;
}

// TRANSPOSITION.  The 64 lanes of a wave hold one 64-bit word each: a 64 x 64 bit matrix, row = lane.  Six exchanges with the lane
// s = 32, 16, .. 1 away (`other` is that lane's word) transpose it: afterwards bit i of lane j's word is what bit j of lane i's was,
// so a popcount gives lane j the number of lanes that had bit j set.  One step swaps the off-diagonal s x s blocks of every
// 2s x 2s block; the steps commute.
KP_HD uint64_t kp_sites_low_mask(int s) {  // the bits whose index has bit s clear
    return s == 32 ? 0x00000000ffffffffull : s == 16 ? 0x0000ffff0000ffffull : s == 8 ? 0x00ff00ff00ff00ffull : s == 4 ? 0x0f0f0f0f0f0f0f0full
         : s == 2 ? 0x3333333333333333ull : 0x5555555555555555ull;
}
KP_HD uint64_t kp_sites_transpose_step(uint64_t x, uint64_t other, int lane, int s) {
    const uint64_t m = kp_sites_low_mask(s);
    return (lane & s) ? (x & ~m) | ((other >> s) & m) : (x & m) | ((other & m) << s);
}
// the same on the host, all 64 words at once
inline void kp_sites_transpose64(uint64_t *x) {
    for (int s = 32; s >= 1; s >>= 1) {
        uint64_t y[64];
        for (int lane = 0; lane < 64; ++lane) y[lane] = kp_sites_transpose_step(x[lane], x[lane ^ s], lane, s);
        for (int lane = 0; lane < 64; ++lane) x[lane] = y[lane];
    }
}

// SITE, and what is derived from a profile
KP_HD int32_t kp_site_alleles(const int32_t *n) { return (n[0] != 0) + (n[1] != 0) + (n[2] != 0) + (n[3] != 0); }
KP_HD int32_t kp_site_gap(const int32_t *n, int32_t n_n, int32_t R) { return R - n[0] - n[1] - n[2] - n[3] - n_n; }
KP_HD bool kp_site_is(const int32_t *n, int32_t n_n, int32_t R, int32_t flags) {
    if (kp_site_alleles(n) < 2) return false;
    return !(flags & KP_SITES_CORE) || (n_n == 0 && kp_site_gap(n, n_n, R) == 0);
}
KP_HD int32_t kp_site_major(const int32_t *n) {  // the smallest k among those with the largest n[k]
    int32_t k = 0;
    for (int32_t i = 1; i < 4; ++i)
        if (n[i] > n[k]) k = i;
    return k;
}
KP_HD bool kp_site_informative(const int32_t *n) { return (n[0] >= 2) + (n[1] >= 2) + (n[2] >= 2) + (n[3] >= 2) >= 2; }

// GENE OF A COLUMN.  The genes of a locus lie in its rows back to back, gene g in gene_blocks[g] blocks: matrix column `column`
// belongs to the gene whose blocks hold it, at the 0-based position *position of that gene (at or beyond the gene's length: padding).
// -1 for a column outside the matrix.
KP_HD int32_t kp_site_gene(const int64_t *gene_blocks, int32_t n_genes, int64_t column, int64_t *position) {
    if (column < 0) return -1;
    int64_t first = 0;
    for (int32_t g = 0; g < n_genes; ++g) {
        const int64_t cols = gene_blocks[g] * 16;
        if (column < first + cols) {
            *position = column - first;
            return g;
        }
        first += cols;
    }
    return -1;
}

// SITE ROWS.  What column k of a block holds for a row whose planes have the bits (lo, hi, valid, present) at the site; the padding of
// the last block of S sites is kp_dist_pad_mask(S).
KP_HD uint64_t kp_site_block_code(int k, uint64_t lo, uint64_t hi, uint64_t valid, uint64_t present) {
    if (!(present & 1ull)) return 1ull << (KP_DIST_GAP_SHIFT + k);
    if (!(valid & 1ull)) return 1ull << (KP_DIST_N_SHIFT + k);
    return ((lo & 1ull) | ((hi & 1ull) << 1)) << (2 * k);
}
KP_HD int64_t kp_site_row_blocks(int64_t n_sites) { return (n_sites + KP_SITES_BLOCK - 1) / KP_SITES_BLOCK; }

// three 8-byte words, like every record the device stores; the five counts lie behind the column, one int32 each
static_assert(sizeof(kp_site) == 24 && offsetof(kp_site, n) == 4 && offsetof(kp_site, n_n) == 20, "a site record is three 8-byte words");
KP_HD void kp_site_store(kp_site *p, int32_t column, int32_t a, int32_t c, int32_t g, int32_t t, int32_t n_n) {
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned long long *d = reinterpret_cast<unsigned long long *>(p);
    d[0] = (uint64_t)(uint32_t)column | ((uint64_t)(uint32_t)a << 32);
    d[1] = (uint64_t)(uint32_t)c | ((uint64_t)(uint32_t)g << 32);
    d[2] = (uint64_t)(uint32_t)t | ((uint64_t)(uint32_t)n_n << 32);
#else
    p->column = column; p->n[0] = a; p->n[1] = c; p->n[2] = g; p->n[3] = t; p->n_n = n_n;
#endif
}
