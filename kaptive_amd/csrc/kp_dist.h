// kp_dist.h -- pairwise distances between locus rows (kp_spec.h, DISTANCES), written once as plain functions: the padding mask of a
// gene's last block, the bit planes of a block and of four blocks (one plane word: 64 columns), the three counts of one plane word
// of a pair and of a whole pair (from planes; from two block rows), the key that loses every minimum, the listing predicate, and the
// tile geometry the tile kernels (kp_dist_handle.h, kp_dist.hip) and their host share.  No HIP header: tests/native_harness compiles it with g++.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "kp_seqs.h"  // KP_HD

#define KP_DIST_TILE 64       /* pairs along either side of a workgroup's tile */
#define KP_DIST_CHUNK 8       /* plane words of a row strip that lie in LDS at a time */
#define KP_DIST_REG 4         /* a lane's register tile: KP_DIST_REG x KP_DIST_REG pairs */
#define KP_DIST_WORD_BLOCKS 4 /* blocks of a plane word: 64 columns */
#define KP_DIST_PLANES 4      /* lo, hi, valid, present */
#define KP_DIST_GAP_SHIFT 48  /* the gap mask of a block (KP_ALN_GAP_SHIFT) */
#define KP_DIST_N_SHIFT 32    /* its N mask */

// PADDING.  The gap bits a locus row sets in the last block of a gene of Lq bases: the columns at or beyond Lq.
KP_HD uint64_t kp_dist_pad_mask(int64_t Lq) {
    const int n = (int)(Lq & 15);
    return n ? (uint64_t)((0xffffu << n) & 0xffffu) << KP_DIST_GAP_SHIFT : 0ull;
}

// the even bits of a 32-bit word, packed into its low 16
KP_HD uint32_t kp_dist_even_bits(uint32_t x) {
    x &= 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u;
    x = (x | (x >> 2)) & 0x0f0f0f0fu;
    x = (x | (x >> 4)) & 0x00ff00ffu;
    x = (x | (x >> 8)) & 0x0000ffffu;
    return x;
}

// PLANES of one block, sixteen bits each: the low and the high bit of every column's code, the columns that hold a code 0..3
// (neither N nor GAP) and the columns that are not GAP.  Code bits of columns that are not valid are dropped.
struct KpDistPlanes16 { uint32_t lo, hi, valid, present; };
KP_HD KpDistPlanes16 kp_dist_block_planes(uint64_t v) {
    const uint32_t w = (uint32_t)v, m = (uint32_t)(v >> KP_DIST_N_SHIFT) & 0xffffu, g = (uint32_t)(v >> KP_DIST_GAP_SHIFT) & 0xffffu;
    KpDistPlanes16 p;
    p.valid = ~(m | g) & 0xffffu;
    p.present = ~g & 0xffffu;
    p.lo = kp_dist_even_bits(w) & p.valid;
    p.hi = kp_dist_even_bits(w >> 1) & p.valid;
    return p;
}

// A plane word: the planes of blocks 4 w .. 4 w + 3 of a row of nb blocks, block k in bits 16 k .. 16 k + 15.  The blocks a short
// last word lacks are invalid and not present.
struct KpDistWord { uint64_t lo, hi, valid, present; };
KP_HD KpDistWord kp_dist_word_planes(const uint64_t *row, int64_t nb, int64_t w) {
    KpDistWord q{0, 0, 0, 0};
    for (int k = 0; k < KP_DIST_WORD_BLOCKS; ++k) {
        const int64_t b = w * KP_DIST_WORD_BLOCKS + k;
        if (b >= nb) break;
        const KpDistPlanes16 p = kp_dist_block_planes(row[b]);
        q.lo |= (uint64_t)p.lo << (16 * k); q.hi |= (uint64_t)p.hi << (16 * k);
        q.valid |= (uint64_t)p.valid << (16 * k); q.present |= (uint64_t)p.present << (16 * k);
    }
    return q;
}
KP_HD int64_t kp_dist_words(int64_t nb) { return (nb + KP_DIST_WORD_BLOCKS - 1) / KP_DIST_WORD_BLOCKS; }

// COUNTS of one plane word of a pair, added to the pair's three counters
KP_HD void kp_dist_word_counts(uint64_t la, uint64_t ha, uint64_t va, uint64_t pa, uint64_t lb, uint64_t hb, uint64_t vb, uint64_t pb,
                               int32_t *compared, int32_t *differences, int32_t *unshared) {
    const uint64_t v = va & vb;
    const uint64_t d = ((la ^ lb) | (ha ^ hb)) & v;
    const uint64_t u = pa ^ pb;
    *compared += __builtin_popcountll(v);
    *differences += __builtin_popcountll(d);
    *unshared += __builtin_popcountll(u);
}

// The three counts of rows (a, b) of a matrix of R rows, from its plane-major planes -- planes[(p * NW + w) * R + r]: what a kernel
// recounts for the one pair a row's key names.
struct KpDistCounts { int32_t compared, differences, unshared; };
KP_HD KpDistCounts kp_dist_plane_counts(const uint64_t *planes, int64_t R, int64_t NW, int64_t a, int64_t b) {
    const size_t plane = (size_t)NW * (size_t)R;
    KpDistCounts n{0, 0, 0};
    for (int64_t w = 0; w < NW; ++w) {
        const uint64_t *at = planes + (size_t)w * (size_t)R;
        kp_dist_word_counts(at[a], at[plane + a], at[2 * plane + a], at[3 * plane + a], at[b], at[plane + b], at[2 * plane + b], at[3 * plane + b], &n.compared,
                            &n.differences, &n.unshared);
    }
    return n;
}
// The same of two rows of nb blocks each, for the host restatements.
inline KpDistCounts kp_dist_row_counts(const uint64_t *a, const uint64_t *b, int64_t nb) {
    KpDistCounts n{0, 0, 0};
    for (int64_t w = 0; w < kp_dist_words(nb); ++w) {
        const KpDistWord x = kp_dist_word_planes(a, nb, w), y = kp_dist_word_planes(b, nb, w);
        kp_dist_word_counts(x.lo, x.hi, x.valid, x.present, y.lo, y.hi, y.valid, y.present, &n.compared, &n.differences, &n.unshared);
    }
    return n;
}

// A packed 64-bit key (kp_clust.h: nearest partner; kp_tree.h: edge) that loses every minimum: no partner, no edge.
#define KP_DIST_KEY_NONE 0xffffffffffffffffull

// LISTED PAIRS
KP_HD bool kp_dist_listed(int32_t compared, int32_t differences, int32_t max_diff, int32_t min_compared) {
    return differences <= max_diff && compared >= min_compared;
}

// ---- tiles ---------------------------------------------------------------------------------------------------------------------------
// The tiles on or above the diagonal of an nt x nt grid, row by row: tile row ti holds nt - ti of them, tj = ti .. nt - 1.
KP_HD int64_t kp_dist_tiles(int64_t nt) { return nt * (nt + 1) / 2; }
KP_HD int64_t kp_dist_tile_row_first(int64_t ti, int64_t nt) { return ti * nt - ti * (ti - 1) / 2; }
// tile t of that list, 0 <= t < kp_dist_tiles(nt): a square root names the row to within one, two integer steps settle it
KP_HD void kp_dist_tile_of(int64_t t, int64_t nt, int32_t *ti, int32_t *tj) {
    const double s = (double)(2 * nt + 1);
    int64_t i = (int64_t)((s - __builtin_sqrt(s * s - 8.0 * (double)t)) * 0.5);
    if (i < 0) i = 0;
    if (i > nt - 1) i = nt - 1;
    while (i > 0 && kp_dist_tile_row_first(i, nt) > t) --i;
    while (i + 1 < nt && kp_dist_tile_row_first(i + 1, nt) <= t) ++i;
    *ti = (int32_t)i;
    *tj = (int32_t)(i + (t - kp_dist_tile_row_first(i, nt)));
}

// three 8-byte words, like every record the device stores
static_assert(sizeof(kp_dist_pair) == 24, "a pair record is three 8-byte words");
KP_HD void kp_dist_pair_store(kp_dist_pair *p, int32_t a, int32_t b, int32_t compared, int32_t differences, int32_t unshared) {
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned long long *d = reinterpret_cast<unsigned long long *>(p);
    d[0] = (uint64_t)(uint32_t)a | ((uint64_t)(uint32_t)b << 32);
    d[1] = (uint64_t)(uint32_t)compared | ((uint64_t)(uint32_t)differences << 32);
    d[2] = (uint64_t)(uint32_t)unshared;
#else
    p->a = a; p->b = b; p->compared = compared; p->differences = differences; p->unshared = unshared; p->pad_ = 0;
#endif
}
