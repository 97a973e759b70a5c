// kp_alleles.h -- the allele digests of the kept records and the locus pieces (kp_spec.h, ALLELES): a stable 64-bit digest of the
// strand-corrected bases of an interval, of a record's protein bytes and of an assembly's pieces in the product's order.  Written
// once as plain functions: the mixer, block i of an interval (sixteen columns from the packed words and the N runs, on either
// strand, at any offset inside a word), block i of a protein, the term of a block, the finish and the locus combination.  The
// device kernel (kp_alleles.hip) gives every block a lane and adds the lanes' terms; the loops at the end take the blocks one after
// the other (host formatter, tests).  Base codes are read through kp_seqs.h only.  No HIP header: tests/native_harness compiles it
// with g++.
#pragma once

#include "kp_seqs.h"

#define KP_AL_TAG_NT 1
#define KP_AL_TAG_AA 2
#define KP_AL_TAG_LOCUS 3
#define KP_AL_COLS 16 /* columns of a nucleotide block */

KP_HD uint64_t kp_al_mix(uint64_t z) {
    z ^= z >> 30; z *= 0xbf58476d1ce4e5b9ull;
    z ^= z >> 27; z *= 0x94d049bb133111ebull;
    z ^= z >> 31;
    return z;
}

// what block i with value v adds to S, and the digest of a finished sum
KP_HD uint64_t kp_al_term(int64_t i, uint64_t v) { return kp_al_mix(kp_al_mix((uint64_t)i + 1u) ^ v); }
KP_HD uint64_t kp_al_finish(uint64_t S, int tag, uint64_t L) { return kp_al_mix(S ^ kp_al_mix(((uint64_t)tag << 56) | L)); }
KP_HD int64_t kp_al_nt_blocks(int64_t L) { return (L + KP_AL_COLS - 1) / KP_AL_COLS; }
KP_HD int64_t kp_al_aa_blocks(int64_t n) { return (n + 7) / 8; }

// the sixteen base pairs of x in reverse order
KP_HD uint32_t kp_al_reverse_pairs(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    x = __brev(x);  // (bits reversed: the pairs are in place, each the wrong way round)
    return ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
#else
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0f0f0f0fu) | ((x & 0x0f0f0f0fu) << 4);
    x = ((x >> 8) & 0x00ff00ffu) | ((x & 0x00ff00ffu) << 8);
    return (x >> 16) | (x << 16);
#endif
}

// the low sixteen bits of m in reverse order
KP_HD uint32_t kp_al_reverse_16(uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __brev(m) >> 16;
#else
    m = ((m >> 1) & 0x5555u) | ((m & 0x5555u) << 1);
    m = ((m >> 2) & 0x3333u) | ((m & 0x3333u) << 2);
    m = ((m >> 4) & 0x0f0fu) | ((m & 0x0f0fu) << 4);
    return ((m >> 8) | (m << 8)) & 0xffffu;
#endif
}

// bit j of m to bits 2j and 2j + 1, j < 16
KP_HD uint32_t kp_al_pair_mask(uint32_t m) {
    m = (m | (m << 8)) & 0x00ff00ffu;
    m = (m | (m << 4)) & 0x0f0f0f0fu;
    m = (m | (m << 2)) & 0x33333333u;
    m = (m | (m << 1)) & 0x55555555u;
    return m * 3u;
}

// An interval [start, end) of a contig (t: its assembly's words and runs, the contig's bounds) in assembly coordinates, checked: it
// lies inside the contig and inside the assembly's packed words.  One that does not has no digest (0).
KP_HD bool kp_al_interval(const KpTargetSeq &t, int32_t start, int32_t end, int32_t *s, int32_t *e) {
    if (start < 0 || end < start || (int64_t)t.cstart + end > t.cend || t.cstart < 0 || (int64_t)t.cend > (int64_t)t.n_words * 16) return false;
    *s = t.cstart + start; *e = t.cstart + end;
    return true;
}

// no N run touches [s, e): every block of the interval may skip the mask
KP_HD bool kp_al_clear_of_runs(const KpTargetSeq &t, int32_t s, int32_t e) {
    const int a = kp_first_run_after(t.runs, t.n_runs, s);
    return a >= t.n_runs || t.runs[2 * a] >= e;
}

// 1 <= n <= 16 strand-corrected columns of the assembly positions p0 .. p0 + n - 1 (inside the assembly's packed words), with their
// N mask: w | m << 32, column j in bits 2j / bit j, nothing above column n - 1.  Forward, column j is position p0 + j; otherwise it
// is position p0 + n - 1 - j, complemented.  The positions sit in one packed word or in two neighbouring ones, and the second is
// read only where one of them lies in it -- never a word beyond the assembly's last.
KP_HD uint64_t kp_al_cols(const KpTargetSeq &t, int32_t p0, int n, bool fwd, bool clear_of_runs) {
    const int wi = p0 >> 4, sh = 2 * (p0 & 15);
    uint32_t w = t.words[wi] >> sh;
    if (((p0 + n - 1) >> 4) != wi) w |= t.words[wi + 1] << (32 - sh);  // (sh > 0 here)
    uint32_t m = clear_of_runs ? 0u : kp_n_mask(t.runs, t.n_runs, p0, n);
    const uint32_t live = n >= 16 ? ~0u : (1u << (2 * n)) - 1u;
    if (!fwd) {  // column j is position p0 + n - 1 - j, complemented
        w = ~kp_al_reverse_pairs(w) >> (2 * (KP_AL_COLS - n));
        m = kp_al_reverse_16(m) >> (KP_AL_COLS - n);
    }
    w &= live & ~kp_al_pair_mask(m);
    return (uint64_t)w | ((uint64_t)m << 32);
}

// v_i of the interval [s, e) (assembly coordinates, checked by kp_al_interval) on `strand`: w_i | m_i << 32.  i < kp_al_nt_blocks.
// The block's n live columns are assembly positions p0 .. p0 + n - 1.
KP_HD uint64_t kp_al_nt_block(const KpTargetSeq &t, int32_t s, int32_t e, int strand, int64_t i, bool clear_of_runs) {
    const int64_t L = (int64_t)e - s, c0 = i * KP_AL_COLS;
    const int n = (int)(L - c0 < KP_AL_COLS ? L - c0 : KP_AL_COLS);
    const bool fwd = strand >= 0;
    return kp_al_cols(t, fwd ? (int32_t)(s + c0) : (int32_t)(e - c0 - n), n, fwd, clear_of_runs);
}

// v_i of n protein bytes: eight per block, little-endian, zero-padded
KP_HD uint64_t kp_al_aa_block(const uint8_t *p, int64_t n, int64_t i) {
    uint64_t v = 0;
    const int64_t b0 = 8 * i;
    const int m = (int)(n - b0 < 8 ? n - b0 : 8);
    for (int j = 0; j < m; ++j) v |= (uint64_t)p[b0 + j] << (8 * j);
    return v;
}

// ---- the blocks one after the other ------------------------------------------------------------------------------------------------
// nucleotide digest of [start, end) of the contig on `strand` (contig coordinates); 0 for an interval outside the contig
KP_HD uint64_t kp_al_nt_digest(const KpTargetSeq &t, int32_t start, int32_t end, int strand) {
    int32_t s, e;
    if (!kp_al_interval(t, start, end, &s, &e)) return 0;
    const bool clear = kp_al_clear_of_runs(t, s, e);
    uint64_t S = 0;
    for (int64_t i = 0, nb = kp_al_nt_blocks((int64_t)e - s); i < nb; ++i) S += kp_al_term(i, kp_al_nt_block(t, s, e, strand, i, clear));
    return kp_al_finish(S, KP_AL_TAG_NT, (uint64_t)((int64_t)e - s));
}

// protein digest of n bytes (a record with prot_len == 0 has none: its field is 0, which is the caller's to say)
KP_HD uint64_t kp_al_aa_digest(const uint8_t *p, int64_t n) {
    uint64_t S = 0;
    for (int64_t i = 0, nb = kp_al_aa_blocks(n); i < nb; ++i) S += kp_al_term(i, kp_al_aa_block(p, n, i));
    return kp_al_finish(S, KP_AL_TAG_AA, (uint64_t)n);
}

// locus digest: the pieces' nucleotide digests in the product's order (order[k]: index of the k-th piece); 0 without a piece
KP_HD uint64_t kp_al_locus_digest(const uint64_t *piece_digests, const int32_t *order, int n) {
    if (n <= 0) return 0;
    uint64_t S = 0;
    for (int k = 0; k < n; ++k) S += kp_al_term(k, piece_digests[order[k]]);
    return kp_al_finish(S, KP_AL_TAG_LOCUS, (uint64_t)n);
}
