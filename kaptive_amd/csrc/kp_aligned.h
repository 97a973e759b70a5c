// kp_aligned.h -- the reference-anchored alignment row of one kept hit (kp_spec.h, ALIGNED ROWS): the contig bases of the hit's M
// columns projected onto the database gene's forward coordinates, Lq columns, sixteen to a block.  Written once as plain functions:
// the check of a walk, the segment an M op gives, the placing of a segment's share of a block, and a loop that makes a whole row
// one op after the other (host tests, harness).  The device kernel (kp_aligned.hip) gives the ops to the lanes of a wave for the
// segments and every block to a lane of its own for the columns.  The columns themselves -- n <= 16 strand-corrected codes from an
// assembly position, with their N mask -- are kp_alleles.h's kp_al_cols; base codes are read through kp_seqs.h only, the gene's
// own bases not at all.  No HIP header: tests/native_harness compiles it with g++.
#pragma once

#include "kp_alleles.h"

#define KP_ALN_COLS 16      /* columns of a block: KP_AL_COLS */
#define KP_ALN_GAP_SHIFT 48 /* the gap mask sits above the ALLELES block's code word (0..31) and N mask (32..47) */

// An M op on the gene's forward strand: columns col .. col + len - 1 of the row; column col is assembly position pos, column
// col + x position pos + x (strand +1) or pos - x, complemented (strand -1).  The direction is the hit's, not the segment's.
struct KpAlnSeg {
    int32_t col, pos, len;
};

KP_HD int64_t kp_aln_blocks(int64_t Lq) { return Lq > 0 ? (Lq + KP_ALN_COLS - 1) / KP_ALN_COLS : 0; }

// block j of a row without a covered column: every column below Lq is GAP
KP_HD uint64_t kp_aln_gap_block(int64_t Lq, int64_t j) {
    const int64_t n = Lq - j * KP_ALN_COLS;
    const uint64_t g = n >= KP_ALN_COLS ? 0xffffull : (n <= 0 ? 0ull : (1ull << n) - 1ull);
    return g << KP_ALN_GAP_SHIFT;
}

// The walk of a hit whose ops advance `rows` along the gene as aligned and `cols` along the contig, from row q0 (q_start, or
// Lq - q_end for strand -1) and contig position t_start: it stays inside the gene, inside the contig and inside the assembly's
// packed words.  (kp_variants.hip makes the same check before it walks.)
KP_HD bool kp_aln_walk_ok(const KpTargetSeq &t, int Lq, int q0, int t_start, int64_t rows, int64_t cols) {
    if (Lq <= 0 || q0 < 0 || (int64_t)q0 + rows > Lq || t_start < 0) return false;
    if (t.cstart < 0 || (int64_t)t.cend > (int64_t)t.n_words * 16) return false;
    return (int64_t)t.cstart + t_start + cols <= t.cend;
}

// what an op adds to the two sums of that check
KP_HD int64_t kp_aln_op_rows(uint32_t op) { return (op & 15u) != KP_CIGAR_D ? (int64_t)(op >> KP_CIGAR_SHIFT) : 0; }
KP_HD int64_t kp_aln_op_cols(uint32_t op) { return (op & 15u) != KP_CIGAR_I ? (int64_t)(op >> KP_CIGAR_SHIFT) : 0; }

// SEGMENT RULE.  The M op of `len` columns that begins at row r of the walk (the gene as aligned) and at assembly position t.
KP_HD KpAlnSeg kp_aln_segment(int r, int t, int len, int Lq, bool rev) {
    KpAlnSeg s;
    s.col = rev ? Lq - r - len : r;
    s.pos = rev ? t + len - 1 : t;
    s.len = len;
    return s;
}

// n columns (kp_al_cols' w | m << 32) into block value v from column o of the block on: their gap bits go, their codes and N bits
// come.  o + n <= 16.
KP_HD uint64_t kp_aln_place(uint64_t v, uint64_t cols, int o, int n) {
    const uint64_t g = ((1ull << n) - 1ull) << o;
    v &= ~(g << KP_ALN_GAP_SHIFT);
    return v | ((cols & 0xffffffffull) << (2 * o)) | ((cols >> 32) << (32 + o));
}

// Block j of the row with the share segment s has of it placed (v unchanged where they do not overlap); *covered grows by the
// columns placed.  The assembly positions read are those of the segment: a valid walk keeps them inside the contig.
KP_HD uint64_t kp_aln_block_add(uint64_t v, const KpTargetSeq &t, const KpAlnSeg &s, bool rev, int64_t j, bool clear_of_runs, int *covered) {
    const int64_t lo = j * KP_ALN_COLS, hi = lo + KP_ALN_COLS;
    const int a = (int)(s.col > lo ? s.col : lo), b = (int)((int64_t)s.col + s.len < hi ? (int64_t)s.col + s.len : hi);
    if (b <= a) return v;
    const int n = b - a;
    const int32_t p0 = rev ? s.pos - (b - 1 - s.col) : s.pos + (a - s.col);  // the lowest assembly position of the n columns
    *covered += n;
    return kp_aln_place(v, kp_al_cols(t, p0, n, !rev, clear_of_runs), (int)(a - lo), n);
}

// three 8-byte words, like every record the device stores
static_assert(sizeof(kp_aligned_row) == 24, "a row record is three 8-byte words");
KP_HD void kp_aligned_row_store(kp_aligned_row *p, int64_t off, int32_t gene_len, int32_t covered, int32_t inserted, int32_t n_ins) {
    const uint64_t w0 = (uint64_t)off, w1 = (uint64_t)(uint32_t)gene_len | ((uint64_t)(uint32_t)covered << 32);
    const uint64_t w2 = (uint64_t)(uint32_t)inserted | ((uint64_t)(uint32_t)n_ins << 32);
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned long long *d = reinterpret_cast<unsigned long long *>(p);
    d[0] = w0; d[1] = w1; d[2] = w2;
#else
    p->off = (int64_t)w0; p->gene_len = gene_len; p->covered = covered; p->inserted = inserted; p->n_ins = n_ins;
    (void)w1; (void)w2;
#endif
}

// ---- a whole row, one op after the other -----------------------------------------------------------------------------------------
// The row of a kept record (q_start, q_end, t_start, strand) of a gene of Lq bases whose hit has the ops `ops` (found: the hit was
// found) on contig t: kp_aln_blocks(Lq) blocks into `blocks`, covered / inserted / n_ins into *row (off is the caller's).  False,
// and the all-GAP row, for an invalid walk.
KP_HD bool kp_aligned_row_blocks(const uint32_t *ops, int64_t n_ops, bool found, const KpTargetSeq &t, int Lq, int q_start, int q_end, int t_start,
                                 int strand, uint64_t *blocks, kp_aligned_row *row) {
    const bool rev = strand < 0;
    const int64_t nb = kp_aln_blocks(Lq);
    for (int64_t j = 0; j < nb; ++j) blocks[j] = kp_aln_gap_block(Lq, j);
    row->gene_len = Lq > 0 ? Lq : 0; row->covered = row->inserted = row->n_ins = 0;
    int64_t rows = 0, cols = 0;
    for (int64_t z = 0; z < n_ops; ++z) { rows += kp_aln_op_rows(ops[z]); cols += kp_aln_op_cols(ops[z]); }
    const int q0 = rev ? Lq - q_end : q_start;
    if (!found || !kp_aln_walk_ok(t, Lq, q0, t_start, rows, cols)) return false;
    const int t0 = t.cstart + t_start;
    const bool clear = kp_al_clear_of_runs(t, t0, (int32_t)(t0 + cols));
    int r = q0, tt = t0, covered = 0;
    for (int64_t z = 0; z < n_ops; ++z) {
        const uint32_t kind = ops[z] & 15u;
        const int len = (int)(ops[z] >> KP_CIGAR_SHIFT);
        if (kind == KP_CIGAR_M) {
            if (len > 0) {
                const KpAlnSeg s = kp_aln_segment(r, tt, len, Lq, rev);
                for (int64_t j = s.col / KP_ALN_COLS; j <= ((int64_t)s.col + s.len - 1) / KP_ALN_COLS; ++j)
                    blocks[j] = kp_aln_block_add(blocks[j], t, s, rev, j, clear, &covered);
            }
            r += len; tt += len;
        } else if (kind == KP_CIGAR_I) r += len;
        else if (kind == KP_CIGAR_D) { tt += len; row->inserted += len; row->n_ins += 1; }
    }
    row->covered = covered;
    return true;
}
