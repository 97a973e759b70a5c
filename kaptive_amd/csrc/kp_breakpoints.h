// kp_breakpoints.h -- the breakpoint records of a kept list (kp_spec.h, BREAKPOINTS): which two kept records are fragments of one
// gene, what lies between them and how far the junction is from a contig end.  Written once as plain functions: what a kept record
// contributes to a pair (KpBpFrag), the pair rule, the choice of one a per b over any range of candidates, the inverted-repeat count
// of the bases between two collinear fragments and the record with its store.  The device kernel (kp_breakpoints.hip) gives every b
// a lane and feeds the candidates from LDS.  No HIP header: tests/native_harness compiles it with g++.
#pragma once

#include <string.h>

#include "kp_seqs.h"

// What a pair reads of a kept record.  gene < 0: not eligible (KP_F_SPURIOUS, or a contig the assembly does not have).
struct KpBpFrag {
    int32_t gene, contig, q_start, q_end, t_start, t_end, ctg_len, strand;
};
#define KP_BP_FRAG_WORDS 8

KP_HD KpBpFrag kp_bp_frag(const kp_kept &k, int n_contigs, const int32_t *ctg_len) {
    KpBpFrag f;
    const bool ok = !(k.flags & KP_F_SPURIOUS) && k.gene >= 0 && k.contig >= 0 && k.contig < n_contigs;
    f.gene = ok ? k.gene : -1;
    f.contig = k.contig; f.q_start = k.q_start; f.q_end = k.q_end; f.t_start = k.t_start; f.t_end = k.t_end;
    f.ctg_len = ok ? ctg_len[k.contig] : 0;
    f.strand = k.strand < 0 ? -1 : 1;
    return f;
}

// The derived values of a fragment pair and its key.
struct KpBpPair {
    int32_t kind, rank;
    int64_t dist;
    int32_t q_gap, t_gap, t_lo, edge_a, edge_b;
};

// (a, b) is a fragment pair: its values into p.  The caller has made sure that a and b are different records.
KP_HD bool kp_bp_pair(const KpBpFrag &a, const KpBpFrag &b, KpBpPair &p) {
    if (a.gene < 0 || a.gene != b.gene) return false;
    if (!(a.q_start < b.q_start && a.q_end < b.q_end)) return false;
    if ((int64_t)a.q_end - b.q_start > KP_BP_MAX_OVERLAP) return false;
    const bool fa = a.strand > 0, fb = b.strand > 0;
    const int64_t pos_a = fa ? (int64_t)a.t_end - 1 : a.t_start, pos_b = fb ? b.t_start : (int64_t)b.t_end - 1;
    p.q_gap = b.q_start - a.q_end;
    p.edge_a = fa ? a.ctg_len - a.t_end : a.t_start;
    p.edge_b = fb ? b.t_start : b.ctg_len - b.t_end;
    p.t_gap = 0; p.t_lo = 0;
    if (a.contig != b.contig) {
        p.kind = KP_BP_CONTIGS; p.rank = 2; p.dist = (int64_t)p.edge_a + (int64_t)p.edge_b;
    } else if (fa != fb) {
        p.kind = KP_BP_INVERTED; p.rank = 1; p.dist = pos_a > pos_b ? pos_a - pos_b : pos_b - pos_a;
    } else {
        const int64_t t_gap = fa ? (int64_t)b.t_start - a.t_end : (int64_t)a.t_start - b.t_end;
        if (t_gap >= -KP_BP_MAX_OVERLAP) {
            p.kind = KP_BP_COLLINEAR; p.rank = 0; p.dist = t_gap + KP_BP_MAX_OVERLAP;
            p.t_gap = (int32_t)t_gap;
            if (t_gap > 0) p.t_lo = fa ? a.t_end : b.t_end;
        } else {
            p.kind = KP_BP_DISORDERED; p.rank = 1; p.dist = pos_a > pos_b ? pos_a - pos_b : pos_b - pos_a;
        }
    }
    return true;
}

// The best a met so far for one b: a < 0 while there is none.
struct KpBpBest {
    int32_t a = -1;
    KpBpPair pair;
};

// Candidates [lo, hi) of the kept list against record ib: `frag(i)` is the KpBpFrag of record i.  The key is (rank, dist, index),
// so the result does not depend on the order or the partition in which the candidates are offered.
template <class Frags>
KP_HD void kp_bp_select(const Frags &frag, int lo, int hi, const KpBpFrag &fb, int ib, KpBpBest &best) {
    if (fb.gene < 0) return;
    for (int i = lo; i < hi; ++i) {
        if (i == ib) continue;
        const KpBpFrag fa = frag(i);
        if (fa.gene != fb.gene) continue;
        KpBpPair p;
        if (!kp_bp_pair(fa, fb, p)) continue;
        const bool better = best.a < 0 || p.rank < best.pair.rank ||
                            (p.rank == best.pair.rank && (p.dist < best.pair.dist || (p.dist == best.pair.dist && i < best.a)));
        if (better) { best.a = i; best.pair = p; }
    }
}

// ir_matches of the t_gap bases from contig coordinate t_lo on (ir_cols = min(KP_BP_IR_COLS, t_gap / 2) columns from either end)
KP_HD int kp_bp_inverted_repeat(const KpTargetSeq &t, int t_lo, int t_gap, int ir_cols) {
    int n = 0;
    const int first = t.cstart + t_lo, last = first + t_gap - 1;
    for (int i = 0; i < ir_cols; ++i) {
        const int x = t.code(first + i), y = t.code(last - i);  // (4: inside an N run, 5: outside the contig -- neither pairs)
        if (x <= 3 && y <= 3 && x == 3 - y) ++n;
    }
    return n;
}

// The record of b = ib with its best a; t: the contig of b (read for COLLINEAR records with t_gap >= 2 only)
KP_HD kp_breakpoint kp_bp_record(const KpBpBest &best, int ib, const KpTargetSeq &t) {
    kp_breakpoint r;
    const KpBpPair &p = best.pair;
    r.kept_a = best.a; r.kept_b = ib;
    r.q_gap = p.q_gap; r.t_gap = p.t_gap; r.t_lo = p.t_lo; r.edge_a = p.edge_a; r.edge_b = p.edge_b;
    r.kind = (uint8_t)p.kind; r.ir_cols = 0; r.ir_matches = 0; r.pad_ = 0;
    if (p.kind == KP_BP_COLLINEAR && p.t_gap >= 2) {
        const int cols = p.t_gap / 2 < KP_BP_IR_COLS ? p.t_gap / 2 : KP_BP_IR_COLS;
        r.ir_cols = (uint8_t)cols;
        r.ir_matches = (uint8_t)kp_bp_inverted_repeat(t, p.t_lo, p.t_gap, cols);
    }
    return r;
}

// A record leaves as four 8-byte words, never as single bytes (kp_variants.h has the same rule and DESIGN.md why).
static_assert(sizeof(kp_breakpoint) == 32, "a record is four 8-byte words");
KP_HD void kp_breakpoint_store(kp_breakpoint *p, const kp_breakpoint &v) {
    const uint64_t w0 = (uint64_t)(uint32_t)v.kept_a | ((uint64_t)(uint32_t)v.kept_b << 32);
    const uint64_t w1 = (uint64_t)(uint32_t)v.q_gap | ((uint64_t)(uint32_t)v.t_gap << 32);
    const uint64_t w2 = (uint64_t)(uint32_t)v.t_lo | ((uint64_t)(uint32_t)v.edge_a << 32);
    const uint64_t w3 = (uint64_t)(uint32_t)v.edge_b | ((uint64_t)v.kind << 32) | ((uint64_t)v.ir_cols << 40) | ((uint64_t)v.ir_matches << 48);
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned long long *d = reinterpret_cast<unsigned long long *>(p);  // (device buffers start on 256 bytes; records are 32 bytes)
    d[0] = w0; d[1] = w1; d[2] = w2; d[3] = w3;
#else
    const uint64_t w[4] = {w0, w1, w2, w3};
    memcpy(p, w, sizeof w);
#endif
}
