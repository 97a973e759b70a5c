// kp_variants.h -- the variant records of one kept hit (kp_spec.h, VARIANTS): a pure function of the hit's CIGAR ops and its two
// sequences, written once and templated on where the records go.  KpVarCount counts them, KpVarStore stores them with every
// store checked against the buffer's end and against the hit's own range; both are fed by the same calls, so the count and the
// records cannot disagree.  The device kernels (kp_variants.hip) give every kept record a lane.  No HIP header:
// tests/native_harness compiles it with g++.
//
// The walk is the cs walk's (kp_cs.h): M columns a gene word at a time through kp_cs_columns, one record per differing column,
// one per I and per D op.  It runs along the target, i.e. along the gene AS ALIGNED; positions are turned to the gene's forward
// strand record by record, and a strand -1 hit stores its records back to front so that they ascend in q_pos.
#pragma once

#include <string.h>

#include "kp_cs.h"

struct KpVarCount {
    int64_t n = 0;
    KP_HD void put(const kp_variant &) { ++n; }
};

// A record leaves as three 8-byte words (24 bytes on an 8-byte boundary), never as single bytes: DESIGN.md section 8 item 7 has
// what byte stores cost the cs emit.
static_assert(sizeof(kp_variant) == 24, "a record is three 8-byte words");
KP_HD void kp_variant_store(kp_variant *p, const kp_variant &v) {
    const uint64_t w0 = (uint64_t)(uint32_t)v.kept | ((uint64_t)(uint32_t)v.q_pos << 32);
    const uint64_t w1 = (uint64_t)(uint32_t)v.t_pos | ((uint64_t)(uint32_t)v.len << 32);
    const uint64_t w2 = (uint64_t)v.kind | ((uint64_t)v.ref << 8) | ((uint64_t)v.alt << 16) | ((uint64_t)v.ref_aa << 24) | ((uint64_t)v.alt_aa << 32);
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned long long *d = reinterpret_cast<unsigned long long *>(p);  // (device buffers start on 256 bytes; 24 * i is a multiple of 8)
    d[0] = w0; d[1] = w1; d[2] = w2;
#else
    const uint64_t w[3] = {w0, w1, w2};
    memcpy(p, w, sizeof w);
#endif
}

struct KpVarStore {
    kp_variant *buf;
    int64_t base, n, cap;  // the hit's n records go to buf[base .. base + n), as far as that lies below cap
    bool rev;              // the k-th record of the walk goes to base + n - 1 - k (strand -1) instead of base + k
    int64_t k = 0;         // records met so far; keeps counting
    KP_HD void put(const kp_variant &v) {
        const int64_t at = base + (rev ? n - 1 - k : k);
        if (k < n && at >= 0 && at < cap) kp_variant_store(buf + at, v);
        ++k;
    }
};

KP_HD unsigned kp_var_comp(unsigned code) { return code > 3u ? 4u : 3u - code; }

// The hit's records into `out`.  ops, s, q0, t0: as kp_cs_hit takes them (the gene as aligned, the path's first row and column);
// fwd: the gene's forward-strand codes (the codon is the database gene's, whichever strand was aligned); rev: the hit is strand -1;
// kept: what goes into kp_variant::kept; codon: the 125-entry table of kp_fill_codon_table.
template <class Sink>
KP_HD void kp_variants_hit(const uint32_t *ops, int64_t n_ops, const KpTaskSeqs &s, const KpQuerySeq &fwd, int q0, int t0, bool rev, int32_t kept,
                           const uint8_t *codon, Sink &out) {
    KpRunCursor w(s.t, t0);
    const int len = s.q.len;
    int r = q0, t = t0;
    kp_variant v;
    v.kept = kept;
    v.pad_[0] = v.pad_[1] = v.pad_[2] = 0;
    for (int64_t z = 0; z < n_ops; ++z) {
        const uint32_t kind = ops[z] & 15u;
        int left = (int)(ops[z] >> KP_CIGAR_SHIFT);
        if (kind == KP_CIGAR_M) {
            while (left > 0) {
                const int in_word = 8 - (r & 7), k = left < in_word ? left : in_word;  // rows of one gene word
                const KpCsCols c = kp_cs_columns(s, w, r, t, k);
                for (uint32_t diff = c.diff; diff; diff &= diff - 1u) {
                    const int j = kp_cs_ctz8(diff);
                    unsigned gc = kp_nib(c.g, j), tc = ((c.nm >> j) & 1u) ? 4u : kp_nib(c.tn, j);
                    if (gc > 4u) gc = 4u;
                    const int qp = rev ? len - 1 - (r + j) : r + j;
                    const unsigned ref = rev ? kp_var_comp(gc) : gc, alt = rev ? kp_var_comp(tc) : tc;
                    v.q_pos = qp; v.t_pos = t + j - s.t.cstart; v.len = 1;
                    v.kind = KP_VAR_SNV; v.ref = (uint8_t)ref; v.alt = (uint8_t)alt;
                    const int c0 = qp - qp % 3;
                    if (c0 + 3 <= len) {
                        unsigned cd[3];
                        for (int x = 0; x < 3; ++x) { cd[x] = (unsigned)fwd.code(c0 + x); if (cd[x] > 4u) cd[x] = 4u; }
                        v.ref_aa = codon[cd[0] * 25 + cd[1] * 5 + cd[2]];
                        cd[qp - c0] = alt;
                        v.alt_aa = codon[cd[0] * 25 + cd[1] * 5 + cd[2]];
                    } else v.ref_aa = v.alt_aa = (uint8_t)'X';  // the gene ends inside its last codon
                    out.put(v);
                }
                r += k; t += k; left -= k;
            }
            continue;
        }
        if (kind != KP_CIGAR_I && kind != KP_CIGAR_D) continue;
        v.t_pos = t - s.t.cstart; v.len = left;
        v.ref = v.alt = v.ref_aa = v.alt_aa = 0;
        if (kind == KP_CIGAR_I) {  // rows r .. r + left of the gene as aligned have no column
            v.kind = KP_VAR_DEL; v.q_pos = rev ? len - r - left : r;
            r += left;
        } else {  // columns t .. t + left lie between rows r - 1 and r
            v.kind = KP_VAR_INS; v.q_pos = rev ? len - r : r;
            t += left;
        }
        out.put(v);
    }
}
