// kp_cs.h -- the cs difference string of one hit (kp_spec.h, CS): a pure function of the hit's CIGAR ops and its two sequences,
// written once and templated on where the bytes go.  KpCsCount counts them, KpCsWrite stores them with every store checked
// against the buffer's end; both are fed by the same calls, so the count and the text cannot disagree.  The device kernels
// (kp_cs.hip) give every finished hit a lane.  No HIP header: tests/native_harness compiles it with g++.
//
// M columns are compared a gene word at a time: up to eight rows whose nibbles lie in one word of the packed gene against the
// sixteen bits of the packed contig beside them, spread to nibbles; one XOR and an "any bit of the nibble" fold leave a bit per
// differing column.  A gene code above 3 differs from every 2-bit code by its bit 2; the contig's N runs are ORed in from a
// cursor into the assembly's run list that only moves forward along the hit.
#pragma once

#include "kp_seqs.h"

struct KpCsCount {
    int64_t n = 0;
    KP_HD void put(char) { ++n; }
};

struct KpCsWrite {
    char *buf;
    int64_t pos, cap;  // the next byte goes to buf[pos] if that lies below cap; pos keeps counting
    KP_HD void put(char c) {
        if (pos >= 0 && pos < cap) buf[pos] = c;
        ++pos;
    }
};

// decimal digits of v; lengths below 1000 (nearly every run of a typing batch) without a division
template <class Sink>
KP_HD void kp_cs_num(Sink &out, uint32_t v) {
    if (v < 10u) { out.put((char)('0' + v)); return; }
    if (v < 100u) {
        const uint32_t t = (v * 205u) >> 11;  // v / 10 for v < 1029
        out.put((char)('0' + t)); out.put((char)('0' + (v - 10u * t)));
        return;
    }
    if (v < 1000u) {
        const uint32_t h = (v * 41u) >> 12, r = v - 100u * h;  // v / 100 for v < 1100
        const uint32_t t = (r * 205u) >> 11;
        out.put((char)('0' + h)); out.put((char)('0' + t)); out.put((char)('0' + (r - 10u * t)));
        return;
    }
    char d[10];
    int n = 0;
    while (v) { d[n++] = (char)('0' + v % 10u); v /= 10u; }
    while (n) out.put(d[--n]);
}

KP_HD char kp_cs_letter(unsigned code) { return code > 3u ? 'n' : (char)("acgt"[code]); }

// the cursor into the assembly's N runs, as a hit is walked along the target (kp_variants.h walks with it too)
struct KpRunCursor {
    const KpTargetSeq &t;
    int run;  // first N run whose end lies beyond the position last asked about
    KP_HD KpRunCursor(const KpTargetSeq &tt, int t0) : t(tt), run(kp_first_run_after(tt.runs, tt.n_runs, t0)) {}
    // positions are asked about in ascending order only
    KP_HD void seek(int pos) { while (run < t.n_runs && t.runs[2 * run + 1] <= pos) ++run; }
    KP_HD bool in_run(int pos) { seek(pos); return run < t.n_runs && t.runs[2 * run] <= pos; }
    // bit j: column pos + j lies in an N run, j < k <= 8
    KP_HD uint32_t n_mask(int pos, int k) {
        seek(pos);
        uint32_t m = 0;
        for (int a = run; a < t.n_runs && t.runs[2 * a] < pos + k; ++a) {
            const int s = t.runs[2 * a] > pos ? t.runs[2 * a] - pos : 0, e = t.runs[2 * a + 1] - pos < k ? t.runs[2 * a + 1] - pos : k;
            if (e > s) m |= ((1u << e) - 1u) & ~((1u << s) - 1u);
        }
        return m;
    }
};

// the open run of identical columns on top of the cursor
template <class Sink>
struct KpCsWalk : KpRunCursor {
    Sink &out;
    uint32_t same = 0;  // identical columns not yet written
    KP_HD KpCsWalk(Sink &o, const KpTargetSeq &tt, int t0) : KpRunCursor(tt, t0), out(o) {}
    KP_HD void close_same() {
        if (!same) return;
        out.put(':'); kp_cs_num(out, same);
        same = 0;
    }
};

// 16 bits, two per base -> eight nibbles holding the codes
KP_HD uint32_t kp_cs_spread(uint32_t x) {
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;
    return x;
}
// a bit per non-zero nibble, gathered into the low eight bits
KP_HD uint32_t kp_cs_any_nibble(uint32_t d) {
    uint32_t x = (d | (d >> 1) | (d >> 2) | (d >> 3)) & 0x11111111u;
    x = (x | (x >> 3)) & 0x03030303u;
    x = (x | (x >> 6)) & 0x000F000Fu;
    return (x | (x >> 12)) & 0xFFu;
}
KP_HD int kp_cs_ctz8(uint32_t m) {  // lowest set bit of a non-zero 8-bit mask
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffs((int)m) - 1;
#else
    return __builtin_ctz(m);
#endif
}

// Up to eight M columns whose rows r .. r + k lie in one word of the packed gene, against the contig from column t: the gene's
// nibbles, the contig's codes spread to nibbles, the columns inside an N run and a bit per differing column (kp_spec.h, CS:
// identical iff both codes are <= 3 and equal).  The cs walk below and the variant walk (kp_variants.h) compare with it.
struct KpCsCols { uint32_t g, tn, nm, diff; };
KP_HD KpCsCols kp_cs_columns(const KpTaskSeqs &s, KpRunCursor &w, int r, int t, int k) {
    const uint32_t keep = k == 8 ? ~0u : (1u << (4 * k)) - 1u;
    KpCsCols c;
    c.g = (s.q.nib[r >> 3] >> (4 * (r & 7))) & keep;
    const int sh = 2 * (t & 15);
    uint32_t bits = s.t.words[t >> 4] >> sh;
    if ((t & 15) + k > 16) bits |= s.t.words[(t >> 4) + 1] << (32 - sh);  // (sh > 0 here)
    c.tn = kp_cs_spread(bits & 0xFFFFu) & keep;
    c.nm = w.n_mask(t, k);
    c.diff = kp_cs_any_nibble(c.g ^ c.tn) | c.nm;
    return c;
}

// The hit's cs string into `out`.  ops: its n_ops CIGAR ops along the target; q0: first row of the path in the gene as aligned
// (s.q is that strand's codes); t0: first column, in the assembly's padded space.
template <class Sink>
KP_HD void kp_cs_hit(const uint32_t *ops, int64_t n_ops, const KpTaskSeqs &s, int q0, int t0, Sink &out) {
    KpCsWalk<Sink> w(out, s.t, t0);
    int r = q0, t = t0;
    for (int64_t z = 0; z < n_ops; ++z) {
        const uint32_t kind = ops[z] & 15u;
        int left = (int)(ops[z] >> KP_CIGAR_SHIFT);
        if (kind == KP_CIGAR_M) {
            while (left > 0) {
                const int in_word = 8 - (r & 7), k = left < in_word ? left : in_word;  // rows of one gene word
                const KpCsCols c = kp_cs_columns(s, w, r, t, k);
                const uint32_t g = c.g, tn = c.tn, nm = c.nm;
                uint32_t diff = c.diff;
                if (!diff) w.same += (uint32_t)k;
                else {
                    int at = 0;
                    while (diff) {
                        const int j = kp_cs_ctz8(diff);
                        diff &= diff - 1u;
                        w.same += (uint32_t)(j - at);
                        w.close_same();
                        out.put('*');
                        out.put(((nm >> j) & 1u) ? 'n' : kp_cs_letter(kp_nib(tn, j)));
                        out.put(kp_cs_letter(kp_nib(g, j)));
                        at = j + 1;
                    }
                    w.same += (uint32_t)(k - at);
                }
                r += k; t += k; left -= k;
            }
        } else if (kind == KP_CIGAR_I) {
            w.close_same();
            out.put('+');
            for (; left > 0; --left, ++r) out.put(kp_cs_letter((unsigned)s.q.code(r)));
        } else if (kind == KP_CIGAR_D) {
            w.close_same();
            out.put('-');
            for (; left > 0; --left, ++t)
                out.put(w.in_run(t) ? 'n' : kp_cs_letter((s.t.words[t >> 4] >> (2 * (t & 15))) & 3u));
        }
    }
    w.close_same();
}
