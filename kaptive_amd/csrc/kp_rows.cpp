// kp_rows.cpp -- KaptiveRow TSV bytes for a whole batch, straight from the records of the batched reduction (host only).
//
// Stands in for KaptiveRow.from_result + __bytes__ (src/kaptive/serotyping/io.py:191-296, 37-43) called once per genome
// through a SerotypingResult object: SURVEY.md section 8 row a15.  The reference builds 22 byte strings per genome in a
// Python loop over the kept hits; here one call formats every assembly of a batch from the arrays kp_batch_typing
// returned plus the per-assembly decisions the host finished column-wise (kaptive_amd/serotyping/batch.py).  Number
// formatting is C's "%.2f" on the same doubles Python's "%.2f" gets (float32 identities / coverages widen exactly), so
// the bytes are identical; tests compare them with the reference's golden rows.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kaptive_amd.h"
#include "kp_alleles.h"
#include "kp_clust.h"
#include "kp_sites.h"
#include "kp_boot.h"
#include "kp_transfer.h"
#include "kp_nj.h"
#include "kp_pars.h"

namespace {

struct Out {
    char *p;
    int64_t cap, n = 0;  // n keeps counting past cap: the caller learns how much room the rows need
    inline void put(const char *s, int64_t len) {
        if (n + len <= cap) std::memcpy(p + n, s, (size_t)len);
        n += len;
    }
    inline void put(char c) {
        if (n < cap) p[n] = c;
        ++n;
    }
    inline void lit(const char *s) { put(s, (int64_t)std::strlen(s)); }
    inline void pct(double v) {  // "%.2f%%"
        char buf[64];
        const int len = std::snprintf(buf, sizeof buf, "%.2f%%", v);
        put(buf, len);
    }
    // "%.2f%%" of a float32 value in [0, 2^20): the product with 100 is exact in double (24 + 7 significant bits), so
    // rounding it to an integer with ties to even is what printf does with the exact decimal expansion
    inline void pct_f32(float v) {
        if (!(v >= 0.0f && v < 1048576.0f)) { pct((double)v); return; }
        long long cents = std::llrint((double)v * 100.0);
        char buf[24];
        int at = 24;
        buf[--at] = '%';
        buf[--at] = (char)('0' + cents % 10); cents /= 10;
        buf[--at] = (char)('0' + cents % 10); cents /= 10;
        buf[--at] = '.';
        do { buf[--at] = (char)('0' + cents % 10); cents /= 10; } while (cents);
        put(buf + at, 24 - at);
    }
    inline void unum(unsigned long long v) {  // "%llu"
        char buf[24];
        int at = 24;
        do { buf[--at] = (char)('0' + v % 10); v /= 10; } while (v);
        put(buf + at, 24 - at);
    }
    inline void num(long long v) {  // "%lld" (negated as unsigned: LLONG_MIN has no positive twin)
        if (v < 0) { put('-'); unum(0ull - (unsigned long long)v); }
        else unum((unsigned long long)v);
    }
};

inline bool out_ok(const char *out, int64_t cap) { return cap >= 0 && (cap == 0 || out); }  // the output buffer of a call
inline bool alive(const kp_kept &k) { return (k.flags & KP_F_SPURIOUS) == 0; }
inline void put_strand(Out &o, int strand) { o.put(strand < 0 ? '-' : '+'); }
inline void put_hex(Out &o, uint64_t v) {  // 16 digits
    char buf[16];
    for (int i = 15; i >= 0; --i, v >>= 4) buf[i] = "0123456789abcdef"[v & 15u];
    o.put(buf, 16);
}
template <class Off>  // (the name tables of the rows have 32-bit offsets, the others 64-bit ones)
inline void put_name(Out &o, const char *names, const Off *off, int64_t i) { o.put(names + off[i], off[i + 1] - off[i]); }
static const char *const STATE_NAMES[] = {"normal", "partial", "truncated", "below_id_threshold"};  // by KP_STATE_*
inline const char *state_name(int state) { return state >= KP_STATE_NORMAL && state <= KP_STATE_NOVEL ? STATE_NAMES[state] : nullptr; }  // (null: no such state)
// The first n columns of a block as text (kp_spec.h, ALIGNED ROWS; a site row's blocks have the same layout, kp_dist.h): a gap bit
// gives '-', an N bit 'n', anything else the letter of its 2-bit code.
inline void put_block_text(Out &o, uint64_t v, int n) {
    const uint32_t m = (uint32_t)(v >> KP_DIST_N_SHIFT) & 0xffffu, g = (uint32_t)(v >> KP_DIST_GAP_SHIFT) & 0xffffu;
    char buf[16];
    for (int k = 0; k < n; ++k) buf[k] = ((g >> k) & 1u) ? '-' : (((m >> k) & 1u) ? 'n' : "acgt"[(v >> (2 * k)) & 3u]);
    o.put(buf, n);
}

// ---- the tables over the records of a batch (kp_spec.h, VARIANTS, BREAKPOINTS, ALLELES, ALIGNED ROWS, RESCUE) ----
// The names of a batch: its genes, its assemblies and, assembly by assembly, their contigs.
struct BatchNames {
    const kp_variant_tables *t;
    struct Window { int64_t c0, nc; };  // the contigs of one assembly: nc of them from c0 on
    bool ok(int32_t n_asm) const { return t && (n_asm <= 0 || (t->asm_name_off && t->asm_first_ctg)); }
    Window window(int a) const { return Window{t->asm_first_ctg[a], t->asm_first_ctg[a + 1] - t->asm_first_ctg[a]}; }
    bool gene_ok(int32_t gene) const { return gene >= 0 && gene < t->n_genes; }
    static bool contig_ok(Window w, int32_t contig) { return contig >= 0 && contig < w.nc; }
    template <class Rec>  // a record's gene is one of the database's and its contig one of its assembly's
    bool gene_contig_ok(const Rec &r, Window w) const { return gene_ok(r.gene) && contig_ok(w, r.contig); }
    void put_asm(Out &o, int a) const { put_name(o, t->asm_names, t->asm_name_off, a); }
    void put_gene(Out &o, int32_t gene) const { put_name(o, t->gene_names, t->gene_name_off, gene); }
    void put_contig(Out &o, Window w, int32_t contig) const { put_name(o, t->ctg_names, t->ctg_name_off, w.c0 + contig); }
};
// The records of a batch, assembly a's being off[a] .. off[a + 1]: the ends ascend, there are records where any are counted, every run ascends.
inline bool run_ok(const int64_t *off, int a) { return off[a + 1] >= off[a]; }
inline bool runs_ok(const int64_t *off, int32_t n_asm, const void *recs) {
    bool ok = n_asm <= 0 || (off && off[n_asm] >= off[0] && (off[n_asm] == off[0] || recs));
    for (int a = 0; ok && a < n_asm; ++a) ok = run_ok(off, a);
    return ok;
}

// ---- the tables over the rows of one locus's matrix (kp_spec.h, DISTANCES, CLUSTERS, TREE, SITES) ----
// The names of the n rows, as the caller stacked them: row r is called names[name_off[at(r)] .. name_off[at(r) + 1]), at(r) = rows[r]
// where a mapping is given.
struct RowNames {
    const char *names; const int64_t *name_off; int32_t n; const int32_t *rows;
    int32_t at(int32_t r) const { return rows ? rows[r] : r; }
    bool valid(int32_t r) const {  // r is a row and its name a run of the table (name_off is not null)
        if (r < 0 || r >= n || at(r) < 0 || at(r) >= n) return false;
        const int64_t *off = name_off + at(r);
        return off[1] >= off[0] && (off[1] == off[0] || names);
    }
    bool valid() const {  // every row
        bool ok = n >= 0 && (n == 0 || name_off);
        for (int32_t r = 0; ok && r < n; ++r) ok = valid(r);
        return ok;
    }
    void put(Out &o, int32_t r) const { put_name(o, names, name_off, at(r)); }
};
// the locus name and the output buffer of a call; an empty name may come as a null pointer
inline bool locus_and_out_ok(const char *locus_name, int32_t len, const char *out, int64_t cap) { return len >= 0 && (len == 0 || locus_name) && out_ok(out, cap); }
inline void put_locus(Out &o, const char *locus_name, int32_t len) { if (len > 0) o.put(locus_name, len); }

// how many distinct genes the selected hits have (np.unique(gene_indices[mask]) in the reference)
template <class Pred>
int distinct_genes(const kp_kept *k, int n, Pred pred) {
    int count = 0;
    for (int i = 0; i < n; ++i) {
        if (!alive(k[i]) || !pred(k[i])) continue;
        bool seen = false;
        for (int j = 0; j < i && !seen; ++j) seen = alive(k[j]) && pred(k[j]) && k[j].gene == k[i].gene;
        count += seen ? 0 : 1;
    }
    return count;
}

// "id,ident%,cov%[,state]" per selected hit, ';'-joined (io.py _gene_details)
template <class Pred>
void details(Out &o, const kp_row_tables *t, const kp_kept *k, int n, Pred pred) {
    bool first = true;
    for (int i = 0; i < n; ++i) {
        if (!alive(k[i]) || !pred(k[i])) continue;
        if (!first) o.put(';');
        first = false;
        put_name(o, t->gene_ids, t->gene_id_off, k[i].gene);
        o.put(',');
        o.pct_f32(k[i].pident);
        o.put(',');
        o.pct_f32(k[i].coverage);
        if (k[i].state != KP_STATE_NORMAL && state_name(k[i].state)) { o.put(','); o.lit(state_name(k[i].state)); }  // (a normal gene gets no word)
    }
}

void share(Out &o, int n, int total) {  // "%d / %d (%.2f%%)"
    if (!total) { o.lit("0 / 0 (0.00%)"); return; }
    o.num(n); o.lit(" / "); o.num(total); o.lit(" (");
    o.pct((double)n / (double)total * 100.0);
    o.put(')');
}

}  // namespace

extern "C" int64_t kp_format_rows(const kp_row_tables *t, int32_t n_asm, const kp_asm_summary *sums, const kp_kept *kept,
                                  int32_t kept_stride, const kp_row_columns *c, char *out, int64_t cap) {
    if (!t || !c || n_asm < 0 || (n_asm > 0 && (!sums || !kept)) || !out_ok(out, cap)) return KP_EINVAL;
    Out o{out, cap};
    for (int a = 0; a < n_asm; ++a) {
        const kp_asm_summary &s = sums[a];
        const kp_kept *k = kept + (size_t)a * (size_t)kept_stride;
        const int n = s.n_kept;
        const int best = c->best_locus[a];
        o.put(t->prefix, t->prefix_len);  // Kaptive version, database name, database version (tab-terminated)
        put_name(o, c->asm_ids, c->asm_id_off, a); o.put('\t');
        put_name(o, t->locus_names, t->locus_name_off, best); o.put('\t');
        put_name(o, c->phenotypes, c->phenotype_off, a); o.put('\t');
        o.lit(c->typeable[a] ? "Typeable" : "Untypeable"); o.put('\t');
        static const char symbols[] = "?+-*!";  // SerotypingProblem.to_symbols (models.py:82-92)
        for (int bit = 0; bit < 5; ++bit)
            if (c->problems[a] & (1 << bit)) o.put(symbols[bit]);
        o.put('\t');
        o.pct(c->identity[a]); o.put('\t');
        o.pct(c->coverage[a]); o.put('\t');
        if (std::isnan(c->length_discrepancy[a])) o.lit("n/a");
        else o.num((long long)c->length_discrepancy[a]);
        o.put('\t');
        auto in_exp = [](const kp_kept &h) { return (h.flags & KP_F_INSIDE) && (h.flags & KP_F_EXPECTED); };
        auto out_exp = [](const kp_kept &h) { return !(h.flags & KP_F_INSIDE) && (h.flags & KP_F_EXPECTED); };
        auto in_other = [](const kp_kept &h) { return (h.flags & KP_F_INSIDE) && !(h.flags & (KP_F_EXPECTED | KP_F_EXTRA)); };
        auto out_other = [](const kp_kept &h) { return !(h.flags & KP_F_INSIDE) && !(h.flags & (KP_F_EXPECTED | KP_F_EXTRA)); };
        const int n_in = distinct_genes(k, n, in_exp), n_out = distinct_genes(k, n, out_exp);
        const int total = n_in + n_out + s.n_missing;
        share(o, n_in, total); o.put('\t');
        details(o, t, k, n, in_exp); o.put('\t');
        {  // missing expected genes, in database order
            const int g0 = t->locus_gene_off[best], ng = t->locus_gene_len[best] < KP_MAX_LOCUS_GENES ? t->locus_gene_len[best] : KP_MAX_LOCUS_GENES;
            bool first = true;
            for (int j = 0; j < ng; ++j) {
                if (!((s.missing_mask[j >> 6] >> (j & 63)) & 1ull)) continue;
                if (!first) o.put(';');
                first = false;
                put_name(o, t->gene_ids, t->gene_id_off, g0 + j);
            }
        }
        o.put('\t');
        o.num(distinct_genes(k, n, in_other)); o.put('\t');
        details(o, t, k, n, in_other); o.put('\t');
        share(o, n_out, total); o.put('\t');
        details(o, t, k, n, out_exp); o.put('\t');
        o.num(distinct_genes(k, n, out_other)); o.put('\t');
        details(o, t, k, n, out_other); o.put('\t');
        details(o, t, k, n, [](const kp_kept &h) { return h.state == KP_STATE_TRUNCATED || h.state == KP_STATE_PARTIAL; });
        o.put('\t');
        details(o, t, k, n, [](const kp_kept &h) { return (h.flags & KP_F_EXTRA) != 0; });
        o.put('\n');
    }
    return o.n;
}

// ---- PAF lines of a hit table (kp_spec.h, CIGAR) ------------------------------------------------------------------------------
// One line per hit, in the table's order: what minimap2 writes for a mapping with -c (the reference keeps the same columns and
// the CIGAR in its Alignments table, src/kaptive/core/alignment.py:392-474, 872).  A loop over the hits in Python costs a
// thousand times the typing of the batch it sits beside.
namespace {

// cs string of one hit (kp_spec.h, CS) checked against its ops: grammar, canonical form, column totals.  With `eqx` the =/X
// CIGAR it stands for goes to `o`.
bool cs_check(const char *cs, int64_t n, const uint32_t *ops, int64_t n_ops, Out *eqx) {
    long long want[3] = {0, 0, 0}, got[3] = {0, 0, 0};
    for (int64_t z = 0; z < n_ops; ++z) {
        if ((ops[z] & 15u) > KP_CIGAR_D) return false;
        want[ops[z] & 15u] += ops[z] >> KP_CIGAR_SHIFT;
    }
    auto base = [](char c) { return c == 'a' || c == 'c' || c == 'g' || c == 't' || c == 'n'; };
    char prev = 0;
    for (int64_t i = 0; i < n;) {
        const char kind = cs[i++];
        if (kind == ':') {
            unsigned long long v = 0;
            const int64_t i0 = i;
            for (; i < n && cs[i] >= '0' && cs[i] <= '9' && i - i0 < 10; ++i) v = v * 10 + (unsigned)(cs[i] - '0');
            if (i == i0 || cs[i0] == '0' || prev == ':') return false;  // no number, :0 or a leading zero, two : tokens touching
            got[KP_CIGAR_M] += (long long)v;
            if (eqx) { eqx->unum(v); eqx->put('='); }
        } else if (kind == '*') {
            if (i + 2 > n || !base(cs[i]) || !base(cs[i + 1])) return false;
            i += 2;
            got[KP_CIGAR_M] += 1;
            if (eqx) {  // a run of * tokens is one X op
                unsigned long long k = 1;
                for (; i + 3 <= n && cs[i] == '*' && base(cs[i + 1]) && base(cs[i + 2]); i += 3) { ++k; got[KP_CIGAR_M] += 1; }
                eqx->unum(k); eqx->put('X');
            }
        } else if (kind == '+' || kind == '-') {
            const int64_t i0 = i;
            while (i < n && base(cs[i])) ++i;
            if (i == i0) return false;
            got[kind == '+' ? KP_CIGAR_I : KP_CIGAR_D] += i - i0;
            if (eqx) { eqx->unum((unsigned long long)(i - i0)); eqx->put(kind == '+' ? 'I' : 'D'); }
        } else return false;
        prev = kind;
    }
    return got[0] == want[0] && got[1] == want[1] && got[2] == want[2];
}

int64_t format_paf(const kp_paf_tables *t, int32_t n_asm, const kp_hit *hits, const int64_t *hit_off, const uint32_t *ops,
                   const int64_t *cigar_off, const char *cs, const int64_t *cs_off, int32_t flags, char *out, int64_t cap) {
    if (!t || n_asm < 0 || !hit_off || !cigar_off || !out_ok(out, cap)) return KP_EINVAL;
    if (n_asm > 0 && (!t->asm_first_ctg || !runs_ok(hit_off, n_asm, hits) || (hit_off[n_asm] > 0 && !hits))) return KP_EINVAL;
    if (flags & ~(KP_PAF_CS | KP_PAF_EQX)) return KP_EINVAL;
    if (flags && !cs_off) return KP_EINVAL;
    const kp_variant_tables tables{t->gene_names, t->gene_name_off, t->n_genes, nullptr, nullptr, t->ctg_names, t->ctg_name_off, t->asm_first_ctg};
    const BatchNames names{&tables};  // (a hit table names no assembly)
    Out o{out, cap};
    for (int a = 0; a < n_asm; ++a) {
        const BatchNames::Window w = names.window(a);
        for (int64_t i = hit_off[a]; i < hit_off[a + 1]; ++i) {
            const kp_hit &h = hits[i];
            if (!names.gene_contig_ok(h, w)) return KP_EINVAL;
            if (cigar_off[i + 1] < cigar_off[i] || (cigar_off[i + 1] > cigar_off[i] && !ops)) return KP_EINVAL;
            if (flags && (cs_off[i + 1] < cs_off[i] || (cs_off[i + 1] > cs_off[i] && !cs))) return KP_EINVAL;
            names.put_gene(o, h.gene); o.put('\t');
            o.num(t->gene_len[h.gene]); o.put('\t');
            o.num(h.q_start); o.put('\t');
            o.num(h.q_end); o.put('\t');
            put_strand(o, h.strand); o.put('\t');
            names.put_contig(o, w, h.contig); o.put('\t');
            o.num(t->ctg_len[w.c0 + h.contig]); o.put('\t');
            o.num(h.t_start); o.put('\t');
            o.num(h.t_end); o.put('\t');
            o.num(h.matches); o.put('\t');
            o.num(h.block_len); o.put('\t');
            o.unum(h.mapq); o.lit("\tAS:i:");
            o.num(h.score); o.lit("\tNM:i:");
            o.num((long long)h.block_len - h.matches); o.lit("\tcg:Z:");
            const char *s = flags ? cs + cs_off[i] : nullptr;
            const int64_t ns = flags ? cs_off[i + 1] - cs_off[i] : 0;
            if (flags && !cs_check(s, ns, ops + cigar_off[i], cigar_off[i + 1] - cigar_off[i], (flags & KP_PAF_EQX) ? &o : nullptr)) return KP_EINVAL;
            if (!(flags & KP_PAF_EQX))
                for (int64_t z = cigar_off[i]; z < cigar_off[i + 1]; ++z) {
                    o.unum(ops[z] >> 4);
                    o.put("MIDNSHP=XB??????"[ops[z] & 15u]);
                }
            if (flags & KP_PAF_CS) { o.lit("\tcs:Z:"); o.put(s, ns); }
            o.put('\n');
        }
    }
    return o.n;
}

}  // namespace

extern "C" int64_t kp_format_paf(const kp_paf_tables *t, int32_t n_asm, const kp_hit *hits, const int64_t *hit_off, const uint32_t *ops,
                                 const int64_t *cigar_off, char *out, int64_t cap) {
    return format_paf(t, n_asm, hits, hit_off, ops, cigar_off, nullptr, nullptr, 0, out, cap);
}

extern "C" int64_t kp_format_paf_tags(const kp_paf_tables *t, int32_t n_asm, const kp_hit *hits, const int64_t *hit_off, const uint32_t *ops,
                                      const int64_t *cigar_off, const char *cs, const int64_t *cs_off, int32_t flags, char *out, int64_t cap) {
    return format_paf(t, n_asm, hits, hit_off, ops, cigar_off, cs, cs_off, flags, out, cap);
}

// ---- variant table (kp_spec.h, VARIANTS) -----------------------------------------------------------------------------------------
// One line per record, straight from the records and the name tables: the streaming command line builds no object per assembly,
// let alone per variant.
extern "C" int64_t kp_format_variants(const kp_variant_tables *t, int32_t n_asm, const kp_kept *kept, int32_t kept_stride, const kp_variant *variants,
                                      const int64_t *var_off, char *out, int64_t cap) {
    const BatchNames names{t};
    if (n_asm < 0 || !out_ok(out, cap) || !names.ok(n_asm) || !runs_ok(var_off, n_asm, kept ? variants : nullptr)) return KP_EINVAL;  // (a record names a kept one)
    static const char letters[] = "acgtn";
    Out o{out, cap};
    for (int a = 0; a < n_asm; ++a) {
        const BatchNames::Window w = names.window(a);
        for (int64_t i = var_off[a]; i < var_off[a + 1]; ++i) {
            const kp_variant &v = variants[i];
            if (v.kept < 0 || v.kept >= kept_stride || v.kind > KP_VAR_DEL) return KP_EINVAL;
            const kp_kept &k = kept[(size_t)a * (size_t)kept_stride + (size_t)v.kept];
            if (!names.gene_contig_ok(k, w)) return KP_EINVAL;
            names.put_asm(o, a); o.put('\t');
            names.put_contig(o, w, k.contig); o.put('\t');
            o.num((long long)v.t_pos + 1); o.put('\t');
            put_strand(o, k.strand); o.put('\t');
            names.put_gene(o, k.gene); o.put('\t');
            o.num((long long)v.q_pos + 1); o.put('\t');
            o.lit(v.kind == KP_VAR_SNV ? "snv" : (v.kind == KP_VAR_INS ? "ins" : "del")); o.put('\t');
            o.num(v.len); o.put('\t');
            if (v.kind == KP_VAR_SNV) {
                o.put(letters[v.ref > 4 ? 4 : v.ref]); o.put('\t');
                o.put(letters[v.alt > 4 ? 4 : v.alt]); o.put('\t');
                o.num((long long)v.q_pos / 3 + 1); o.put('\t');
                o.put((char)v.ref_aa); o.put('\t');
                o.put((char)v.alt_aa); o.put('\t');
                if (v.ref > 3 || v.alt > 3) o.lit("ambiguous");
                else if (v.ref_aa == v.alt_aa) o.lit("synonymous");
                else if (v.alt_aa == '*') o.lit("nonsense");
                else if (v.ref_aa == '*') o.lit("stop_lost");
                else o.lit("missense");
            } else {
                o.lit(".\t.\t.\t.\t.\t");
                o.lit(v.len % 3 != 0 ? "frameshift" : "inframe");
            }
            o.put('\n');
        }
    }
    return o.n;
}

// ---- breakpoint table (kp_spec.h, BREAKPOINTS) -------------------------------------------------------------------------------------
// One line per record; the event's name is derived here, from the record's kind, its two gaps and its two edges.
extern "C" int64_t kp_format_breakpoints(const kp_variant_tables *t, int32_t n_asm, const kp_kept *kept, int32_t kept_stride, const kp_breakpoint *bps,
                                         const int64_t *bp_off, int32_t edge_tolerance, char *out, int64_t cap) {
    const BatchNames names{t};
    if (n_asm < 0 || !out_ok(out, cap) || !names.ok(n_asm) || !runs_ok(bp_off, n_asm, kept ? bps : nullptr)) return KP_EINVAL;  // (a record names two kept ones)
    Out o{out, cap};
    for (int a = 0; a < n_asm; ++a) {
        const BatchNames::Window w = names.window(a);
        for (int64_t i = bp_off[a]; i < bp_off[a + 1]; ++i) {
            const kp_breakpoint &r = bps[i];
            if (r.kept_a < 0 || r.kept_a >= kept_stride || r.kept_b < 0 || r.kept_b >= kept_stride || r.kind > KP_BP_CONTIGS) return KP_EINVAL;
            const kp_kept &ka = kept[(size_t)a * (size_t)kept_stride + (size_t)r.kept_a], &kb = kept[(size_t)a * (size_t)kept_stride + (size_t)r.kept_b];
            if (!names.gene_contig_ok(ka, w) || !names.contig_ok(w, kb.contig)) return KP_EINVAL;
            const char *event;
            if (r.kind == KP_BP_COLLINEAR) event = r.t_gap > 0 ? (r.q_gap > 0 ? "replacement" : "insertion") : (r.q_gap > 0 ? "deletion" : "overlap");
            else if (r.kind == KP_BP_INVERTED) event = "inversion";
            else if (r.kind == KP_BP_DISORDERED) event = "rearrangement";
            else event = (r.edge_a <= edge_tolerance && r.edge_b <= edge_tolerance) ? "contig_break" : "translocation";
            const bool fa = ka.strand >= 0, fb = kb.strand >= 0;
            names.put_asm(o, a); o.put('\t');
            names.put_gene(o, ka.gene); o.put('\t');
            o.lit(event); o.put('\t');
            o.num(ka.q_end); o.put('\t');
            o.num(r.q_gap); o.put('\t');
            names.put_contig(o, w, ka.contig); o.put('\t');
            o.num(fa ? (long long)ka.t_end : (long long)ka.t_start + 1); o.put('\t');  // pos_a + 1
            put_strand(o, ka.strand); o.put('\t');
            names.put_contig(o, w, kb.contig); o.put('\t');
            o.num(fb ? (long long)kb.t_start + 1 : (long long)kb.t_end); o.put('\t');  // pos_b + 1
            put_strand(o, kb.strand); o.put('\t');
            if (r.kind == KP_BP_COLLINEAR) o.num(r.t_gap); else o.put('.');
            o.put('\t');
            o.num(r.q_gap < 0 ? -(long long)r.q_gap : 0); o.put('\t');
            o.num(r.edge_a); o.put('\t');
            o.num(r.edge_b); o.put('\t');
            if (r.ir_cols) { o.num(r.ir_matches); o.put('/'); o.num(r.ir_cols); } else o.put('.');
            o.put('\n');
        }
    }
    return o.n;
}

// ---- allele table (kp_spec.h, ALLELES) -------------------------------------------------------------------------------------------
// One line per kept record the report lists; the locus digest of an assembly is combined here, by kp_alleles.h's one function, from
// the piece digests in the product's order.

extern "C" uint64_t kp_allele_locus_digest(const uint64_t *piece_digests, const int32_t *order, int32_t n) {
    if (n <= 0 || !piece_digests || !order) return 0;
    return kp_al_locus_digest(piece_digests, order, n);
}

extern "C" int64_t kp_format_alleles(const kp_allele_tables *t, int32_t n_asm, const int32_t *n_kept, const int32_t *n_pieces, const int32_t *best_locus,
                                     const kp_kept *kept, const kp_allele *alleles, int32_t kept_stride, const uint64_t *piece_digests,
                                     const int32_t *piece_order, int32_t piece_stride, char *out, int64_t cap) {
    const BatchNames names{t ? &t->names : nullptr};
    if (n_asm < 0 || !out_ok(out, cap) || kept_stride < 0 || piece_stride < 0 || !names.ok(n_asm) || (n_asm > 0 && (!n_kept || !n_pieces || !best_locus || !t->locus_name_off)))
        return KP_EINVAL;
    Out o{out, cap};
    for (int a = 0; a < n_asm; ++a) {
        const int nk = n_kept[a], np = n_pieces[a], best = best_locus[a];
        if (nk < 0 || nk > kept_stride || np < 0 || np > piece_stride || (nk > 0 && (!kept || !alleles)) || (np > 0 && (!piece_digests || !piece_order)))
            return KP_EINVAL;
        if (nk == 0) continue;
        if (best < 0 || best >= t->n_loci) return KP_EINVAL;
        const BatchNames::Window w = names.window(a);
        const int32_t *order = np ? piece_order + (size_t)a * (size_t)piece_stride : nullptr;
        for (int p = 0; p < np; ++p)
            if (order[p] < 0 || order[p] >= np) return KP_EINVAL;
        const uint64_t locus = np ? kp_al_locus_digest(piece_digests + (size_t)a * (size_t)piece_stride, order, np) : 0;
        for (int i = 0; i < nk; ++i) {
            const kp_kept &k = kept[(size_t)a * (size_t)kept_stride + (size_t)i];
            const kp_allele &d = alleles[(size_t)a * (size_t)kept_stride + (size_t)i];
            if (!alive(k)) continue;
            if (!names.gene_contig_ok(k, w) || !state_name(k.state)) return KP_EINVAL;
            names.put_asm(o, a); o.put('\t');
            put_name(o, t->locus_names, t->locus_name_off, best); o.put('\t');
            if (np) put_hex(o, locus); else o.put('.');
            o.put('\t');
            names.put_gene(o, k.gene); o.put('\t');
            o.lit((k.flags & KP_F_EXPECTED) ? "expected" : ((k.flags & KP_F_EXTRA) ? "extra" : "other"));
            o.lit((k.flags & KP_F_INSIDE) ? "_in" : "_out"); o.put('\t');
            names.put_contig(o, w, k.contig); o.put('\t');
            o.num((long long)k.t_start + 1); o.put('\t');
            o.num(k.t_end); o.put('\t');
            put_strand(o, k.strand); o.put('\t');
            o.lit(state_name(k.state)); o.put('\t');  // ("normal" included)
            o.num((long long)k.t_end - k.t_start); o.put('\t');
            put_hex(o, d.nt); o.put('\t');
            o.num(k.prot_len); o.put('\t');
            if (k.prot_len > 0) put_hex(o, d.aa); else o.put('.');
            o.put('\n');
        }
    }
    return o.n;
}

// ---- aligned table (kp_spec.h, ALIGNED ROWS) --------------------------------------------------------------------------------------
// One line per kept record the report lists; the row is unpacked here, sixteen columns a block (put_block_text).
extern "C" int64_t kp_format_aligned(const kp_variant_tables *t, int32_t n_asm, const int32_t *n_kept, const kp_kept *kept, int32_t kept_stride,
                                     const kp_aligned_row *rows, const uint64_t *blocks, int64_t n_blocks, char *out, int64_t cap) {
    const BatchNames names{t};
    if (n_asm < 0 || !out_ok(out, cap) || kept_stride < 0 || n_blocks < 0 || (n_blocks > 0 && !blocks) || !names.ok(n_asm) || (n_asm > 0 && !n_kept)) return KP_EINVAL;
    Out o{out, cap};
    for (int a = 0; a < n_asm; ++a) {
        const int nk = n_kept[a];
        if (nk < 0 || nk > kept_stride || (nk > 0 && (!kept || !rows))) return KP_EINVAL;
        const BatchNames::Window w = names.window(a);
        for (int i = 0; i < nk; ++i) {
            const kp_kept &k = kept[(size_t)a * (size_t)kept_stride + (size_t)i];
            const kp_aligned_row &r = rows[(size_t)a * (size_t)kept_stride + (size_t)i];
            if (!alive(k)) continue;
            if (!names.gene_contig_ok(k, w)) return KP_EINVAL;
            const int64_t nb = r.gene_len < 0 ? -1 : ((int64_t)r.gene_len + 15) / 16;
            if (nb < 0 || r.off < 0 || r.off > n_blocks || nb > n_blocks - r.off) return KP_EINVAL;
            names.put_asm(o, a); o.put('\t');
            names.put_gene(o, k.gene); o.put('\t');
            names.put_contig(o, w, k.contig); o.put('\t');
            o.num((long long)k.t_start + 1); o.put('\t');
            o.num(k.t_end); o.put('\t');
            put_strand(o, k.strand); o.put('\t');
            o.num(r.gene_len); o.put('\t');
            o.num((long long)k.q_start + 1); o.put('\t');
            o.num(k.q_end); o.put('\t');
            o.num(r.covered); o.put('\t');
            o.num(r.inserted); o.put('\t');
            o.num(r.n_ins); o.put('\t');
            for (int64_t j = 0; j < nb; ++j) put_block_text(o, blocks[r.off + j], (int)std::min<int64_t>(16, (int64_t)r.gene_len - 16 * j));
            o.put('\n');
        }
    }
    return o.n;
}

// ---- rescue table (kp_spec.h, RESCUE) ---------------------------------------------------------------------------------------------
// One line per record; the call is derived here, from the record's score, stops, edge and the share of the protein it covers.
extern "C" int64_t kp_format_rescue(const kp_allele_tables *t, int32_t n_asm, const int32_t *prot_len, const int32_t *best_locus, const kp_rescue *recs,
                                    const int64_t *rescue_off, int32_t min_score, char *out, int64_t cap) {
    const BatchNames names{t ? &t->names : nullptr};
    if (n_asm < 0 || !out_ok(out, cap) || !names.ok(n_asm) || !runs_ok(rescue_off, n_asm, recs) || (n_asm > 0 && (!best_locus || !prot_len || !t->locus_name_off))) return KP_EINVAL;
    Out o{out, cap};
    auto fixed2 = [&o](long long num, long long den) {  // "%.2f" of num / den (0 where den is 0)
        char buf[64];
        o.put(buf, std::snprintf(buf, sizeof buf, "%.2f", den > 0 ? (double)num / (double)den : 0.0));
    };
    for (int a = 0; a < n_asm; ++a) {
        if (rescue_off[a + 1] == rescue_off[a]) continue;
        const int best = best_locus[a];
        if (best < 0 || best >= t->n_loci) return KP_EINVAL;
        const BatchNames::Window w = names.window(a);
        for (int64_t i = rescue_off[a]; i < rescue_off[a + 1]; ++i) {
            const kp_rescue &r = recs[i];
            const bool found = r.score > 0;
            if (!names.gene_ok(r.gene) || (found && (!names.contig_ok(w, r.contig) || r.frame > 2))) return KP_EINVAL;
            const long long plen = prot_len[r.gene], span = (long long)r.p_end - r.p_start, cols = (long long)r.matches + r.mismatches + r.gaps;
            const bool short_cov = span * 100 < 90 * plen;
            // (an alignment that reaches the protein's trailing * ends on the gene's own stop: a local path ends on a positive column, and * scores
            // positive against * only.  That stop interrupts nothing.)
            const long long inner_stops = (long long)r.stops - (found && plen > 0 && r.p_end == plen ? 1 : 0);
            const char *call = r.score < min_score ? "absent" : (inner_stops > 0 ? "interrupted" : (short_cov ? (r.edge ? "partial" : "fragment") : "diverged"));
            names.put_asm(o, a); o.put('\t');
            put_name(o, t->locus_names, t->locus_name_off, best); o.put('\t');
            names.put_gene(o, r.gene); o.put('\t');
            o.num(plen); o.put('\t');
            o.lit(call); o.put('\t');
            o.num(r.score); o.put('\t');
            if (found) {
                names.put_contig(o, w, r.contig); o.put('\t');
                o.num((long long)r.t_start + 1); o.put('\t');
                o.num(r.t_end); o.put('\t');
                put_strand(o, r.strand); o.put('\t');
                o.num((long long)r.frame + 1); o.put('\t');
                o.num((long long)r.p_start + 1); o.put('\t');
                o.num(r.p_end); o.put('\t');
            } else {
                o.lit(".\t.\t.\t.\t.\t.\t.\t");
            }
            o.num(r.matches); o.put('\t');
            o.num(r.mismatches); o.put('\t');
            o.num(r.gaps); o.put('\t');
            fixed2((long long)r.matches * 100, cols); o.put('\t');
            fixed2(span * 100, plen); o.put('\t');
            o.num(r.stops); o.put('\t');
            o.lit(!found || !r.edge ? "." : (r.edge == 3 ? "both" : (r.edge == 1 ? "start" : "end")));
            o.put('\n');
        }
    }
    return o.n;
}

// ---- distance table (kp_spec.h, DISTANCES) ----------------------------------------------------------------------------------------
// One line per listed pair of one locus; the rows of the matrix are named by the caller, in the order it stacked them (no mapping).
extern "C" int64_t kp_format_distances(const char *locus_name, int32_t locus_name_len, int64_t columns, const char *names, const int64_t *name_off,
                                       int32_t n_names, const kp_dist_pair *pairs, int64_t n_pairs, char *out, int64_t cap) {
    if (!locus_and_out_ok(locus_name, locus_name_len, out, cap) || columns < 0 || n_names < 0 || n_pairs < 0) return KP_EINVAL;
    if (n_pairs > 0 && (!pairs || !name_off || n_names == 0)) return KP_EINVAL;
    const RowNames t{names, name_off, n_names, nullptr};
    Out o{out, cap};
    for (int64_t i = 0; i < n_pairs; ++i) {
        const kp_dist_pair &r = pairs[i];
        if (!t.valid(r.a) || !t.valid(r.b)) return KP_EINVAL;  // (only the rows a pair names are looked at)
        put_locus(o, locus_name, locus_name_len); o.put('\t');
        t.put(o, r.a); o.put('\t');
        t.put(o, r.b); o.put('\t');
        o.num(columns); o.put('\t');
        o.num(r.compared); o.put('\t');
        o.num(r.differences); o.put('\t');
        o.num(r.unshared);
        o.put('\n');
    }
    return o.n;
}

// ---- cluster table (kp_spec.h, CLUSTERS) --------------------------------------------------------------------------------------------
// One line per row of one locus's matrix, in row order: its cluster number at every level (kp_clust_numbers), then its nearest row.
extern "C" int64_t kp_format_clusters(const char *locus_name, int32_t locus_name_len, const char *names, const int64_t *name_off, int32_t n_names,
                                      const int32_t *rows, int32_t n_levels, const int32_t *labels, const kp_dist_nearest *nearest, char *out, int64_t cap) {
    const RowNames t{names, name_off, n_names, rows};
    if (!locus_and_out_ok(locus_name, locus_name_len, out, cap) || !t.valid() || n_levels < 0 || n_levels > KP_CLUST_MAX_LEVELS) return KP_EINVAL;
    if (n_names > 0 && (!nearest || (n_levels > 0 && !labels))) return KP_EINVAL;
    for (int32_t r = 0; r < n_names; ++r)
        if (nearest[r].row < -1 || nearest[r].row >= n_names) return KP_EINVAL;
    std::vector<int32_t> number((size_t)n_levels * (size_t)n_names), rank((size_t)n_names);
    for (int32_t k = 0; k < n_levels; ++k)
        if (!kp_clust_numbers(labels + (size_t)k * (size_t)n_names, n_names, rank.data(), number.data() + (size_t)k * (size_t)n_names)) return KP_EINVAL;
    Out o{out, cap};
    for (int32_t r = 0; r < n_names; ++r) {
        const kp_dist_nearest &nr = nearest[r];
        put_locus(o, locus_name, locus_name_len); o.put('\t');
        t.put(o, r); o.put('\t');
        for (int32_t k = 0; k < n_levels; ++k) { o.num(number[(size_t)k * (size_t)n_names + (size_t)r]); o.put('\t'); }
        if (nr.row >= 0) {
            t.put(o, nr.row); o.put('\t');
            o.num(nr.differences); o.put('\t');
            o.num(nr.compared); o.put('\t');
            o.num(nr.unshared);
        } else {
            o.lit(".\t.\t.\t.");
        }
        o.put('\n');
    }
    return o.n;
}

// ---- Newick table (kp_spec.h, TREE) ---------------------------------------------------------------------------------------------------
// A Newick label: bare when every byte is one of A-Za-z0-9_.- ; otherwise in single quotes with every ' doubled.
static void put_newick_name(Out &o, const char *s, int64_t n) {
    bool bare = true;
    for (int64_t i = 0; i < n && bare; ++i) {
        const unsigned char c = (unsigned char)s[i];
        bare = (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || (c >= '0' && c <= '9') || c == '_' || c == '.' || c == '-';
    }
    if (bare) { o.put(s, n); return; }
    o.put('\'');
    for (int64_t i = 0; i < n; ++i) {
        if (s[i] == '\'') o.put('\'');
        o.put(s[i]);
    }
    o.put('\'');
}

// One line per tree of one locus's forest, ascending in the component's label: every tree rooted at its smallest row, a node's
// children ascending by (differences, row), written with a stack of its own -- a chain of 2^18 rows is a legal tree.
extern "C" int64_t kp_format_newick(const char *locus_name, int32_t locus_name_len, const char *names, const int64_t *name_off, int32_t n_names,
                                    const int32_t *rows, const kp_dist_pair *edges, int64_t n_edges, const int32_t *component, char *out, int64_t cap) {
    const RowNames t{names, name_off, n_names, rows};
    if (!locus_and_out_ok(locus_name, locus_name_len, out, cap) || !t.valid() || n_edges < 0) return KP_EINVAL;
    if (n_names > 0 && !component) return KP_EINVAL;
    if (n_edges > 0 && !edges) return KP_EINVAL;
    const int32_t R = n_names;
    // the edges must be a forest over the rows, and component[] the smallest row of every row's tree
    std::vector<int32_t> parent((size_t)R);
    for (int32_t r = 0; r < R; ++r) parent[(size_t)r] = r;
    std::vector<int64_t> first((size_t)R + 1, 0);
    for (int64_t e = 0; e < n_edges; ++e) {
        const kp_dist_pair &p = edges[e];
        if (p.a < 0 || p.b >= R || p.a >= p.b) return KP_EINVAL;
        if (!kp_clust_unite(parent.data(), p.a, p.b)) return KP_EINVAL;  // (closes a cycle)
        ++first[(size_t)p.a + 1]; ++first[(size_t)p.b + 1];
    }
    std::vector<int32_t> size((size_t)R, 0);
    for (int32_t r = 0; r < R; ++r) {
        if (component[r] != kp_clust_find(parent.data(), r)) return KP_EINVAL;  // (the larger root went under the smaller: a root is its tree's smallest row)
        ++size[(size_t)component[r]];
    }
    // neighbours of every row, ascending by (differences, row)
    struct Nb { int32_t differences, row; };
    for (int32_t r = 0; r < R; ++r) first[(size_t)r + 1] += first[(size_t)r];
    std::vector<Nb> nb((size_t)(2 * n_edges));
    {
        std::vector<int64_t> at(first.begin(), first.end() - 1);
        for (int64_t e = 0; e < n_edges; ++e) {
            const kp_dist_pair &p = edges[e];
            nb[(size_t)at[(size_t)p.a]++] = Nb{p.differences, p.b};
            nb[(size_t)at[(size_t)p.b]++] = Nb{p.differences, p.a};
        }
    }
    for (int32_t r = 0; r < R; ++r)
        std::sort(nb.begin() + first[(size_t)r], nb.begin() + first[(size_t)r + 1],
                  [](const Nb &x, const Nb &y) { return x.differences != y.differences ? x.differences < y.differences : x.row < y.row; });
    Out o{out, cap};
    struct Frame { int32_t row, from, length; int64_t next; bool open; };  // from: the row it was reached from; length: that edge's differences
    std::vector<Frame> stack;
    long long tree = 0;
    for (int32_t root = 0; root < R; ++root) {
        if (component[root] != root) continue;
        put_locus(o, locus_name, locus_name_len); o.put('\t');
        o.num(++tree); o.put('\t');
        o.num(size[(size_t)root]); o.put('\t');
        stack.push_back(Frame{root, -1, 0, first[(size_t)root], false});
        while (!stack.empty()) {
            Frame &f = stack.back();
            if (f.next < first[(size_t)f.row + 1] && nb[(size_t)f.next].row == f.from) ++f.next;  // (a forest: the way back is one neighbour)
            if (f.next < first[(size_t)f.row + 1]) {
                const Nb child = nb[(size_t)f.next++];
                o.put(f.open ? ',' : '(');
                f.open = true;
                const int32_t here = f.row;
                stack.push_back(Frame{child.row, here, child.differences, first[(size_t)child.row], false});  // (f is dead from here on)
                continue;
            }
            if (f.open) o.put(')');
            const int32_t at = t.at(f.row);
            put_newick_name(o, names + name_off[at], name_off[at + 1] - name_off[at]);
            const bool is_root = f.from < 0;
            const int32_t length = f.length;
            stack.pop_back();
            if (!is_root) { o.put(':'); o.num(length); }
        }
        o.lit(";\n");
    }
    return o.n;
}

// ---- neighbour-joining table (kp_spec.h, NJ) -------------------------------------------------------------------------------------------
// One line for one locus's tree, none for fewer than two taxa: the unrooted tree written from its last record, inner nodes unnamed,
// lengths with %.9g, with a stack of its own -- a caterpillar of 16384 taxa is a legal tree.
// With `support` (kp_spec.h, BOOTSTRAP) the line has the Replicates column, and the node of a record with an inner edge its label.
// With `transfer` (kp_spec.h, TRANSFER) instead, the label is the transfer support in thousandths, three decimals.
static int64_t format_nj_line(const char *locus_name, int32_t locus_name_len, const char *names, const int64_t *name_off, int32_t n_names, const int32_t *rows,
                              const int32_t *taxa, int32_t n_taxa, const kp_nj_node *nodes, int64_t n_nodes, const int32_t *support, const int64_t *transfer,
                              int32_t replicates, char *out, int64_t cap) {
    const RowNames t{names, name_off, n_names, rows};
    if (!locus_and_out_ok(locus_name, locus_name_len, out, cap) || !t.valid() || n_taxa < 0 || n_taxa > n_names || n_nodes < 0) return KP_EINVAL;
    if ((n_taxa > 0 && !taxa) || (n_nodes > 0 && !nodes)) return KP_EINVAL;
    const int64_t n = n_taxa;
    if (n_nodes != kp_nj_records(n)) return KP_EINVAL;
    for (int64_t k = 0; k < n; ++k)
        if (taxa[k] < 0 || taxa[k] >= n_names || (k > 0 && taxa[k] <= taxa[k - 1])) return KP_EINVAL;
    // record r makes node n + r out of nodes made before it, and no node is a child twice: a tree, and no cycle
    std::vector<char> used((size_t)(n + n_nodes), 0);
    for (int64_t r = 0; r < n_nodes; ++r) {
        const kp_nj_node &p = nodes[r];
        const bool last = r == n_nodes - 1, three = last && n > 2;
        const int32_t child[3] = {p.a, p.b, p.c};
        if (!three && p.c != -1) return KP_EINVAL;
        for (int k = 0; k < (three ? 3 : 2); ++k) {
            if (child[k] < 0 || child[k] >= n + r || used[(size_t)child[k]]) return KP_EINVAL;
            used[(size_t)child[k]] = 1;
        }
    }
    const int64_t labelled = kp_boot_splits(n);  // records whose node has an inner edge above it
    if (support)
        for (int64_t r = 0; r < n_nodes; ++r)
            if (r < labelled ? (support[r] < 0 || support[r] > replicates) : support[r] != -1) return KP_EINVAL;
    std::vector<int32_t> depth;  // of every record with an inner edge: the light side of its split
    if (transfer) {
        depth.resize((size_t)labelled);
        kp_transfer_sizes(nodes, (int32_t)n, depth.data());
        for (int64_t r = 0; r < labelled; ++r) depth[(size_t)r] = kp_transfer_depth(depth[(size_t)r], (int32_t)n);
        for (int64_t r = 0; r < n_nodes; ++r)
            if (r < labelled ? (transfer[r] < 0 || transfer[r] > (int64_t)replicates * (depth[(size_t)r] - 1)) : transfer[r] != -1) return KP_EINVAL;
    }
    Out o{out, cap};
    if (n_nodes == 0) return 0;
    put_locus(o, locus_name, locus_name_len); o.put('\t');
    o.num(n_names); o.put('\t');
    o.num(n); o.put('\t');
    if (support || transfer) { o.num(replicates); o.put('\t'); }
    const auto put_length = [&o](double v) {
        char buf[40];
        o.put(':');
        o.put(buf, std::snprintf(buf, sizeof buf, "%.9g", v));
    };
    struct Frame { int64_t rec; int next; };  // the record of an open inner node, and which of its children comes next
    std::vector<Frame> stack;
    stack.push_back(Frame{n_nodes - 1, 0});
    o.put('(');
    while (!stack.empty()) {
        const Frame f = stack.back();
        const kp_nj_node &p = nodes[f.rec];
        if (f.next == (p.c >= 0 ? 3 : 2)) {  // closed: its own length follows, unless it is the tree
            o.put(')');
            stack.pop_back();
            if (support && f.rec < labelled) o.num(support[f.rec]);
            if (transfer && f.rec < labelled) {
                char buf[16];
                const int64_t K = kp_transfer_label(transfer[f.rec], replicates, depth[(size_t)f.rec]);
                o.put(buf, std::snprintf(buf, sizeof buf, "%d.%03d", (int)(K / 1000), (int)(K % 1000)));
            }
            if (!stack.empty()) {
                const Frame &up = stack.back();
                const kp_nj_node &q = nodes[up.rec];
                put_length(up.next == 1 ? q.la : (up.next == 2 ? q.lb : q.lc));
            }
            continue;
        }
        if (f.next > 0) o.put(',');
        const int32_t id = f.next == 0 ? p.a : (f.next == 1 ? p.b : p.c);
        ++stack.back().next;
        if (id < n) {
            const int32_t at = t.at(taxa[id]);
            put_newick_name(o, names + name_off[at], name_off[at + 1] - name_off[at]);
            put_length(f.next == 0 ? p.la : (f.next == 1 ? p.lb : p.lc));
        } else {
            o.put('(');
            stack.push_back(Frame{(int64_t)id - n, 0});
        }
    }
    o.lit(";\n");
    return o.n;
}
extern "C" int64_t kp_format_nj(const char *locus_name, int32_t locus_name_len, const char *names, const int64_t *name_off, int32_t n_names,
                                const int32_t *rows, const int32_t *taxa, int32_t n_taxa, const kp_nj_node *nodes, int64_t n_nodes, char *out, int64_t cap) {
    return format_nj_line(locus_name, locus_name_len, names, name_off, n_names, rows, taxa, n_taxa, nodes, n_nodes, nullptr, nullptr, 0, out, cap);
}
extern "C" int64_t kp_format_nj_support(const char *locus_name, int32_t locus_name_len, const char *names, const int64_t *name_off, int32_t n_names,
                                        const int32_t *rows, const int32_t *taxa, int32_t n_taxa, const kp_nj_node *nodes, int64_t n_nodes, const int32_t *support,
                                        int32_t replicates, char *out, int64_t cap) {
    if (replicates < 1 || replicates > KP_BOOT_MAX_REPLICATES || (n_nodes > 0 && !support)) return KP_EINVAL;
    static const int32_t none = -1;  // (no record: the shared body still writes the five-column form of nothing)
    return format_nj_line(locus_name, locus_name_len, names, name_off, n_names, rows, taxa, n_taxa, nodes, n_nodes, support ? support : &none, nullptr, replicates, out, cap);
}
extern "C" int64_t kp_format_nj_transfer(const char *locus_name, int32_t locus_name_len, const char *names, const int64_t *name_off, int32_t n_names,
                                         const int32_t *rows, const int32_t *taxa, int32_t n_taxa, const kp_nj_node *nodes, int64_t n_nodes, const int64_t *transfer,
                                         int32_t replicates, char *out, int64_t cap) {
    if (replicates < 1 || replicates > KP_BOOT_MAX_REPLICATES || (n_nodes > 0 && !transfer)) return KP_EINVAL;
    static const int64_t none = -1;  // (no record: as above)
    return format_nj_line(locus_name, locus_name_len, names, name_off, n_names, rows, taxa, n_taxa, nodes, n_nodes, nullptr, transfer ? transfer : &none, replicates, out, cap);
}

// ---- site table (kp_spec.h, SITES) ---------------------------------------------------------------------------------------------------
// One line per site of one locus, in the sites' order; the genes of the locus are named by the caller (RowNames: a gene per "row").
extern "C" int64_t kp_format_sites(const char *locus_name, int32_t locus_name_len, const char *gene_names, const int64_t *gene_name_off, int32_t n_genes,
                                   const int32_t *genes, const int32_t *gene_len, int32_t n_rows, const kp_site *sites, int64_t n_sites, char *out, int64_t cap) {
    const RowNames t{gene_names, gene_name_off, n_genes, genes};
    if (!locus_and_out_ok(locus_name, locus_name_len, out, cap) || !t.valid() || n_rows < 0 || n_sites < 0) return KP_EINVAL;
    if ((n_genes > 0 && !gene_len) || (n_sites > 0 && !sites)) return KP_EINVAL;
    std::vector<int64_t> blocks((size_t)n_genes), before((size_t)n_genes);  // every gene's blocks, and the real columns of the genes before it
    int64_t real = 0;
    for (int32_t g = 0; g < n_genes; ++g) {
        if (gene_len[g] < 0) return KP_EINVAL;
        blocks[(size_t)g] = ((int64_t)gene_len[g] + 15) / 16;
        before[(size_t)g] = real;
        real += gene_len[g];
    }
    Out o{out, cap};
    for (int64_t i = 0; i < n_sites; ++i) {
        const kp_site &s = sites[i];
        int64_t pos = 0;
        const int32_t g = kp_site_gene(blocks.data(), n_genes, s.column, &pos);
        if (g < 0 || pos >= gene_len[g]) return KP_EINVAL;  // outside the matrix, or padding
        if (i > 0 && s.column <= sites[i - 1].column) return KP_EINVAL;
        int64_t held = s.n_n;
        for (int k = 0; k < 4; ++k) {
            if (s.n[k] < 0) return KP_EINVAL;
            held += s.n[k];
        }
        if (s.n_n < 0 || held > n_rows || kp_site_alleles(s.n) < 2) return KP_EINVAL;
        put_locus(o, locus_name, locus_name_len); o.put('\t');
        t.put(o, g); o.put('\t');
        o.num(pos + 1); o.put('\t');
        o.num(before[(size_t)g] + pos + 1); o.put('\t');
        o.num(n_rows); o.put('\t');
        for (int k = 0; k < 4; ++k) { o.num(s.n[k]); o.put('\t'); }
        o.num(s.n_n); o.put('\t');
        o.num(kp_site_gap(s.n, s.n_n, n_rows)); o.put('\t');
        o.num(kp_site_alleles(s.n)); o.put('\t');
        o.put("acgt"[kp_site_major(s.n)]); o.put('\t');
        o.lit(kp_site_informative(s.n) ? "yes" : "no");
        o.put('\n');
    }
    return o.n;
}

// ---- SNP alignment (kp_spec.h, SITES, SITE ROWS) ------------------------------------------------------------------------------------------
// One line per row of one locus's matrix, in row order: its codes at the locus's sites as text.
extern "C" int64_t kp_format_site_rows(const char *locus_name, int32_t locus_name_len, const char *names, const int64_t *name_off, int32_t n_names,
                                       const int32_t *rows, int64_t n_sites, const uint64_t *blocks, char *out, int64_t cap) {
    const RowNames t{names, name_off, n_names, rows};
    if (!locus_and_out_ok(locus_name, locus_name_len, out, cap) || !t.valid() || n_sites < 0) return KP_EINVAL;
    const int64_t SB = kp_site_row_blocks(n_sites);
    if (n_names > 0 && SB > 0 && !blocks) return KP_EINVAL;
    Out o{out, cap};
    if (n_sites == 0) return 0;  // a locus without a site writes no line
    for (int32_t r = 0; r < n_names; ++r) {
        put_locus(o, locus_name, locus_name_len); o.put('\t');
        t.put(o, r); o.put('\t');
        o.num(n_sites); o.put('\t');
        for (int64_t b = 0; b < SB; ++b) {
            const uint64_t v = blocks[(size_t)r * (size_t)SB + (size_t)b];
            const uint64_t pad = b == SB - 1 ? kp_dist_pad_mask(n_sites) : 0ull;  // (padding is flagged as gap)
            if (((v >> KP_DIST_N_SHIFT) & (v >> KP_DIST_GAP_SHIFT) & 0xffffu) || (v & pad) != pad) return KP_EINVAL;  // (N and gap never both)
            put_block_text(o, v, (int)std::min<int64_t>(KP_SITES_BLOCK, n_sites - b * KP_SITES_BLOCK));
        }
        o.put('\n');
    }
    return o.n;
}

// ---- parsimony tables (kp_spec.h, PARSIMONY) ---------------------------------------------------------------------------------------------
namespace {
// The genes of one locus as the site table has them: a column of the matrix -> its gene, its position there and its column among the
// real columns; false for a column outside the matrix or in padding.
struct GeneColumns {
    RowNames t;
    const int32_t *gene_len;
    std::vector<int64_t> blocks, before;
    bool valid() {
        if (!t.valid() || (t.n > 0 && !gene_len)) return false;
        blocks.resize((size_t)t.n); before.resize((size_t)t.n);
        int64_t real = 0;
        for (int32_t g = 0; g < t.n; ++g) {
            if (gene_len[g] < 0) return false;
            blocks[(size_t)g] = ((int64_t)gene_len[g] + 15) / 16;
            before[(size_t)g] = real;
            real += gene_len[g];
        }
        return true;
    }
    bool put(Out &o, int64_t column) const {  // Gene, Position, Column
        int64_t pos = 0;
        const int32_t g = kp_site_gene(blocks.data(), t.n, column, &pos);
        if (g < 0 || pos >= gene_len[g]) return false;
        t.put(o, g); o.put('\t');
        o.num(pos + 1); o.put('\t');
        o.num(before[(size_t)g] + pos + 1);
        return true;
    }
};
}  // namespace

// One line per column the tree needs a step for, in the records' order.
extern "C" int64_t kp_format_nj_homoplasy(const char *locus_name, int32_t locus_name_len, const char *gene_names, const int64_t *gene_name_off, int32_t n_genes,
                                          const int32_t *genes, const int32_t *gene_len, const kp_pars_site *sites, int64_t n_sites, char *out, int64_t cap) {
    GeneColumns gc{RowNames{gene_names, gene_name_off, n_genes, genes}, gene_len, {}, {}};
    if (!locus_and_out_ok(locus_name, locus_name_len, out, cap) || !gc.valid() || n_sites < 0 || (n_sites > 0 && !sites)) return KP_EINVAL;
    Out o{out, cap};
    for (int64_t i = 0; i < n_sites; ++i) {
        const kp_pars_site &s = sites[i];
        const int32_t held = kp_pars_allele_count(s.alleles);
        if ((s.alleles & ~15) || held < 2 || s.steps < held - 1) return KP_EINVAL;  // (a column of one base has no step)
        if (i > 0 && s.column <= sites[i - 1].column) return KP_EINVAL;
        put_locus(o, locus_name, locus_name_len); o.put('\t');
        if (!gc.put(o, s.column)) return KP_EINVAL;
        o.put('\t');
        o.num(held); o.put('\t');
        o.num(s.steps); o.put('\t');
        o.num(s.steps - (held - 1));
        o.put('\n');
    }
    return o.n;
}

// One line per change, in the records' order.  What lies below every node -- its lowest taxon, the number of its taxa -- is made in
// one pass over the records, children before parents: no recursion.
extern "C" int64_t kp_format_nj_changes(const char *locus_name, int32_t locus_name_len, const char *names, const int64_t *name_off, int32_t n_names, const int32_t *rows,
                                        const int32_t *taxa, int32_t n_taxa, const kp_nj_node *nodes, int64_t n_nodes, const char *gene_names, const int64_t *gene_name_off,
                                        int32_t n_genes, const int32_t *genes, const int32_t *gene_len, const kp_pars_change *changes, int64_t n_changes, char *out, int64_t cap) {
    const RowNames t{names, name_off, n_names, rows};
    GeneColumns gc{RowNames{gene_names, gene_name_off, n_genes, genes}, gene_len, {}, {}};
    if (!locus_and_out_ok(locus_name, locus_name_len, out, cap) || !t.valid() || !gc.valid() || n_taxa < 0 || n_taxa > n_names || n_nodes < 0 || n_changes < 0) return KP_EINVAL;
    if ((n_taxa > 0 && !taxa) || (n_nodes > 0 && !nodes) || (n_changes > 0 && !changes)) return KP_EINVAL;
    const int64_t n = n_taxa, all = n + n_nodes;
    for (int64_t k = 0; k < n; ++k)
        if (taxa[k] < 0 || taxa[k] >= n_names || (k > 0 && taxa[k] <= taxa[k - 1])) return KP_EINVAL;
    std::vector<int32_t> up((size_t)all), low((size_t)all), tips((size_t)all);
    if (!kp_pars_tree_ok(nodes, n_nodes, n_taxa, up.data())) return KP_EINVAL;
    for (int64_t k = 0; k < n; ++k) { low[(size_t)k] = (int32_t)k; tips[(size_t)k] = 1; }
    for (int64_t r = 0; r < n_nodes; ++r) {
        int32_t least = INT32_MAX, sum = 0;
        for (int k = 0; k < kp_pars_children(nodes[r]); ++k) {
            const int32_t id = kp_pars_child_id(nodes[r], k);
            least = std::min(least, low[(size_t)id]);
            sum += tips[(size_t)id];
        }
        low[(size_t)(n + r)] = least; tips[(size_t)(n + r)] = sum;
    }
    Out o{out, cap};
    const auto name = [&](int32_t k) {
        const int32_t at = t.at(taxa[k]);
        put_newick_name(o, names + name_off[at], name_off[at + 1] - name_off[at]);
    };
    for (int64_t i = 0; i < n_changes; ++i) {
        const kp_pars_change &c = changes[i];
        if (c.node < 0 || c.node >= all - 1 || c.parent != up[(size_t)c.node] || c.from > 3 || c.to > 3 || c.from == c.to) return KP_EINVAL;
        if (i > 0 && (c.node < changes[i - 1].node || (c.node == changes[i - 1].node && c.column <= changes[i - 1].column))) return KP_EINVAL;
        put_locus(o, locus_name, locus_name_len); o.put('\t');
        if (c.node < n) {
            name(c.node); o.put('\t');
            name(c.node); o.lit("\t.\t");
        } else {
            const kp_nj_node &p = nodes[c.node - n];
            o.put('#'); o.num(c.node - n + 1); o.put('\t');
            name(low[(size_t)p.a]); o.put('\t');
            name(low[(size_t)p.b]); o.put('\t');
        }
        o.num(tips[(size_t)c.node]); o.put('\t');
        if (!gc.put(o, c.column)) return KP_EINVAL;
        o.put('\t');
        o.put("acgt"[c.from]); o.put('\t');
        o.put("acgt"[c.to]);
        o.put('\n');
    }
    return o.n;
}
