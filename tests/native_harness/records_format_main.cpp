// records_format_main.cpp -- a stand-alone program around kp_format_variants, kp_format_breakpoints, kp_format_rescue, kp_format_paf and
// kp_format_paf_tags, for a run under the host sanitizers (no GPU, nothing loaded into an interpreter):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -o records_format_main
//       tests/native_harness/records_format_main.cpp kaptive_amd/csrc/kp_rows.cpp && ./records_format_main
// Every table is a heap block of exactly the size the call may read or write: an access past an end stops the program.  One batch of
// two assemblies, three contigs and three genes with a kept stride of 2; every formatter writes its good table (compared with a
// literal; sized with cap 0, then written into a buffer of exactly that size) and refuses each malformed input with KP_EINVAL: a null
// name-offset table, offsets that descend within a run, offsets whose end lies below their start, a kept index equal to the stride, a
// contig equal to its window's size, a gene equal to n_genes and, for PAF with flags, a cs string that does not fit its ops.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/kaptive_amd.h"

template <class T>
struct Exact {  // a heap block of exactly n items (std::vector may round its capacity up)
    T *p;
    size_t n;
    explicit Exact(const std::vector<T> &v) : p((T *)std::malloc(v.size() * sizeof(T) + (v.empty() ? 1 : 0))), n(v.size()) {
        if (!v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T));
    }
    ~Exact() { std::free(p); }
    Exact(const Exact &) = delete;
};
static std::vector<char> chars(const std::string &s) { return std::vector<char>(s.begin(), s.end()); }

static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #x); ++fails; } } while (0)

using Call = std::function<int64_t(char *, int64_t)>;
// the sizing call and the call into a buffer of exactly that size return the same size, and the bytes are `want`
static void good(const char *what, const Call &call, const std::string &want) {
    const int64_t need = call(nullptr, 0);
    if (need != (int64_t)want.size()) { std::fprintf(stderr, "%s: size %lld, expected %zu\n", what, (long long)need, want.size()); ++fails; return; }
    Exact<char> out(std::vector<char>((size_t)need, '#'));
    const int64_t again = call(out.p, need);
    if (again != need || std::memcmp(out.p, want.data(), (size_t)need) != 0) {
        std::fprintf(stderr, "%s: wrote (%lld)\n%.*s", what, (long long)again, (int)need, out.p);
        ++fails;
    }
    if (need > 1) {  // a buffer one byte short: the count is the same, nothing is written past it
        Exact<char> shorter(std::vector<char>((size_t)need - 1, '#'));
        CHECK(call(shorter.p, need - 1) == need);
    }
}
#define REFUSED(call) CHECK((call) == KP_EINVAL)

int main() {
    const int n_asm = 2, stride = 2, n_genes = 3;
    Exact<char> gene_b(chars("g0gene1g2")), asm_b(chars("a0asm1")), ctg_b(chars("c0ctg1c2")), locus_b(chars("L0KL2"));
    Exact<int32_t> gene_off({0, 2, 7, 9}), locus_off({0, 2, 5});
    Exact<int64_t> asm_off({0, 2, 6}), ctg_off({0, 2, 6, 8}), first({0, 2, 3});  // assembly 0: c0, ctg1; assembly 1: c2
    kp_variant_tables t{};
    t.gene_names = gene_b.p; t.gene_name_off = gene_off.p; t.n_genes = n_genes;
    t.asm_names = asm_b.p; t.asm_name_off = asm_off.p; t.ctg_names = ctg_b.p; t.ctg_name_off = ctg_off.p; t.asm_first_ctg = first.p;
    kp_variant_tables no_names = t;
    no_names.asm_name_off = nullptr;
    Exact<int64_t> descending({0, 2, 1}), end_below_start({2, 2, 1});  // (offsets of n_asm + 1 entries, for tables of two or three records)

    std::vector<kp_kept> kept((size_t)n_asm * stride);
    std::memset(kept.data(), 0, kept.size() * sizeof(kp_kept));
    auto keep = [&](int a, int i, int gene, int contig, int q0, int q1, int t0, int t1, int strand) {
        kp_kept &k = kept[(size_t)a * stride + i];
        k.gene = gene; k.contig = contig; k.q_start = q0; k.q_end = q1; k.t_start = t0; k.t_end = t1; k.strand = (int8_t)strand;
    };
    keep(0, 0, 0, 1, 0, 30, 100, 130, 1);
    keep(0, 1, 0, 0, 30, 60, 500, 530, -1);
    keep(1, 0, 2, 0, 5, 25, 10, 30, -1);
    keep(1, 1, 2, 0, 20, 50, 200, 230, -1);
    Exact<kp_kept> kept_b(kept);
    // the same table with one record's gene or contig outside the name tables
    auto kept_with = [&](int a, int i, int gene, int contig) {
        std::vector<kp_kept> k2 = kept;
        k2[(size_t)a * stride + i].gene = gene; k2[(size_t)a * stride + i].contig = contig;
        return k2;
    };
    Exact<kp_kept> kept_gene(kept_with(0, 1, n_genes, 0)), kept_ctg0(kept_with(0, 0, 0, 2)), kept_ctg1(kept_with(1, 0, 2, 1)), kept_ctg_b(kept_with(0, 1, 0, 2));

    // ---- variants
    {
        std::vector<kp_variant> v(3);
        std::memset(v.data(), 0, v.size() * sizeof(kp_variant));
        v[0].kept = 0; v[0].q_pos = 6; v[0].t_pos = 106; v[0].len = 1; v[0].kind = KP_VAR_SNV; v[0].ref = 0; v[0].alt = 2; v[0].ref_aa = 'K'; v[0].alt_aa = 'R';
        v[1].kept = 1; v[1].q_pos = 40; v[1].t_pos = 510; v[1].len = 4; v[1].kind = KP_VAR_INS;
        v[2].kept = 0; v[2].q_pos = 9; v[2].t_pos = 20; v[2].len = 3; v[2].kind = KP_VAR_DEL;
        Exact<kp_variant> recs(v);
        Exact<int64_t> off({0, 2, 3});
        good("variants", [&](char *out, int64_t cap) { return kp_format_variants(&t, n_asm, kept_b.p, stride, recs.p, off.p, out, cap); },
             "a0\tctg1\t107\t+\tg0\t7\tsnv\t1\ta\tg\t3\tK\tR\tmissense\n"
             "a0\tc0\t511\t-\tg0\t41\tins\t4\t.\t.\t.\t.\t.\tframeshift\n"
             "asm1\tc2\t21\t-\tg2\t10\tdel\t3\t.\t.\t.\t.\t.\tinframe\n");
        REFUSED(kp_format_variants(&no_names, n_asm, kept_b.p, stride, recs.p, off.p, nullptr, 0));
        REFUSED(kp_format_variants(&t, n_asm, kept_b.p, stride, recs.p, descending.p, nullptr, 0));
        REFUSED(kp_format_variants(&t, n_asm, kept_b.p, stride, recs.p, end_below_start.p, nullptr, 0));
        { std::vector<kp_variant> b = v; b[1].kept = stride; Exact<kp_variant> bad(b); REFUSED(kp_format_variants(&t, n_asm, kept_b.p, stride, bad.p, off.p, nullptr, 0)); }
        REFUSED(kp_format_variants(&t, n_asm, kept_ctg0.p, stride, recs.p, off.p, nullptr, 0));
        REFUSED(kp_format_variants(&t, n_asm, kept_ctg1.p, stride, recs.p, off.p, nullptr, 0));
        REFUSED(kp_format_variants(&t, n_asm, kept_gene.p, stride, recs.p, off.p, nullptr, 0));
        REFUSED(kp_format_variants(&t, n_asm, nullptr, stride, recs.p, off.p, nullptr, 0));  // records without the kept table they name
        CHECK(kp_format_variants(&t, 0, nullptr, 0, nullptr, nullptr, nullptr, 0) == 0);
    }
    // ---- breakpoints
    {
        std::vector<kp_breakpoint> v(2);
        std::memset(v.data(), 0, v.size() * sizeof(kp_breakpoint));
        v[0].kept_a = 0; v[0].kept_b = 1; v[0].edge_a = 3; v[0].edge_b = 7; v[0].kind = KP_BP_CONTIGS;
        v[1].kept_a = 0; v[1].kept_b = 1; v[1].q_gap = -5; v[1].t_gap = 12; v[1].edge_a = 100; v[1].edge_b = 200; v[1].kind = KP_BP_COLLINEAR; v[1].ir_cols = 20; v[1].ir_matches = 18;
        Exact<kp_breakpoint> recs(v);
        Exact<int64_t> off({0, 1, 2}), off3({0, 2, 3});
        good("breakpoints", [&](char *out, int64_t cap) { return kp_format_breakpoints(&t, n_asm, kept_b.p, stride, recs.p, off.p, 5, out, cap); },
             "a0\tg0\ttranslocation\t30\t0\tctg1\t130\t+\tc0\t530\t-\t.\t0\t3\t7\t.\n"
             "asm1\tg2\tinsertion\t25\t-5\tc2\t11\t-\tc2\t230\t-\t12\t5\t100\t200\t18/20\n");
        REFUSED(kp_format_breakpoints(&no_names, n_asm, kept_b.p, stride, recs.p, off.p, 5, nullptr, 0));
        { std::vector<kp_breakpoint> b{v[0], v[0], v[1]}; Exact<kp_breakpoint> three(b);  // (three records, so that the offsets above stay inside them)
          CHECK(kp_format_breakpoints(&t, n_asm, kept_b.p, stride, three.p, off3.p, 5, nullptr, 0) > 0);
          REFUSED(kp_format_breakpoints(&t, n_asm, kept_b.p, stride, three.p, descending.p, 5, nullptr, 0));
          REFUSED(kp_format_breakpoints(&t, n_asm, kept_b.p, stride, three.p, end_below_start.p, 5, nullptr, 0)); }
        { std::vector<kp_breakpoint> b = v; b[0].kept_b = stride; Exact<kp_breakpoint> bad(b); REFUSED(kp_format_breakpoints(&t, n_asm, kept_b.p, stride, bad.p, off.p, 5, nullptr, 0)); }
        { std::vector<kp_breakpoint> b = v; b[1].kept_a = stride; Exact<kp_breakpoint> bad(b); REFUSED(kp_format_breakpoints(&t, n_asm, kept_b.p, stride, bad.p, off.p, 5, nullptr, 0)); }
        REFUSED(kp_format_breakpoints(&t, n_asm, kept_ctg0.p, stride, recs.p, off.p, 5, nullptr, 0));   // fragment a's contig
        REFUSED(kp_format_breakpoints(&t, n_asm, kept_ctg_b.p, stride, recs.p, off.p, 5, nullptr, 0));  // fragment b's
        REFUSED(kp_format_breakpoints(&t, n_asm, kept_ctg1.p, stride, recs.p, off.p, 5, nullptr, 0));
        { Exact<kp_kept> bad(kept_with(0, 0, n_genes, 1)); REFUSED(kp_format_breakpoints(&t, n_asm, bad.p, stride, recs.p, off.p, 5, nullptr, 0)); }
        CHECK(kp_format_breakpoints(&t, 0, nullptr, 0, nullptr, nullptr, 5, nullptr, 0) == 0);
        // the integer column: the bytes of "%lld" at the ends of the 32-bit range and around the digit counts
        for (int32_t gap : {INT32_MIN, -2147483647, -10, -9, -1, 0, 9, 10, 99, 100, INT32_MAX}) {
            std::vector<kp_breakpoint> b{v[0]};
            b[0].q_gap = gap;
            Exact<kp_breakpoint> one(b);
            Exact<int64_t> o1({0, 1, 1});
            char want[160];
            std::snprintf(want, sizeof want, "a0\tg0\ttranslocation\t30\t%lld\tctg1\t130\t+\tc0\t530\t-\t.\t%lld\t3\t7\t.\n", (long long)gap, gap < 0 ? -(long long)gap : 0ll);
            good("integers", [&](char *out, int64_t cap) { return kp_format_breakpoints(&t, n_asm, kept_b.p, stride, one.p, o1.p, 5, out, cap); }, want);
        }
    }
    // ---- rescue
    {
        kp_allele_tables at{};
        at.names = t; at.locus_names = locus_b.p; at.locus_name_off = locus_off.p; at.n_loci = 2;
        kp_allele_tables at_no_names = at;
        at_no_names.names.asm_name_off = nullptr;
        Exact<int32_t> prot_len({10, 20, 30}), best({1, 0});
        std::vector<kp_rescue> v(2);
        std::memset(v.data(), 0, v.size() * sizeof(kp_rescue));
        v[0].gene = 1; v[0].piece = 0; v[0].contig = 1; v[0].t_start = 60; v[0].t_end = 120; v[0].score = 95; v[0].matches = 18; v[0].mismatches = 2;
        v[0].p_start = 0; v[0].p_end = 20; v[0].stops = 1; v[0].strand = -1; v[0].frame = 2;
        v[1].gene = 2; v[1].piece = -1;
        Exact<kp_rescue> recs(v);
        Exact<int64_t> off({0, 1, 2}), off3({0, 2, 3});
        good("rescue", [&](char *out, int64_t cap) { return kp_format_rescue(&at, n_asm, prot_len.p, best.p, recs.p, off.p, 80, out, cap); },
             "a0\tKL2\tgene1\t20\tdiverged\t95\tctg1\t61\t120\t-\t3\t1\t20\t18\t2\t0\t90.00\t100.00\t1\t.\n"
             "asm1\tL0\tg2\t30\tabsent\t0\t.\t.\t.\t.\t.\t.\t.\t0\t0\t0\t0.00\t0.00\t0\t.\n");
        REFUSED(kp_format_rescue(&at_no_names, n_asm, prot_len.p, best.p, recs.p, off.p, 80, nullptr, 0));
        { std::vector<kp_rescue> b{v[0], v[0], v[1]}; Exact<kp_rescue> three(b);
          CHECK(kp_format_rescue(&at, n_asm, prot_len.p, best.p, three.p, off3.p, 80, nullptr, 0) > 0);
          REFUSED(kp_format_rescue(&at, n_asm, prot_len.p, best.p, three.p, descending.p, 80, nullptr, 0));
          REFUSED(kp_format_rescue(&at, n_asm, prot_len.p, best.p, three.p, end_below_start.p, 80, nullptr, 0)); }
        { std::vector<kp_rescue> b = v; b[0].contig = 2; Exact<kp_rescue> bad(b); REFUSED(kp_format_rescue(&at, n_asm, prot_len.p, best.p, bad.p, off.p, 80, nullptr, 0)); }
        { std::vector<kp_rescue> b = v; b[1].gene = n_genes; Exact<kp_rescue> bad(b); REFUSED(kp_format_rescue(&at, n_asm, prot_len.p, best.p, bad.p, off.p, 80, nullptr, 0)); }
        { Exact<int32_t> bad({2, 0}); REFUSED(kp_format_rescue(&at, n_asm, prot_len.p, bad.p, recs.p, off.p, 80, nullptr, 0)); }  // a locus equal to n_loci
        CHECK(kp_format_rescue(&at, 0, nullptr, nullptr, nullptr, nullptr, 80, nullptr, 0) == 0);
    }
    // ---- PAF, without and with the cs strings
    {
        Exact<int32_t> gene_len({60, 70, 40}), ctg_len({1000, 2000, 300});
        kp_paf_tables pt{};
        pt.gene_names = gene_b.p; pt.gene_name_off = gene_off.p; pt.gene_len = gene_len.p; pt.n_genes = n_genes;
        pt.ctg_names = ctg_b.p; pt.ctg_name_off = ctg_off.p; pt.ctg_len = ctg_len.p; pt.asm_first_ctg = first.p;
        kp_paf_tables pt_no_first = pt;  // (a hit table names no assembly: the table of its assemblies is their first contigs)
        pt_no_first.asm_first_ctg = nullptr;
        std::vector<kp_hit> v(2);
        std::memset(v.data(), 0, v.size() * sizeof(kp_hit));
        v[0].gene = 0; v[0].contig = 1; v[0].q_start = 0; v[0].q_end = 30; v[0].t_start = 100; v[0].t_end = 130; v[0].score = 55; v[0].matches = 29; v[0].block_len = 30;
        v[0].strand = 1; v[0].mapq = 60;
        v[1].gene = 2; v[1].contig = 0; v[1].q_start = 5; v[1].q_end = 25; v[1].t_start = 10; v[1].t_end = 32; v[1].score = 30; v[1].matches = 20; v[1].block_len = 22;
        v[1].strand = -1;
        auto op = [](uint32_t kind, uint32_t n) { return (n << KP_CIGAR_SHIFT) | kind; };
        Exact<kp_hit> hits(v);
        Exact<uint32_t> ops({op(KP_CIGAR_M, 30), op(KP_CIGAR_M, 10), op(KP_CIGAR_D, 2), op(KP_CIGAR_M, 10)});
        Exact<int64_t> off({0, 1, 2}), cigar_off({0, 1, 4}), cs_off({0, 9, 18});
        Exact<char> cs(chars(":12*ag:17:10-ac:10")), cs_bad(chars(":12*ag:16:10-ac:10"));
        const std::string head0 = "g0\t60\t0\t30\t+\tctg1\t2000\t100\t130\t29\t30\t60\tAS:i:55\tNM:i:1\tcg:Z:", head1 = "g2\t40\t5\t25\t-\tc2\t300\t10\t32\t20\t22\t0\tAS:i:30\tNM:i:2\tcg:Z:";
        const std::string plain = head0 + "30M\n" + head1 + "10M2D10M\n";
        good("paf", [&](char *out, int64_t cap) { return kp_format_paf(&pt, n_asm, hits.p, off.p, ops.p, cigar_off.p, out, cap); }, plain);
        auto tags = [&](const kp_paf_tables *tables, const kp_hit *h, const int64_t *hit_off, const char *text, int32_t flags, char *out, int64_t cap) {
            return kp_format_paf_tags(tables, n_asm, h, hit_off, ops.p, cigar_off.p, text, cs_off.p, flags, out, cap);
        };
        good("paf, flags 0", [&](char *out, int64_t cap) { return tags(&pt, hits.p, off.p, nullptr, 0, out, cap); }, plain);
        good("paf, cs", [&](char *out, int64_t cap) { return tags(&pt, hits.p, off.p, cs.p, KP_PAF_CS, out, cap); },
             head0 + "30M\tcs:Z::12*ag:17\n" + head1 + "10M2D10M\tcs:Z::10-ac:10\n");
        good("paf, cs and eqx", [&](char *out, int64_t cap) { return tags(&pt, hits.p, off.p, cs.p, KP_PAF_CS | KP_PAF_EQX, out, cap); },
             head0 + "12=1X17=\tcs:Z::12*ag:17\n" + head1 + "10=2D10=\tcs:Z::10-ac:10\n");
        for (int32_t flags : {0, KP_PAF_CS, KP_PAF_EQX, KP_PAF_CS | KP_PAF_EQX}) {
            REFUSED(tags(&pt_no_first, hits.p, off.p, cs.p, flags, nullptr, 0));
            REFUSED(tags(&pt, hits.p, descending.p, cs.p, flags, nullptr, 0));
            REFUSED(tags(&pt, hits.p, end_below_start.p, cs.p, flags, nullptr, 0));
            { std::vector<kp_hit> b = v; b[0].contig = 2; Exact<kp_hit> bad(b); REFUSED(tags(&pt, bad.p, off.p, cs.p, flags, nullptr, 0)); }
            { std::vector<kp_hit> b = v; b[1].contig = 1; Exact<kp_hit> bad(b); REFUSED(tags(&pt, bad.p, off.p, cs.p, flags, nullptr, 0)); }
            { std::vector<kp_hit> b = v; b[1].gene = n_genes; Exact<kp_hit> bad(b); REFUSED(tags(&pt, bad.p, off.p, cs.p, flags, nullptr, 0)); }
            if (flags) REFUSED(tags(&pt, hits.p, off.p, cs_bad.p, flags, nullptr, 0));  // 29 columns of cs for 30M
        }
        REFUSED(tags(&pt, hits.p, off.p, cs.p, 4, nullptr, 0));  // an unknown flag
        REFUSED(kp_format_paf(&pt, n_asm, hits.p, descending.p, ops.p, cigar_off.p, nullptr, 0));
        { Exact<int64_t> none({0}); CHECK(kp_format_paf(&pt, 0, nullptr, none.p, nullptr, none.p, nullptr, 0) == 0); }
    }
    std::printf(fails ? "FAILED: %d checks\n" : "records_format_main: all checks passed\n", fails);
    return fails ? 1 : 0;
}
