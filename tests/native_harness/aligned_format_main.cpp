// aligned_format_main.cpp -- a stand-alone program around kp_format_aligned and the rows of kaptive_amd/csrc/kp_aligned.h, for a run
// under the host sanitizers (no GPU, nothing loaded into an interpreter):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -o aligned_format_main
//       tests/native_harness/aligned_format_main.cpp kaptive_amd/csrc/kp_rows.cpp && ./aligned_format_main
// Every table is a heap block of exactly the size the call may read or write: an access past an end stops the program.  It makes
// rows from random canonical op lists of 1 to 2000 ops on both strands at every residue of q_start, of the contig position and of
// the gene length, with N runs, on contigs that end with the assembly's last packed word, and compares every column with a walk
// through kp_code_at; makes the known answers of the specification and each kind of invalid walk; then formats a batch twice (sizing
// call with cap 0, then into a buffer of exactly the size returned) and checks every refusal.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kaptive_amd.h"
#include "../../kaptive_amd/csrc/kp_aligned.h"

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

static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #x); ++fails; } } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) {  // xorshift64*: [0, n)
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)(((rng_state * 0x2545f4914f6cdd1dull) >> 33) % n);
}

static uint32_t op(uint32_t kind, uint32_t n) { return (n << KP_CIGAR_SHIFT) | kind; }

// a canonical op list: M first and last, a gap of one or two kinds between neighbouring M ops, exactly n_ops ops where that can be
static std::vector<uint32_t> canonical(int n_ops) {
    std::vector<uint32_t> ops{op(KP_CIGAR_M, 1 + rnd(24))};
    while ((int)ops.size() + 2 <= n_ops) {
        const uint32_t first = rnd(2) ? KP_CIGAR_I : KP_CIGAR_D;
        ops.push_back(op(first, rnd(20) == 0 ? 16 * (1 + rnd(3)) : 1 + rnd(24)));
        if ((int)ops.size() + 2 <= n_ops && rnd(4) == 0) ops.push_back(op(first == KP_CIGAR_I ? KP_CIGAR_D : KP_CIGAR_I, 1 + rnd(24)));
        ops.push_back(op(KP_CIGAR_M, rnd(20) == 0 ? 16 * (1 + rnd(3)) : 1 + rnd(24)));
    }
    return ops;
}

// One record against a walk column by column through kp_code_at.  The contig is the assembly's second and last: it ends with the
// last packed word when (cstart + clen) % 16 == 0.
static void one_case(const std::vector<uint32_t> &ops_v, int strand, int q_start, int t_start, int pad_q, int pad_t, bool with_runs) {
    int64_t rows = 0, cols = 0;
    for (uint32_t o : ops_v) { rows += kp_aln_op_rows(o); cols += kp_aln_op_cols(o); }
    const int Lq = q_start + (int)rows + pad_q, cstart = 32, clen = t_start + (int)cols + pad_t;
    const int n_words = (cstart + clen + 15) / 16;
    std::vector<uint32_t> words_v((size_t)n_words);
    for (auto &w : words_v) w = rnd(0x7fffffff) * 2u + rnd(2);
    std::vector<int32_t> runs_v;
    if (with_runs)
        for (int at = (int)rnd(40); at + 2 < cstart + clen; at += 30 + (int)rnd(200)) {
            const int len = 1 + (int)rnd(35);
            runs_v.push_back(at); runs_v.push_back(at + len < cstart + clen ? at + len : cstart + clen);
            at += len;
        }
    Exact<uint32_t> words(words_v), ops(ops_v);
    Exact<int32_t> runs(runs_v);
    KpTargetSeq t;
    t.words = words.p; t.n_words = n_words; t.runs = runs.p; t.n_runs = (int)(runs_v.size() / 2); t.cstart = cstart; t.cend = cstart + clen;
    Exact<uint64_t> blocks(std::vector<uint64_t>((size_t)kp_aln_blocks(Lq), 0x5555555555555555ull));
    kp_aligned_row row;
    const bool ok = kp_aligned_row_blocks(ops.p, (int64_t)ops.n, true, t, Lq, q_start, q_start + (int)rows, t_start, strand, blocks.p, &row);
    if (!ok) { CHECK(!"a valid walk was refused"); return; }
    std::vector<int> want((size_t)Lq, 5);
    int r = strand < 0 ? Lq - (q_start + (int)rows) : q_start, tt = cstart + t_start, inserted = 0, n_ins = 0, covered = 0;
    for (uint32_t o : ops_v) {
        const int n = (int)(o >> KP_CIGAR_SHIFT);
        const uint32_t kind = o & 15u;
        if (kind == KP_CIGAR_M) {
            for (int x = 0; x < n; ++x) {
                int c = t.at(tt + x);
                if (strand < 0 && c <= 3) c = 3 - c;
                want[(size_t)(strand < 0 ? Lq - 1 - (r + x) : r + x)] = c;
            }
            r += n; tt += n; covered += n;
        } else if (kind == KP_CIGAR_I) r += n;
        else { tt += n; inserted += n; ++n_ins; }
    }
    bool same = row.gene_len == Lq && row.covered == covered && row.inserted == inserted && row.n_ins == n_ins;
    for (int j = 0; j < Lq && same; ++j) {
        const uint64_t v = blocks.p[j / 16];
        const int c = j % 16, got = ((v >> (48 + c)) & 1u) ? 5 : (((v >> (32 + c)) & 1u) ? 4 : (int)((v >> (2 * c)) & 3u));
        same = got == want[(size_t)j] && (got <= 3 || ((v >> (2 * c)) & 3u) == 0);
    }
    if (Lq % 16) same = same && (blocks.p[Lq / 16] >> (48 + Lq % 16)) == 0 && ((blocks.p[Lq / 16] >> 32) & 0xffffu) >> (Lq % 16) == 0;
    if (!same) { std::fprintf(stderr, "row differs: %zu ops, strand %d, q_start %d, t_start %d, Lq %d\n", ops_v.size(), strand, q_start, t_start, Lq); ++fails; }
}

int main() {
    // ---- rows against the column-by-column walk
    const int sizes[] = {1, 3, 5, 63, 65, 127, 129, 257, 511, 513, 1999, 2000};
    for (int strand = -1; strand <= 1; strand += 2) {
        for (int n_ops : sizes) one_case(canonical(n_ops), strand, (int)rnd(50), (int)rnd(50), (int)rnd(50), (int)rnd(20), true);
        for (int res = 0; res < 16; ++res)
            for (int other = 0; other < 16; ++other) {
                const std::vector<uint32_t> ops = canonical(9 + (int)rnd(30));
                int64_t cols = 0;
                for (uint32_t o : ops) cols += kp_aln_op_cols(o);
                one_case(ops, strand, res, other, (res * 7 + other) % 16, (int)((16 - (other + cols) % 16) % 16), (res + other) % 3 == 0);  // (the contig ends with the last word)
                one_case(ops, strand, 16 + other, res, res, 0, false);
            }
        one_case({op(KP_CIGAR_M, 16), op(KP_CIGAR_I, 16), op(KP_CIGAR_M, 32), op(KP_CIGAR_D, 16), op(KP_CIGAR_M, 16), op(KP_CIGAR_I, 48), op(KP_CIGAR_M, 16)}, strand, 16, 0, 16, 0, true);
        one_case({op(KP_CIGAR_M, 1)}, strand, 0, 0, 0, 0, false);
        one_case({op(KP_CIGAR_M, 1)}, strand, 15, 15, 0, 0, true);
    }
    // ---- the known answers of the specification, and each kind of invalid walk
    {
        // "ttacgtnacgga": t t a c g t n a c g g a
        const int codes[12] = {3, 3, 0, 1, 2, 3, 0, 0, 1, 2, 2, 0};
        uint32_t w = 0;
        for (int i = 0; i < 12; ++i) w |= (uint32_t)codes[i] << (2 * i);
        Exact<uint32_t> words({w});
        Exact<int32_t> runs({6, 7});
        Exact<uint32_t> ops({op(KP_CIGAR_M, 4), op(KP_CIGAR_I, 2), op(KP_CIGAR_M, 3), op(KP_CIGAR_D, 1), op(KP_CIGAR_M, 1)});
        KpTargetSeq t;
        t.words = words.p; t.n_words = 1; t.runs = runs.p; t.n_runs = 1; t.cstart = 0; t.cend = 12;
        Exact<uint64_t> blocks(std::vector<uint64_t>(2, 0));
        kp_aligned_row row;
        CHECK(kp_aligned_row_blocks(ops.p, 5, true, t, 20, 2, 12, 2, 1, blocks.p, &row));
        CHECK(blocks.p[0] == 0xf0c3010000900e40ull && blocks.p[1] == 0x000f000000000000ull && row.covered == 8 && row.inserted == 1 && row.n_ins == 1);
        CHECK(kp_aligned_row_blocks(ops.p, 5, true, t, 20, 2, 12, 2, -1, blocks.p, &row));
        CHECK(blocks.p[0] == 0xf0c3002000e40390ull && blocks.p[1] == 0x000f000000000000ull && row.covered == 8 && row.inserted == 1 && row.n_ins == 1);
        auto all_gap = [&](bool found, int Lq, int q_start, int q_end, int t_start, int strand) {
            blocks.p[0] = blocks.p[1] = 1;
            const bool ok = kp_aligned_row_blocks(ops.p, 5, found, t, Lq, q_start, q_end, t_start, strand, blocks.p, &row);
            const bool gap = Lq <= 0 || (blocks.p[0] == 0xffffull << 48 && blocks.p[1] == (Lq >= 32 ? 0xffffull : (1ull << (Lq - 16)) - 1) << 48);
            return !ok && gap && row.covered == 0 && row.inserted == 0 && row.n_ins == 0;
        };
        CHECK(all_gap(false, 20, 2, 12, 2, 1));   // the hit is not found
        CHECK(all_gap(true, 20, 2, 12, 4, 1));    // the contig ends before the ops do
        CHECK(all_gap(true, 20, 2, 12, -1, 1));   // a negative contig position
        CHECK(all_gap(true, 20, 11, 21, 2, 1));   // the gene ends before the ops do
        CHECK(all_gap(true, 20, -1, 9, 2, 1));    // a negative row
        CHECK(all_gap(true, 20, 11, 21, 2, -1));  // strand -1: the walk's first row is negative
        CHECK(all_gap(true, 20, -1, 9, 2, -1));   // strand -1: the gene ends before the ops do
        CHECK(all_gap(true, 0, 0, 0, 2, 1));      // a gene without a base: no block is written
        CHECK(blocks.p[0] == 1 && blocks.p[1] == 1);
        Exact<uint32_t> huge(std::vector<uint32_t>(40, op(KP_CIGAR_M, (1u << 28) - 1)));
        CHECK(!kp_aligned_row_blocks(huge.p, 40, true, t, 20, 0, 20, 0, 1, blocks.p, &row) && row.covered == 0);
    }

    // ---- the table: three assemblies (none, four records of which one spurious, one)
    const int n_asm = 3, kept_stride = 4;
    const std::string genes = "g0gene1g2", asms = "emptyasm twothree", ctgs = "xc1contig twoab";
    Exact<int32_t> gene_off({0, 2, 7, 9});
    Exact<int64_t> asm_off({0, 5, 12, 17}), ctg_off({0, 1, 3, 13, 14, 15}), first({0, 1, 3, 5});
    Exact<char> gene_b(std::vector<char>(genes.begin(), genes.end())), asm_b(std::vector<char>(asms.begin(), asms.end()));
    Exact<char> ctg_b(std::vector<char>(ctgs.begin(), ctgs.end()));
    std::vector<kp_kept> kept((size_t)n_asm * kept_stride);
    std::vector<kp_aligned_row> rows((size_t)n_asm * kept_stride);
    std::memset(kept.data(), 0, kept.size() * sizeof(kp_kept));
    std::memset(rows.data(), 0, rows.size() * sizeof(kp_aligned_row));
    const int lens[4] = {20, 16, 33, 1};
    std::vector<uint64_t> blk{0xf0c3010000900e40ull, 0x000f000000000000ull, 0x1b1b1b1bull, 0, 0xffffull << 48, 1ull << 48, 2};
    const int64_t offs[4] = {0, 2, 3, 6};
    for (int i = 0; i < 4; ++i) {
        kp_kept &k = kept[(size_t)kept_stride + i];
        k.gene = i % 3; k.contig = i & 1; k.t_start = 100 * i; k.t_end = 100 * i + lens[i]; k.q_start = i; k.q_end = lens[i]; k.strand = (i & 1) ? -1 : 1;
        k.flags = i == 1 ? KP_F_SPURIOUS : 0;
        rows[(size_t)kept_stride + i] = kp_aligned_row{offs[i], lens[i], lens[i] - i, i, i / 2};
    }
    kept[(size_t)2 * kept_stride] = kept[(size_t)kept_stride];
    rows[(size_t)2 * kept_stride] = rows[(size_t)kept_stride];
    Exact<kp_kept> kept_b(kept);
    Exact<kp_aligned_row> rows_b(rows);
    Exact<uint64_t> blocks_b(blk);
    Exact<int32_t> n_kept({0, 4, 1});
    kp_variant_tables t{};
    t.gene_names = gene_b.p; t.gene_name_off = gene_off.p; t.n_genes = 3;
    t.asm_names = asm_b.p; t.asm_name_off = asm_off.p; t.ctg_names = ctg_b.p; t.ctg_name_off = ctg_off.p; t.asm_first_ctg = first.p;
    const int64_t nblk = (int64_t)blk.size();
    const int64_t need = kp_format_aligned(&t, n_asm, n_kept.p, kept_b.p, kept_stride, rows_b.p, blocks_b.p, nblk, nullptr, 0);
    CHECK(need > 0);
    Exact<char> out(std::vector<char>((size_t)need, '#'));
    CHECK(kp_format_aligned(&t, n_asm, n_kept.p, kept_b.p, kept_stride, rows_b.p, blocks_b.p, nblk, out.p, need) == need);
    const std::string text(out.p, (size_t)need);
    int lines = 0;
    for (char c : text) lines += c == '\n';
    CHECK(lines == 3 + 1);
    CHECK(text.rfind("asm two\tg0\tc1\t1\t20\t+\t20\t1\t20\t20\t0\t0\t--acgt--nacg--------\n", 0) == 0);
    CHECK(text.find("gene1") == std::string::npos);  // the spurious record
    CHECK(text.find("asm two\tg2\tc1\t201\t233\t+\t33\t3\t33\t31\t2\t1\taaaaaaaaaaaaaaaa-----------------\n") != std::string::npos);
    CHECK(text.find("asm two\tg0\tcontig two\t301\t301\t-\t1\t4\t1\t-2\t3\t1\tg\n") != std::string::npos);
    CHECK(text.find("three\tg0\ta\t1\t20\t+\t20\t") != std::string::npos);
    if (need > 1) {  // a buffer one byte short: the count is the same, nothing is written past it
        Exact<char> shorter(std::vector<char>((size_t)need - 1, '#'));
        CHECK(kp_format_aligned(&t, n_asm, n_kept.p, kept_b.p, kept_stride, rows_b.p, blocks_b.p, nblk, shorter.p, need - 1) == need);
    }
    // ---- refusals
    auto refused = [&](const int32_t *nk, const kp_kept *k, const kp_aligned_row *r, int64_t nb) {
        return kp_format_aligned(&t, n_asm, nk, k, kept_stride, r, blocks_b.p, nb, nullptr, 0) == KP_EINVAL;
    };
    { Exact<int32_t> bad({0, 5, 1}); CHECK(refused(bad.p, kept_b.p, rows_b.p, nblk)); }
    { Exact<int32_t> bad({0, -1, 1}); CHECK(refused(bad.p, kept_b.p, rows_b.p, nblk)); }
    CHECK(refused(n_kept.p, kept_b.p, rows_b.p, nblk - 1));  // the last row runs outside the blocks
    CHECK(refused(n_kept.p, kept_b.p, rows_b.p, -1));
    for (int what = 0; what < 4; ++what) {
        std::vector<kp_aligned_row> r2 = rows;
        kp_aligned_row &r = r2[(size_t)kept_stride + 2];
        if (what == 0) r.off = nblk; else if (what == 1) r.off = -1; else if (what == 2) r.gene_len = -1; else r.gene_len = 16 * 4 + 1;
        Exact<kp_aligned_row> bad(r2);
        CHECK(refused(n_kept.p, kept_b.p, bad.p, nblk));
    }
    for (int what = 0; what < 3; ++what) {
        std::vector<kp_kept> k2 = kept;
        kp_kept &k = k2[(size_t)kept_stride + 2];
        if (what == 0) k.gene = 3; else if (what == 1) k.contig = 2; else k.gene = -1;
        Exact<kp_kept> bad(k2);
        CHECK(refused(n_kept.p, bad.p, rows_b.p, nblk));
    }
    CHECK(kp_format_aligned(nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 0) == KP_EINVAL);
    CHECK(kp_format_aligned(&t, 0, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 0) == 0);
    std::printf(fails ? "FAILED: %d checks\n" : "aligned_format_main: all checks passed\n", fails);
    return fails ? 1 : 0;
}
