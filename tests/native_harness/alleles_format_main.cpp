// alleles_format_main.cpp -- a stand-alone program around kp_format_alleles and the digests of kaptive_amd/csrc/kp_alleles.h, for a
// run under the host sanitizers (no GPU, nothing loaded into an interpreter):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -o alleles_format_main
//       tests/native_harness/alleles_format_main.cpp kaptive_amd/csrc/kp_rows.cpp && ./alleles_format_main
// Every table is a heap block of exactly the size the call may read: a read or write past an end stops the program.  It formats a
// batch twice (sizing call with cap 0, then into a buffer of exactly the size returned), checks every refusal, and digests
// intervals that end on the last base of the last packed word on both strands.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kaptive_amd.h"
#include "../../kaptive_amd/csrc/kp_alleles.h"

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

int main() {
    // ---- the table: three assemblies (none, six records of which one spurious and one without a protein, two records and no piece)
    const int n_asm = 3, kept_stride = 6, piece_stride = 2;
    const std::string genes = "g0gene1g2", loci = "KL1KL20", asms = "emptyasm twothree", ctgs = "xc1contig twoab";
    Exact<int32_t> gene_off({0, 2, 7, 9}), locus_off({0, 3, 7});
    Exact<int64_t> asm_off({0, 5, 12, 17}), ctg_off({0, 1, 3, 13, 14, 15}), first({0, 1, 3, 5});
    Exact<char> gene_b(std::vector<char>(genes.begin(), genes.end())), locus_b(std::vector<char>(loci.begin(), loci.end()));
    Exact<char> asm_b(std::vector<char>(asms.begin(), asms.end())), ctg_b(std::vector<char>(ctgs.begin(), ctgs.end()));
    std::vector<kp_kept> kept((size_t)n_asm * kept_stride);
    std::vector<kp_allele> al((size_t)n_asm * kept_stride);
    std::memset(kept.data(), 0, kept.size() * sizeof(kp_kept));
    const uint8_t flags[6] = {KP_F_EXPECTED | KP_F_INSIDE, KP_F_EXPECTED, KP_F_INSIDE, 0, KP_F_EXTRA | KP_F_INSIDE | KP_F_SPURIOUS, KP_F_EXTRA};
    for (int i = 0; i < 6; ++i) {
        kp_kept &k = kept[(size_t)kept_stride + i];
        k.gene = i % 3; k.contig = i & 1; k.t_start = 100 * i; k.t_end = 100 * i + 50 + i; k.strand = (i & 1) ? -1 : 1; k.state = (int8_t)(i % 4);
        k.flags = flags[i]; k.prot_len = i == 2 ? 0 : 10 + i;
        al[(size_t)kept_stride + i] = kp_allele{0x0123456789abcdefull * (uint64_t)(i + 1), i == 2 ? 0 : ~0ull - (uint64_t)i};
    }
    for (int i = 0; i < 2; ++i) {
        kept[(size_t)2 * kept_stride + i] = kept[(size_t)kept_stride + i];
        al[(size_t)2 * kept_stride + i] = al[(size_t)kept_stride + i];
    }
    Exact<kp_kept> kept_b(kept);
    Exact<kp_allele> al_b(al);
    Exact<uint64_t> pd({0, 0, 0x1111111111111111ull, 0x2222222222222222ull, 0, 0});
    Exact<int32_t> order({0, 1, 1, 0, 0, 1}), n_kept({0, 6, 2}), n_pieces({0, 2, 0}), best({1, 1, 0});
    kp_allele_tables t{};
    t.names.gene_names = gene_b.p; t.names.gene_name_off = gene_off.p; t.names.n_genes = 3;
    t.names.asm_names = asm_b.p; t.names.asm_name_off = asm_off.p; t.names.ctg_names = ctg_b.p; t.names.ctg_name_off = ctg_off.p;
    t.names.asm_first_ctg = first.p;
    t.locus_names = locus_b.p; t.locus_name_off = locus_off.p; t.n_loci = 2;

    const int64_t need = kp_format_alleles(&t, n_asm, n_kept.p, n_pieces.p, best.p, kept_b.p, al_b.p, kept_stride, pd.p, order.p, piece_stride, nullptr, 0);
    CHECK(need > 0);
    Exact<char> out(std::vector<char>((size_t)need, '#'));
    CHECK(kp_format_alleles(&t, n_asm, n_kept.p, n_pieces.p, best.p, kept_b.p, al_b.p, kept_stride, pd.p, order.p, piece_stride, out.p, need) == need);
    const std::string text(out.p, (size_t)need);
    int lines = 0;
    for (char c : text) lines += c == '\n';
    CHECK(lines == 5 + 2);
    const int32_t ord[2] = {1, 0};
    char hex[17];
    std::snprintf(hex, sizeof hex, "%016llx", (unsigned long long)kp_allele_locus_digest(pd.p + 2, ord, 2));
    CHECK(text.rfind(std::string("asm two\tKL20\t") + hex + "\tg0\texpected_in\tc1\t1\t50\t+\tnormal\t50\t0123456789abcdef\t10\tffffffffffffffff\n", 0) == 0);
    CHECK(text.find("\tg2\tother_in\tc1\t201\t252\t+\ttruncated\t52\t") != std::string::npos && text.find("\t0\t.\n") != std::string::npos);
    CHECK(text.find("three\tKL1\t.\tg0\t") != std::string::npos && text.find("extra_in") == std::string::npos && text.find("extra_out") != std::string::npos);
    if (need > 1) {  // a buffer one byte short: the count is the same, nothing is written past it
        Exact<char> shorter(std::vector<char>((size_t)need - 1, '#'));
        CHECK(kp_format_alleles(&t, n_asm, n_kept.p, n_pieces.p, best.p, kept_b.p, al_b.p, kept_stride, pd.p, order.p, piece_stride, shorter.p, need - 1) == need);
    }
    // ---- refusals
    auto refused = [&](const int32_t *nk, const int32_t *np, const int32_t *b, const kp_kept *k, const int32_t *o) {
        return kp_format_alleles(&t, n_asm, nk, np, b, k, al_b.p, kept_stride, pd.p, o, piece_stride, nullptr, 0) == KP_EINVAL;
    };
    { Exact<int32_t> bad({0, 7, 2}); CHECK(refused(bad.p, n_pieces.p, best.p, kept_b.p, order.p)); }
    { Exact<int32_t> bad({0, -1, 2}); CHECK(refused(bad.p, n_pieces.p, best.p, kept_b.p, order.p)); }
    { Exact<int32_t> bad({0, 3, 0}); CHECK(refused(n_kept.p, bad.p, best.p, kept_b.p, order.p)); }
    { Exact<int32_t> bad({1, 2, 0}); CHECK(refused(n_kept.p, n_pieces.p, bad.p, kept_b.p, order.p)); }
    { Exact<int32_t> bad({0, 1, 2, 0, 0, 1}); CHECK(refused(n_kept.p, n_pieces.p, best.p, kept_b.p, bad.p)); }
    for (int what = 0; what < 3; ++what) {
        std::vector<kp_kept> k2 = kept;
        kp_kept &k = k2[(size_t)kept_stride + 3];
        if (what == 0) k.gene = 3; else if (what == 1) k.contig = 2; else k.state = 4;
        Exact<kp_kept> bad(k2);
        CHECK(refused(n_kept.p, n_pieces.p, best.p, bad.p, order.p));
    }
    CHECK(kp_format_alleles(nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 0) == KP_EINVAL);
    CHECK(kp_format_alleles(&t, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 0) == 0);
    CHECK(kp_allele_locus_digest(pd.p, nullptr, 0) == 0);

    // ---- digests of intervals that end on the last base of the last packed word, and known answers
    std::vector<uint32_t> w(5);
    for (size_t i = 0; i < w.size(); ++i) w[i] = 0x9e3779b9u * (uint32_t)(i + 1);
    Exact<uint32_t> words(w);
    Exact<int32_t> runs({3, 5, 30, 47, 79, 80});
    KpTargetSeq seq;
    seq.words = words.p; seq.n_words = 5; seq.runs = runs.p; seq.n_runs = 3; seq.cstart = 16; seq.cend = 80;
    for (int strand = -1; strand <= 1; strand += 2)
        for (int start = 0; start <= 64; ++start)
            for (int end = start; end <= 64; ++end) {
                uint64_t S = 0;  // the blocks through kp_code_at, column by column
                const int L = end - start;
                for (int i = 0; i < (L + 15) / 16; ++i) {
                    uint64_t wv = 0, mv = 0;
                    for (int j = 0; j < 16 && 16 * i + j < L; ++j) {
                        const int p = 16 * i + j;
                        int x = seq.at(strand >= 0 ? seq.cstart + start + p : seq.cstart + end - 1 - p);
                        if (strand < 0 && x <= 3) x = 3 - x;
                        if (x < 4) wv |= (uint64_t)x << (2 * j); else mv |= 1ull << j;
                    }
                    S += kp_al_term(i, wv | (mv << 32));
                }
                if (kp_al_nt_digest(seq, start, end, strand) != kp_al_finish(S, KP_AL_TAG_NT, (uint64_t)L)) { CHECK(!"interval digest"); start = end = 65; }
            }
    CHECK(kp_al_nt_digest(seq, 0, 65, 1) == 0 && kp_al_nt_digest(seq, -1, 5, 1) == 0);
    Exact<uint32_t> acgt({0xe4u});
    Exact<int32_t> none(std::vector<int32_t>{});
    KpTargetSeq one;
    one.words = acgt.p; one.n_words = 1; one.runs = none.p; one.n_runs = 0; one.cstart = 0; one.cend = 4;
    CHECK(kp_al_nt_digest(one, 0, 4, 1) == 0x5eeccfc7d63eed1eull && kp_al_nt_digest(one, 0, 0, 1) == 0x332e6d2b1a14193eull);
    CHECK(kp_al_nt_digest(one, 0, 4, -1) == 0x5eeccfc7d63eed1eull);  // (acgt is its own reverse complement)
    Exact<uint8_t> prot({'M', 'K', 'L', 'V', 'A', 'A', 'A', 'A', 'W'});
    CHECK(kp_al_aa_digest(prot.p, 9) == 0x973b1ff3dad4bcacull && kp_al_aa_digest(prot.p, 8) == 0x329e08ccffb44565ull && kp_al_aa_digest(prot.p, 1) == 0x137859f1719b82adull);
    std::printf(fails ? "FAILED: %d checks\n" : "alleles_format_main: all checks passed\n", fails);
    return fails ? 1 : 0;
}
