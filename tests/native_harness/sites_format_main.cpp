// sites_format_main.cpp -- a stand-alone program around kaptive_amd/csrc/kp_sites.h, kp_format_sites and kp_format_site_rows, for a run
// under the host sanitizers (no GPU, nothing loaded into an interpreter):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -o sites_format_main
//       tests/native_harness/sites_format_main.cpp kaptive_amd/csrc/kp_rows.cpp && ./sites_format_main
// Every table is a heap block of exactly the size the call may read or write: an access past an end stops the program.  It adds
// random masks into the bit-sliced counter up to its limit and compares with a plain count; transposes random 64 x 64 bit matrices;
// makes matrices of 1 to 70 blocks and up to 600 rows from random codes, profiles them the way a wave does (a counter per lane, the
// transposition, a popcount) and compares every column with a walk row by row, cuts the site rows and decodes them again; maps every
// column of a locus to its gene; then formats both tables twice (sizing call with cap 0, then into a buffer of exactly the size
// returned) and checks every refusal.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kaptive_amd.h"
#include "../../kaptive_amd/csrc/kp_sites.h"

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
static uint64_t rnd64() {  // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return rng_state * 0x2545f4914f6cdd1dull;
}
static uint32_t rnd(uint32_t n) { return (uint32_t)((rnd64() >> 33) % n); }

// codes 0..3, 4 = N, 5 = GAP -> blocks
static std::vector<uint64_t> pack(const std::vector<uint8_t> &codes) {
    std::vector<uint64_t> b(codes.size() / 16, 0);
    for (size_t c = 0; c < codes.size(); ++c) {
        const int j = (int)(c & 15);
        if (codes[c] < 4) b[c / 16] |= (uint64_t)codes[c] << (2 * j);
        else if (codes[c] == 4) b[c / 16] |= 1ull << (32 + j);
        else b[c / 16] |= 1ull << (48 + j);
    }
    return b;
}

static void counter_case(int n, int kind) {
    KpSiteCounter c{};
    int32_t want[64] = {0};
    for (int i = 0; i < n; ++i) {
        const uint64_t m = kind == 0 ? rnd64() : kind == 1 ? ~0ull : 0ull;
        kp_sites_counter_add(&c, m);
        for (int j = 0; j < 64; ++j) want[j] += (int32_t)((m >> j) & 1);
    }
    for (int j = 0; j < 64; ++j) CHECK(kp_sites_counter_get(&c, j) == want[j]);
}

static void transpose_case() {
    std::vector<uint64_t> v(64);
    for (auto &x : v) x = rnd64();
    const Exact<uint64_t> x(v);
    kp_sites_transpose64(x.p);
    for (int i = 0; i < 64; ++i)
        for (int j = 0; j < 64; ++j) CHECK(((x.p[j] >> i) & 1) == ((v[(size_t)i] >> j) & 1));
}

static void matrix_case(int R, int nb, int32_t flags) {
    const int cols = 16 * nb;
    std::vector<uint8_t> codes((size_t)R * cols);
    std::vector<uint8_t> founder((size_t)cols);
    for (auto &c : founder) c = (uint8_t)rnd(4);
    for (int r = 0; r < R; ++r)
        for (int c = 0; c < cols; ++c) {
            const uint32_t u = rnd(40);
            codes[(size_t)r * cols + c] = u < 34 ? founder[(size_t)c] : u < 37 ? (uint8_t)rnd(4) : u < 38 ? 4 : 5;
        }
    const Exact<uint64_t> m(pack(codes));
    const int64_t NW = kp_dist_words(nb);
    std::vector<kp_site> table((size_t)(64 * NW));
    for (int64_t c = 0; c < 64 * NW; ++c) kp_site_store(&table[(size_t)c], (int32_t)c, 0, 0, 0, 0, 0);
    for (int64_t w = 0; w < NW; ++w)
        for (int r0 = 0; r0 < R; r0 += 64 * KP_SITES_LANE_ROWS) {  // a wave and its rows
            KpSiteCounter cnt[64][KP_SITES_CLASSES] = {};
            for (int lane = 0; lane < 64; ++lane)
                for (int i = 0; i < KP_SITES_LANE_ROWS; ++i) {
                    const int r = r0 + i * 64 + lane;
                    if (r >= R) continue;
                    const KpDistWord q = kp_dist_word_planes(m.p + (size_t)r * nb, nb, w);
                    const KpSiteMasks k = kp_sites_masks(q.lo, q.hi, q.valid, q.present);
                    for (int c = 0; c < KP_SITES_CLASSES; ++c) kp_sites_counter_add(&cnt[lane][c], k.m[c]);
                }
            for (int c = 0; c < KP_SITES_CLASSES; ++c)
                for (int b = 0; b < KP_SITES_PLANES; ++b) {
                    uint64_t x[64];
                    for (int lane = 0; lane < 64; ++lane) x[lane] = cnt[lane][c].p[b];
                    kp_sites_transpose64(x);
                    for (int j = 0; j < 64; ++j) (&table[(size_t)(w * 64 + j)].n[0])[c] += __builtin_popcountll(x[j]) << b;
                }
        }
    std::vector<kp_site> sites;
    for (int c = 0; c < cols; ++c) {
        int32_t want[6] = {0, 0, 0, 0, 0, 0};
        for (int r = 0; r < R; ++r) ++want[codes[(size_t)r * cols + c]];
        const kp_site &t = table[(size_t)c];
        CHECK(t.column == c && t.n[0] == want[0] && t.n[1] == want[1] && t.n[2] == want[2] && t.n[3] == want[3] && t.n_n == want[4]);
        CHECK(kp_site_gap(t.n, t.n_n, R) == want[5]);
        const bool two = (want[0] > 0) + (want[1] > 0) + (want[2] > 0) + (want[3] > 0) >= 2;
        CHECK(kp_site_is(t.n, t.n_n, R, flags) == (two && (!(flags & KP_SITES_CORE) || (want[4] == 0 && want[5] == 0))));
        if (kp_site_is(t.n, t.n_n, R, flags)) sites.push_back(t);
    }
    for (int64_t c = cols; c < 64 * NW; ++c) CHECK(kp_site_alleles(table[(size_t)c].n) == 0 && table[(size_t)c].n_n == 0);  // a short last word
    // the site rows, cut and decoded again
    const int64_t S = (int64_t)sites.size(), SB = kp_site_row_blocks(S);
    std::vector<uint64_t> rows((size_t)(R * SB));
    for (int r = 0; r < R; ++r)
        for (int64_t sb = 0; sb < SB; ++sb) {
            uint64_t v = 0;
            for (int k = 0; k < KP_SITES_BLOCK; ++k) {
                const int64_t s = sb * KP_SITES_BLOCK + k;
                if (s >= S) { v |= 1ull << (KP_DIST_GAP_SHIFT + k); continue; }
                const int64_t c = sites[(size_t)s].column;
                const KpDistWord q = kp_dist_word_planes(m.p + (size_t)r * nb, nb, c >> 6);
                const int bit = (int)(c & 63);
                v |= kp_site_block_code(k, q.lo >> bit, q.hi >> bit, q.valid >> bit, q.present >> bit);
            }
            rows[(size_t)(r * SB + sb)] = v;
        }
    if (SB > 0) CHECK((rows[(size_t)(SB - 1)] & kp_dist_pad_mask(S)) == kp_dist_pad_mask(S));
    std::vector<char> names;
    std::vector<int64_t> off{0};
    for (int r = 0; r < R; ++r) { names.push_back((char)('A' + r % 26)); off.push_back((int64_t)names.size()); }
    const Exact<char> nm(names);
    const Exact<int64_t> no(off);
    const Exact<uint64_t> blk(rows);
    const int64_t need = kp_format_site_rows("L", 1, nm.p, no.p, R, nullptr, S, blk.p, nullptr, 0);
    CHECK(need == (S ? (int64_t)R * (1 + 1 + 1 + 1 + (int64_t)std::to_string(S).size() + 1 + S + 1) : 0));
    const Exact<char> out(std::vector<char>((size_t)need, '?'));
    CHECK(kp_format_site_rows("L", 1, nm.p, no.p, R, nullptr, S, blk.p, out.p, need) == need);
    int64_t at = 0;
    for (int r = 0; r < R && S; ++r) {
        at += 4 + (int64_t)std::to_string(S).size() + 1;
        for (int64_t s = 0; s < S; ++s) CHECK(out.p[at + s] == "acgtn-"[codes[(size_t)r * cols + sites[(size_t)s].column]]);
        at += S + 1;
    }
}

int main() {
    for (int kind = 0; kind < 3; ++kind)
        for (int n = 0; n <= KP_SITES_LANE_ROWS; ++n) counter_case(n, kind);
    for (int rep = 0; rep < 8; ++rep) transpose_case();
    for (int nb : {1, 2, 3, 4, 5, 8, 33, 70})
        for (int R : {1, 2, 3, 63, 64, 65, 600}) matrix_case(R, nb, (R + nb) & 1 ? KP_SITES_CORE : 0);
    {   // the predicate and what is derived, at the specification's known answers and at the ties
        const int32_t a[4] = {1, 1, 0, 0}, b[4] = {0, 2, 2, 0}, c[4] = {0, 0, 0, 5}, d[4] = {1, 2, 0, 2};
        CHECK(kp_site_is(a, 0, 3, 0) && !kp_site_is(a, 0, 3, KP_SITES_CORE) && kp_site_is(a, 0, 2, KP_SITES_CORE) && !kp_site_is(a, 1, 3, KP_SITES_CORE));
        CHECK(kp_site_alleles(a) == 2 && kp_site_major(a) == 0 && !kp_site_informative(a) && kp_site_gap(a, 0, 3) == 1);
        CHECK(kp_site_major(b) == 1 && kp_site_informative(b) && !kp_site_is(c, 0, 5, 0) && kp_site_major(c) == 3 && kp_site_major(d) == 1 && kp_site_informative(d));
        kp_site rec;
        kp_site_store(&rec, 9, 1, 2, 3, 4, 5);
        CHECK(rec.column == 9 && rec.n[0] == 1 && rec.n[1] == 2 && rec.n[2] == 3 && rec.n[3] == 4 && rec.n_n == 5);
        // the three blocks of the known answers
        uint64_t v[3] = {0, 0, 0};
        const char *text[3] = {"acgacg", "cgtcgt", "------"};
        for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 16; ++k) {
                const char ch = k < 6 ? text[r][k] : '-';
                const int code = ch == 'a' ? 0 : ch == 'c' ? 1 : ch == 'g' ? 2 : 3;
                v[r] |= ch == '-' ? kp_site_block_code(k, 0, 0, 0, 0) : kp_site_block_code(k, code & 1, code >> 1, 1, 1);
            }
        }
        CHECK(v[0] == 0xffc0000000000924ull && v[1] == 0xffc0000000000e79ull && v[2] == 0xffff000000000000ull);
        CHECK(kp_site_block_code(3, 0, 0, 0, 1) == 1ull << 35 && kp_site_row_blocks(0) == 0 && kp_site_row_blocks(16) == 1 && kp_site_row_blocks(17) == 2);
    }
    {   // every column of a locus of genes of 1, 15, 16, 17 and 32 bases
        const int len[5] = {1, 15, 16, 17, 32};
        const Exact<int64_t> gb({1, 1, 1, 2, 2});
        int64_t col = 0;
        for (int g = 0; g < 5; ++g)
            for (int64_t p = 0; p < 16 * gb.p[g]; ++p, ++col) {
                int64_t pos = -1;
                CHECK(kp_site_gene(gb.p, 5, col, &pos) == g && pos == p);
                (void)len;
            }
        int64_t pos = 0;
        CHECK(col == 112 && kp_site_gene(gb.p, 5, 112, &pos) == -1 && kp_site_gene(gb.p, 5, -1, &pos) == -1 && kp_site_gene(gb.p, 0, 0, &pos) == -1);
    }
    {   // the site formatter: size, then fill exactly
        const std::string names_s = "wzi" "gene two" "" "g_4";
        const Exact<char> names(std::vector<char>(names_s.begin(), names_s.end()));
        const Exact<int64_t> off({0, 3, 11, 11, 14});
        const Exact<int32_t> len({16, 17, 31, 20});  // first columns 0, 16, 48, 80
        const Exact<kp_site> sites({{0, {1, 1, 0, 0}, 0}, {32, {0, 1, 0, 1}, 7}, {78, {3, 0, 0, 3}, 0}, {99, {0, 8, 1, 0}, 0}});
        const Exact<char> locus(std::vector<char>{'K', 'L', '2'});
        const std::string want = "KL2\twzi\t1\t1\t9\t1\t1\t0\t0\t0\t7\t2\ta\tno\nKL2\tgene two\t17\t33\t9\t0\t1\t0\t1\t7\t0\t2\tc\tno\n"
                                 "KL2\t\t31\t64\t9\t3\t0\t0\t3\t0\t3\t2\ta\tyes\nKL2\tg_4\t20\t84\t9\t0\t8\t1\t0\t0\t0\t2\tc\tno\n";
        const int64_t need = kp_format_sites(locus.p, 3, names.p, off.p, 4, nullptr, len.p, 9, sites.p, 4, nullptr, 0);
        CHECK(need == (int64_t)want.size());
        const Exact<char> out(std::vector<char>((size_t)need, '?'));
        CHECK(kp_format_sites(locus.p, 3, names.p, off.p, 4, nullptr, len.p, 9, sites.p, 4, out.p, need) == need);
        CHECK(std::memcmp(out.p, want.data(), want.size()) == 0);
        const Exact<char> small(std::vector<char>(10, '?'));  // too small: counted, nothing stored past its end
        CHECK(kp_format_sites(locus.p, 3, names.p, off.p, 4, nullptr, len.p, 9, sites.p, 4, small.p, 10) == need);
        const Exact<int32_t> genes({3, 2, 1, 0});
        CHECK(kp_format_sites(locus.p, 3, names.p, off.p, 4, genes.p, len.p, 9, sites.p, 1, small.p, 10) == (int64_t)std::strlen("KL2\tg_4\t1\t1\t9\t1\t1\t0\t0\t0\t7\t2\ta\tno\n"));
        CHECK(kp_format_sites(locus.p, 3, names.p, off.p, 4, nullptr, len.p, 9, sites.p, 0, nullptr, 0) == 0);
        CHECK(kp_format_sites(nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, 0) == 0);
        CHECK(kp_format_sites(locus.p, 3, names.p, off.p, 4, nullptr, len.p, 8, sites.p, 4, nullptr, 0) == KP_EINVAL);  // counts that exceed R
        CHECK(kp_format_sites(locus.p, 3, names.p, off.p, 3, nullptr, len.p, 9, sites.p, 4, nullptr, 0) == KP_EINVAL);  // a site outside the matrix
        CHECK(kp_format_sites(locus.p, 3, names.p, nullptr, 4, nullptr, len.p, 9, sites.p, 4, nullptr, 0) == KP_EINVAL);
        CHECK(kp_format_sites(locus.p, 3, names.p, off.p, 4, nullptr, nullptr, 9, sites.p, 4, nullptr, 0) == KP_EINVAL);
        CHECK(kp_format_sites(locus.p, 3, names.p, off.p, 4, nullptr, len.p, 9, nullptr, 4, nullptr, 0) == KP_EINVAL);
        CHECK(kp_format_sites(locus.p, 3, names.p, off.p, 4, nullptr, len.p, 9, sites.p, 4, nullptr, 5) == KP_EINVAL);
        CHECK(kp_format_sites(locus.p, -1, names.p, off.p, 4, nullptr, len.p, 9, sites.p, 4, nullptr, 0) == KP_EINVAL);
        CHECK(kp_format_sites(locus.p, 3, names.p, off.p, 4, nullptr, len.p, -1, sites.p, 4, nullptr, 0) == KP_EINVAL);
        const Exact<int32_t> wrong({0, 1, 2, 4});
        CHECK(kp_format_sites(locus.p, 3, names.p, off.p, 4, wrong.p, len.p, 9, sites.p, 4, nullptr, 0) == KP_EINVAL);
        for (const kp_site &bad : {kp_site{33, {1, 1, 0, 0}, 0}, kp_site{79, {1, 1, 0, 0}, 0}, kp_site{112, {1, 1, 0, 0}, 0}, kp_site{-1, {1, 1, 0, 0}, 0},
                                   kp_site{0, {9, 0, 0, 0}, 0}, kp_site{0, {0, 0, 0, 0}, 9}, kp_site{0, {-1, 2, 1, 0}, 0}, kp_site{0, {1, 1, 0, 0}, -1}}) {
            const Exact<kp_site> one({bad});
            CHECK(kp_format_sites(locus.p, 3, names.p, off.p, 4, nullptr, len.p, 9, one.p, 1, nullptr, 0) == KP_EINVAL);
        }
        const Exact<kp_site> twice({{5, {1, 1, 0, 0}, 0}, {5, {1, 1, 0, 0}, 0}});
        CHECK(kp_format_sites(locus.p, 3, names.p, off.p, 4, nullptr, len.p, 9, twice.p, 2, nullptr, 0) == KP_EINVAL);  // sites ascend
    }
    {   // the alignment formatter's refusals
        const Exact<char> names(std::vector<char>{'a', 'b'});
        const Exact<int64_t> off({0, 1, 2});
        const Exact<uint64_t> blk({0xfffc000000000004ull, 0xfffc000100000000ull});
        const std::string want = "x\ta\t2\tac\nx\tb\t2\tna\n";
        const Exact<char> out(std::vector<char>(want.size(), '?'));
        CHECK(kp_format_site_rows("x", 1, names.p, off.p, 2, nullptr, 2, blk.p, out.p, (int64_t)want.size()) == (int64_t)want.size() && std::memcmp(out.p, want.data(), want.size()) == 0);
        const Exact<int32_t> swap({1, 0});
        CHECK(kp_format_site_rows("x", 1, names.p, off.p, 2, swap.p, 2, blk.p, out.p, (int64_t)want.size()) == (int64_t)want.size() && out.p[2] == 'b');
        CHECK(kp_format_site_rows("x", 1, names.p, off.p, 2, nullptr, 0, nullptr, nullptr, 0) == 0);
        CHECK(kp_format_site_rows("x", 1, names.p, off.p, 2, nullptr, 1, blk.p, nullptr, 0) == KP_EINVAL);   // column 1 is not flagged
        CHECK(kp_format_site_rows("x", 1, names.p, off.p, 2, nullptr, 2, nullptr, nullptr, 0) == KP_EINVAL);
        CHECK(kp_format_site_rows("x", 1, names.p, nullptr, 2, nullptr, 2, blk.p, nullptr, 0) == KP_EINVAL);
        CHECK(kp_format_site_rows("x", 1, names.p, off.p, 2, nullptr, -1, blk.p, nullptr, 0) == KP_EINVAL);
        CHECK(kp_format_site_rows("x", 1, names.p, off.p, 2, nullptr, 2, blk.p, nullptr, 3) == KP_EINVAL);
        const Exact<int32_t> wrong({0, 2});
        CHECK(kp_format_site_rows("x", 1, names.p, off.p, 2, wrong.p, 2, blk.p, nullptr, 0) == KP_EINVAL);
        const Exact<uint64_t> both({0xfffc000000000004ull, 0xfffd000100000000ull});  // N and GAP at once
        CHECK(kp_format_site_rows("x", 1, names.p, off.p, 2, nullptr, 2, both.p, nullptr, 0) == KP_EINVAL);
    }
    std::printf(fails ? "FAILED: %d checks\n" : "sites_format_main: all checks passed\n", fails);
    return fails ? 1 : 0;
}
