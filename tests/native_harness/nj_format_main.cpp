// nj_format_main.cpp -- a stand-alone program around kaptive_amd/csrc/kp_nj.h and kp_format_nj, for a run under the host sanitizers
// (no GPU, nothing loaded into an interpreter):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -o nj_format_main
//       tests/native_harness/nj_format_main.cpp kaptive_amd/csrc/kp_rows.cpp && ./nj_format_main
// Every table is a heap block of exactly the size the call may read or write: an access past an end stops the program.  It checks
// SUM64 at its edges, the two known answers of kp_nj_host, the taxa and the matrix of blocks at the edge of the taxon rule, and the
// formatter: sized with cap 0, filled into a buffer of exactly the size returned, quoted names, %.9g, a negative length, two and
// three taxa, a caterpillar of the most taxa, and every refusal.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kaptive_amd.h"
#include "../../kaptive_amd/csrc/kp_nj.h"

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

static kp_nj_node node(int32_t a, int32_t b, int32_t c, double la, double lb, double lc) { return kp_nj_node{a, b, c, 0, la, lb, lc}; }
static bool same(const kp_nj_node &x, const kp_nj_node &y) { return std::memcmp(&x, &y, sizeof x) == 0; }

// the formatter on exact blocks: sized, then filled into exactly that much
static int64_t format(const std::string &locus, const std::vector<std::string> &names, const std::vector<int32_t> *rows, const std::vector<int32_t> &taxa,
                      const std::vector<kp_nj_node> &nodes, std::string *text) {
    std::vector<char> blob;
    std::vector<int64_t> off{0};
    for (const std::string &n : names) { blob.insert(blob.end(), n.begin(), n.end()); off.push_back((int64_t)blob.size()); }
    Exact<char> nb(blob), lc(std::vector<char>(locus.begin(), locus.end()));
    Exact<int64_t> no(off);
    Exact<int32_t> tx(taxa), rw(rows ? *rows : std::vector<int32_t>());
    Exact<kp_nj_node> nd(nodes);
    const int32_t n = (int32_t)names.size();
    const auto call = [&](char *out, int64_t cap) {
        return kp_format_nj(lc.p, (int32_t)locus.size(), nb.p, no.p, n, rows ? rw.p : nullptr, tx.p, (int32_t)taxa.size(), nd.p, (int64_t)nodes.size(), out, cap);
    };
    const int64_t need = call(nullptr, 0);
    if (need < 0) return need;
    Exact<char> out(std::vector<char>((size_t)need, '?'));
    CHECK(call(out.p, need) == need);
    if (need > 1) {
        Exact<char> shorter(std::vector<char>((size_t)need - 1, '?'));  // a buffer one byte short is not written past
        CHECK(call(shorter.p, need - 1) == need);
    }
    if (text) text->assign(out.p, (size_t)need);
    return need;
}

int main() {
    // ---- SUM64 against its definition
    for (int m : {0, 1, 63, 64, 65, 127, 128, 129, 200}) {
        std::vector<double> v((size_t)m);
        for (int k = 0; k < m; ++k) v[(size_t)k] = 1.0 / (double)(3 * k + 1);
        double s[64] = {0};
        for (int k = 0; k < m; ++k) s[k % 64] = s[k % 64] + v[(size_t)k];
        for (int o = 32; o >= 1; o >>= 1)
            for (int l = 0; l < o; ++l) s[l] = s[l] + s[l + o];
        Exact<double> e(v);
        CHECK(kp_nj_sum64(e.p, m) == s[0]);
    }
    // ---- the known answers
    {
        const std::vector<double> five{0, 5, 9, 9, 8, 5, 0, 10, 10, 9, 9, 10, 0, 8, 7, 9, 10, 8, 0, 3, 8, 9, 7, 3, 0};
        Exact<double> d(five);
        Exact<kp_nj_node> out(std::vector<kp_nj_node>(3));
        CHECK(kp_nj_host(d.p, 5, out.p) == 3);
        CHECK(same(out.p[0], node(0, 1, -1, 2, 3, 0)) && same(out.p[1], node(5, 2, -1, 3, 4, 0)) && same(out.p[2], node(6, 4, 3, 2, 1, 2)));
        Exact<double> zero(std::vector<double>(36, 0.0));
        Exact<kp_nj_node> out6(std::vector<kp_nj_node>(4));
        CHECK(kp_nj_host(zero.p, 6, out6.p) == 4);
        CHECK(same(out6.p[0], node(0, 1, -1, 0, 0, 0)) && same(out6.p[1], node(6, 5, -1, 0, 0, 0)) && same(out6.p[2], node(7, 4, -1, 0, 0, 0)) &&
              same(out6.p[3], node(8, 3, 2, 0, 0, 0)));
        Exact<kp_nj_node> none{std::vector<kp_nj_node>()};
        CHECK(kp_nj_host(d.p, 0, none.p) == 0 && kp_nj_host(d.p, 1, none.p) == 0);
        Exact<kp_nj_node> one(std::vector<kp_nj_node>(1));
        CHECK(kp_nj_host(d.p, 3, one.p) == 1 && one.p[0].a == 0 && one.p[0].b == 1 && one.p[0].c == 2);
        const std::vector<double> two{0, 3, 3, 0};
        Exact<double> d2(two);
        CHECK(kp_nj_host(d2.p, 2, one.p) == 1 && same(one.p[0], node(0, 1, -1, 1.5, 1.5, 0)));
    }
    // ---- the taxon rule at its edge: W = 64, min_compared = 2: 33 bases are in, 32 are out; bases in columns 0..32 and 31..63
    // compare in exactly two
    {
        CHECK(kp_nj_taxon(33, 64, 2) && !kp_nj_taxon(32, 64, 2) && kp_nj_taxon(33, 64, 1) && kp_nj_taxon(33, 64, 0) && !kp_nj_taxon(33, 64, 3));
        std::vector<uint64_t> m(3 * 4);
        const auto block = [](int from, int to, int b) {  // block b of a row that holds base a in columns [from, to) and GAP elsewhere
            uint64_t gap = 0;
            for (int k = 0; k < 16; ++k)
                if (16 * b + k < from || 16 * b + k >= to) gap |= 1ull << k;
            return gap << KP_DIST_GAP_SHIFT;
        };
        for (int b = 0; b < 4; ++b) { m[(size_t)b] = block(0, 33, b); m[4 + (size_t)b] = block(31, 64, b); m[8 + (size_t)b] = block(0, 32, b); }
        Exact<uint64_t> blocks(m);
        Exact<int32_t> taxa(std::vector<int32_t>(3, -9));
        CHECK(kp_nj_row_bases(blocks.p, 4) == 33 && kp_nj_row_bases(blocks.p + 8, 4) == 32);
        CHECK(kp_nj_matrix_host(blocks.p, 3, 4, 2, taxa.p, nullptr) == 2 && taxa.p[0] == 0 && taxa.p[1] == 1);
        Exact<double> D(std::vector<double>(4, -1.0));
        CHECK(kp_nj_matrix_host(blocks.p, 3, 4, 2, taxa.p, D.p) == 2 && D.p[0] == 0 && D.p[1] == 0 && D.p[2] == 0 && D.p[3] == 0);
        CHECK(kp_dist_row_counts(blocks.p, blocks.p + 4, 4).compared == 2);
    }
    // ---- the formatter
    std::string text;
    const std::vector<std::string> five{"a", "b", "c", "d", "e"};
    const std::vector<kp_nj_node> known{node(0, 1, -1, 2, 3, 0), node(5, 2, -1, 3, 4, 0), node(6, 4, 3, 2, 1, 2)};
    CHECK(format("K1", five, nullptr, {0, 1, 2, 3, 4}, known, &text) > 0 && text == "K1\t5\t5\t(((a:2,b:3):3,c:4):2,e:1,d:2);\n");
    const std::vector<int32_t> rows{4, 3, 2, 1, 0};
    CHECK(format("", five, &rows, {0, 1, 2, 3, 4}, known, &text) > 0 && text == "\t5\t5\t(((e:2,d:3):3,c:4):2,a:1,b:2);\n");
    CHECK(format("L", {"it's", "skipped", "two words", ""}, nullptr, {0, 2, 3}, {node(0, 1, 2, 1.0 / 3.0, -0.125, 1e-12)}, &text) > 0 &&
          text == "L\t4\t3\t('it''s':0.333333333,'two words':-0.125,:1e-12);\n");
    CHECK(format("L", {"x", "y"}, nullptr, {0, 1}, {node(0, 1, -1, 0.5, 0.5, 0)}, &text) > 0 && text == "L\t2\t2\t(x:0.5,y:0.5);\n");
    CHECK(format("L", {"x", "y"}, nullptr, {1}, {}, &text) == 0 && format("L", {}, nullptr, {}, {}, &text) == 0);
    {
        const int32_t n = KP_NJ_MAX_TAXA;  // a caterpillar of the most taxa: no recursion
        std::vector<std::string> names((size_t)n, "x");
        std::vector<int32_t> taxa((size_t)n);
        for (int32_t k = 0; k < n; ++k) taxa[(size_t)k] = k;
        std::vector<kp_nj_node> cat{node(0, 1, -1, 0, 0, 0)};
        for (int32_t r = 1; r < n - 3; ++r) cat.push_back(node(n + r - 1, r + 1, -1, 0, 0, 0));
        cat.push_back(node(2 * n - 4, n - 2, n - 1, 0, 0, 0));
        const std::string tail = "):0,x:0,x:0);\n";
        CHECK(format("L", names, nullptr, taxa, cat, &text) > 0 && std::count(text.begin(), text.end(), '(') == n - 2 &&
              text.compare(text.size() - tail.size(), tail.size(), tail) == 0);
    }
    const std::vector<int32_t> all{0, 1, 2, 3, 4};
    CHECK(format("x", five, nullptr, {0, 1, 2, 3, 5}, known, nullptr) == KP_EINVAL);                                                       // a taxon outside the rows
    CHECK(format("x", five, nullptr, {0, 1, 3, 2, 4}, known, nullptr) == KP_EINVAL);                                                       // taxa that do not ascend
    CHECK(format("x", five, nullptr, {0, 1, 2, 3}, known, nullptr) == KP_EINVAL);                                                          // records of another tree
    CHECK(format("x", five, nullptr, all, {known[0], known[1]}, nullptr) == KP_EINVAL);
    CHECK(format("x", five, nullptr, all, {node(0, 7, -1, 0, 0, 0), known[1], known[2]}, nullptr) == KP_EINVAL);                           // a node id outside the range
    CHECK(format("x", five, nullptr, all, {node(-1, 1, -1, 0, 0, 0), known[1], known[2]}, nullptr) == KP_EINVAL);
    CHECK(format("x", five, nullptr, all, {node(0, 5, -1, 0, 0, 0), known[1], known[2]}, nullptr) == KP_EINVAL);                           // a cycle: its own node
    CHECK(format("x", five, nullptr, all, {node(0, 6, -1, 0, 0, 0), known[1], known[2]}, nullptr) == KP_EINVAL);                           // ... a later one
    CHECK(format("x", five, nullptr, all, {known[0], node(5, 1, -1, 0, 0, 0), known[2]}, nullptr) == KP_EINVAL);                           // a child used twice
    CHECK(format("x", five, nullptr, all, {known[0], node(5, 5, -1, 0, 0, 0), known[2]}, nullptr) == KP_EINVAL);
    CHECK(format("x", five, nullptr, all, {node(0, 1, 2, 0, 0, 0), known[1], known[2]}, nullptr) == KP_EINVAL);                            // a third child before the end
    CHECK(format("x", five, nullptr, all, {known[0], known[1], node(6, 4, -1, 0, 0, 0)}, nullptr) == KP_EINVAL);                           // none at the end
    CHECK(format("x", {"x", "y"}, nullptr, {0, 1}, {node(0, 1, 0, 0, 0, 0)}, nullptr) == KP_EINVAL);
    const std::vector<int32_t> bad_rows{0, 1, 2, 3, 5};
    CHECK(format("x", five, &bad_rows, all, known, nullptr) == KP_EINVAL);
    CHECK(kp_format_nj("x", 1, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, 5) == KP_EINVAL);                            // room without a buffer
    CHECK(kp_format_nj(nullptr, 1, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, 0) == KP_EINVAL);
    if (fails) { std::fprintf(stderr, "%d checks failed\n", fails); return 1; }
    std::puts("nj_format_main: all checks passed");
    return 0;
}
