// pars_format_main.cpp -- a stand-alone program around kaptive_amd/csrc/kp_pars.h, kp_format_nj_homoplasy and kp_format_nj_changes, for
// a run under the host sanitizers (no GPU, nothing loaded into an interpreter):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -o pars_format_main
//       tests/native_harness/pars_format_main.cpp kaptive_amd/csrc/kp_rows.cpp && ./pars_format_main
// Every table is a heap block of exactly the size the call may read or write: an access past an end stops the program.  It checks the
// spec's known answers through kp_pars_host, a matrix with a short last plane word and a missing row, the check of a record list, and
// the two formatters: sized with cap 0, filled into a buffer of exactly the size returned, names that need quoting, an empty list,
// every refusal of their own.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kaptive_amd.h"
#include "../../kaptive_amd/csrc/kp_pars.h"

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

static kp_nj_node node(int32_t a, int32_t b, int32_t c) { return kp_nj_node{a, b, c, 0, 0.0, 0.0, 0.0}; }
static kp_pars_site site(int32_t column, int32_t steps, int32_t alleles) { return kp_pars_site{column, steps, alleles, 0}; }
static kp_pars_change change(int32_t column, int32_t v, int32_t parent, int from, int to) { return kp_pars_change{column, v, parent, (uint8_t)from, (uint8_t)to, 0}; }

// rows of text over acgtn- -> blocks, padded with GAP to whole blocks
static std::vector<uint64_t> pack(const std::vector<std::string> &rows, int64_t *nb) {
    *nb = ((int64_t)rows[0].size() + 15) / 16;
    std::vector<uint64_t> out(rows.size() * (size_t)*nb, 0);
    for (size_t r = 0; r < rows.size(); ++r)
        for (int64_t c = 0; c < 16 * *nb; ++c) {
            const char ch = c < (int64_t)rows[r].size() ? rows[r][(size_t)c] : '-';
            uint64_t &v = out[r * (size_t)*nb + (size_t)(c / 16)];
            const int j = (int)(c % 16);
            if (ch == '-') v |= 1ull << (KP_DIST_GAP_SHIFT + j);
            else if (ch == 'n') v |= 1ull << (KP_DIST_N_SHIFT + j);
            else v |= (uint64_t)(ch == 'a' ? 0 : ch == 'c' ? 1 : ch == 'g' ? 2 : 3) << (2 * j);
        }
    return out;
}

struct Names {
    std::vector<char> blob;
    std::vector<int64_t> off{0};
    explicit Names(const std::vector<std::string> &names) {
        for (const std::string &n : names) { blob.insert(blob.end(), n.begin(), n.end()); off.push_back((int64_t)blob.size()); }
    }
};

static int64_t homoplasy(const std::vector<std::string> &genes, const std::vector<int32_t> &gene_len, const std::vector<kp_pars_site> &sites, std::string *text) {
    const Names g(genes);
    Exact<char> gb(g.blob);
    Exact<int64_t> go(g.off);
    Exact<int32_t> gl(gene_len);
    Exact<kp_pars_site> st(sites);
    const auto call = [&](char *out, int64_t cap) { return kp_format_nj_homoplasy("L", 1, gb.p, go.p, (int32_t)genes.size(), nullptr, gl.p, st.p, (int64_t)sites.size(), out, cap); };
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

static int64_t changes_of(const std::vector<std::string> &names, const std::vector<int32_t> &taxa, const std::vector<kp_nj_node> &nodes, const std::vector<std::string> &genes,
                          const std::vector<int32_t> &gene_len, const std::vector<kp_pars_change> &changes, std::string *text) {
    const Names nm(names), g(genes);
    Exact<char> nb(nm.blob), gb(g.blob);
    Exact<int64_t> no(nm.off), go(g.off);
    Exact<int32_t> tx(taxa), gl(gene_len);
    Exact<kp_nj_node> nd(nodes);
    Exact<kp_pars_change> ch(changes);
    const auto call = [&](char *out, int64_t cap) {
        return kp_format_nj_changes("L", 1, nb.p, no.p, (int32_t)names.size(), nullptr, tx.p, (int32_t)taxa.size(), nd.p, (int64_t)nodes.size(), gb.p, go.p, (int32_t)genes.size(),
                                    nullptr, gl.p, ch.p, (int64_t)changes.size(), out, cap);
    };
    const int64_t need = call(nullptr, 0);
    if (need < 0) return need;
    Exact<char> out(std::vector<char>((size_t)need, '?'));
    CHECK(call(out.p, need) == need);
    if (need > 1) {
        Exact<char> shorter(std::vector<char>((size_t)need - 1, '?'));
        CHECK(call(shorter.p, need - 1) == need);
    }
    if (text) text->assign(out.p, (size_t)need);
    return need;
}

int main() {
    const std::vector<kp_nj_node> five{node(0, 1, -1), node(5, 2, -1), node(6, 4, 3)};
    // ---- the known answers of the spec: the columns aaaaa ccaaa gagaa ccctg ccnaa as columns 0 .. 4 of five rows
    {
        int64_t nb = 0;
        Exact<uint64_t> blocks(pack({"acgcc", "acacc", "aagcn", "aaata", "aaaga"}, &nb));
        Exact<int32_t> taxa(std::vector<int32_t>{0, 1, 2, 3, 4});
        Exact<kp_nj_node> rec(five);
        std::vector<kp_pars_site> s;
        std::vector<kp_pars_change> c;
        kp_pars_host(blocks.p, nb, taxa.p, 5, rec.p, 3, &s, &c);
        CHECK(s.size() == 4 && c.size() == 6);
        if (s.size() == 4 && c.size() == 6) {
            const kp_pars_site want[4] = {site(1, 1, 3), site(2, 2, 5), site(3, 2, 14), site(4, 1, 3)};
            CHECK(std::memcmp(s.data(), want, sizeof want) == 0);
            const kp_pars_change wc[6] = {change(2, 1, 5, 2, 0), change(3, 3, 7, 1, 3), change(3, 4, 7, 1, 2), change(1, 5, 6, 0, 1), change(2, 6, 7, 0, 2), change(4, 6, 7, 0, 1)};
            CHECK(std::memcmp(c.data(), wc, sizeof wc) == 0);
        }
    }
    {  // two taxa, a short last plane word (five blocks: two words), a third row that is no taxon
        int64_t nb = 0;
        std::string x(70, 'a'), y(70, 'a'), z(70, '-');
        y[0] = 'c'; y[63] = 'g'; y[64] = 't'; y[69] = 'c'; x[5] = 'n';
        Exact<uint64_t> blocks(pack({x, z, y}, &nb));
        CHECK(nb == 5);
        Exact<int32_t> taxa(std::vector<int32_t>{0, 2});
        Exact<kp_nj_node> rec(std::vector<kp_nj_node>{node(0, 1, -1)});
        std::vector<kp_pars_site> s;
        std::vector<kp_pars_change> c;
        kp_pars_host(blocks.p, nb, taxa.p, 2, rec.p, 1, &s, &c);
        CHECK(s.size() == 4 && c.size() == 4 && s[0].column == 0 && s[1].column == 63 && s[2].column == 64 && s[3].column == 69 && s[3].steps == 1 && s[3].alleles == 3);
        for (const kp_pars_change &r : c) CHECK(r.node == 1 && r.parent == 2 && r.from == 0);  // the top takes a, the smaller code; taxon 1 carries the change
    }
    // ---- the check of a record list
    {
        Exact<kp_nj_node> ok(five);
        std::vector<int32_t> up(8, -9);
        CHECK(kp_pars_tree_ok(ok.p, 3, 5, up.data()) && up[0] == 5 && up[1] == 5 && up[2] == 6 && up[5] == 6 && up[3] == 7 && up[4] == 7 && up[6] == 7 && up[7] == -1);
        CHECK(!kp_pars_tree_ok(ok.p, 3, 4, nullptr) && !kp_pars_tree_ok(ok.p, 2, 5, nullptr) && kp_pars_tree_ok(nullptr, 0, 0, nullptr) && kp_pars_tree_ok(nullptr, 0, 1, nullptr));
        Exact<kp_nj_node> twice(std::vector<kp_nj_node>{node(0, 1, -1), node(5, 1, -1), node(6, 4, 3)});
        Exact<kp_nj_node> forward(std::vector<kp_nj_node>{node(0, 6, -1), node(5, 2, -1), node(1, 4, 3)});
        Exact<kp_nj_node> middle(std::vector<kp_nj_node>{node(0, 1, 2), node(5, 3, -1), node(6, 4, -1)});
        Exact<kp_nj_node> outside(std::vector<kp_nj_node>{node(-1, 99, -1), node(5, 2, -1), node(6, 4, 3)});
        CHECK(!kp_pars_tree_ok(twice.p, 3, 5, nullptr) && !kp_pars_tree_ok(forward.p, 3, 5, nullptr) && !kp_pars_tree_ok(middle.p, 3, 5, nullptr) && !kp_pars_tree_ok(outside.p, 3, 5, nullptr));
        Exact<kp_nj_node> two(std::vector<kp_nj_node>{node(0, 1, -1)}), three(std::vector<kp_nj_node>{node(0, 1, 2)});
        CHECK(kp_pars_tree_ok(two.p, 1, 2, nullptr) && kp_pars_tree_ok(three.p, 1, 3, nullptr) && !kp_pars_tree_ok(two.p, 1, 3, nullptr) && !kp_pars_tree_ok(three.p, 1, 2, nullptr));
        CHECK(kp_pars_taxa_of(two.p, 1) == 2 && kp_pars_taxa_of(three.p, 1) == 3 && kp_pars_taxa_of(ok.p, 3) == 5 && kp_pars_taxa_of(nullptr, 0) == 0);
    }
    // ---- the formatters: two genes of 20 and 5 bases, the second from matrix column 32 on
    const std::vector<std::string> genes{"wzi", "wca J"};
    const std::vector<int32_t> lens{20, 5};
    std::string text;
    CHECK(homoplasy(genes, lens, {site(1, 1, 3), site(19, 2, 5), site(32, 3, 15), site(36, 2, 14)}, &text) > 0 &&
          text == "L\twzi\t2\t2\t2\t1\t0\nL\twzi\t20\t20\t2\t2\t1\nL\twca J\t1\t21\t4\t3\t0\nL\twca J\t5\t25\t3\t2\t0\n");
    CHECK(homoplasy(genes, lens, {}, &text) == 0);
    CHECK(homoplasy(genes, lens, {site(20, 1, 3)}, nullptr) == KP_EINVAL && homoplasy(genes, lens, {site(37, 1, 3)}, nullptr) == KP_EINVAL);   // padding
    CHECK(homoplasy(genes, lens, {site(48, 1, 3)}, nullptr) == KP_EINVAL && homoplasy(genes, lens, {site(-1, 1, 3)}, nullptr) == KP_EINVAL);   // outside
    CHECK(homoplasy(genes, lens, {site(1, 1, 1)}, nullptr) == KP_EINVAL && homoplasy(genes, lens, {site(1, 1, 7)}, nullptr) == KP_EINVAL);     // one base; too few steps
    CHECK(homoplasy(genes, lens, {site(1, 1, 19)}, nullptr) == KP_EINVAL && homoplasy(genes, lens, {site(2, 1, 3), site(2, 1, 3)}, nullptr) == KP_EINVAL);
    CHECK(homoplasy(genes, {20, -1}, {site(1, 1, 3)}, nullptr) == KP_EINVAL);
    CHECK(kp_format_nj_homoplasy("x", 1, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, 5) == KP_EINVAL);  // room without a buffer
    CHECK(kp_format_nj_homoplasy("x", 1, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 1, nullptr, 0) == KP_EINVAL);  // records without a table
    const std::vector<std::string> names{"a", "it's", "two words", "d", "skipped", "e"};
    const std::vector<int32_t> taxa{0, 1, 2, 3, 5};
    CHECK(changes_of(names, taxa, five, genes, lens, {change(2, 1, 5, 2, 0), change(3, 3, 7, 1, 3), change(1, 5, 6, 0, 1), change(32, 6, 7, 0, 2)}, &text) > 0 &&
          text == "L\t'it''s'\t'it''s'\t.\t1\twzi\t3\t3\tg\ta\nL\td\td\t.\t1\twzi\t4\t4\tc\tt\nL\t#1\ta\t'it''s'\t2\twzi\t2\t2\ta\tc\nL\t#2\ta\t'two words'\t3\twca J\t1\t21\ta\tg\n");
    CHECK(changes_of(names, taxa, five, genes, lens, {}, &text) == 0);
    CHECK(changes_of(names, taxa, five, genes, lens, {change(2, 7, -1, 2, 0)}, nullptr) == KP_EINVAL && changes_of(names, taxa, five, genes, lens, {change(2, -1, 5, 2, 0)}, nullptr) == KP_EINVAL);
    CHECK(changes_of(names, taxa, five, genes, lens, {change(2, 1, 6, 2, 0)}, nullptr) == KP_EINVAL && changes_of(names, taxa, five, genes, lens, {change(2, 1, 5, 2, 2)}, nullptr) == KP_EINVAL);
    CHECK(changes_of(names, taxa, five, genes, lens, {change(2, 1, 5, 4, 0)}, nullptr) == KP_EINVAL && changes_of(names, taxa, five, genes, lens, {change(20, 1, 5, 2, 0)}, nullptr) == KP_EINVAL);
    CHECK(changes_of(names, taxa, five, genes, lens, {change(2, 1, 5, 2, 0), change(2, 1, 5, 2, 0)}, nullptr) == KP_EINVAL);
    CHECK(changes_of(names, taxa, five, genes, lens, {change(2, 3, 7, 2, 0), change(3, 1, 5, 2, 0)}, nullptr) == KP_EINVAL);
    CHECK(changes_of(names, {0, 1, 2, 3}, five, genes, lens, {}, nullptr) == KP_EINVAL && changes_of(names, {0, 1, 3, 2, 5}, five, genes, lens, {}, nullptr) == KP_EINVAL);
    CHECK(changes_of(names, taxa, {node(0, 1, -1), node(5, 5, -1), node(6, 4, 3)}, genes, lens, {}, nullptr) == KP_EINVAL);  // a node that is a child twice
    CHECK(changes_of({"x", "y"}, {0, 1}, {node(0, 1, -1)}, genes, lens, {change(0, 1, 2, 0, 3)}, &text) > 0 && text == "L\ty\ty\t.\t1\twzi\t1\t1\ta\tt\n");
    CHECK(changes_of({"x"}, {0}, {}, genes, lens, {}, &text) == 0);
    if (fails) return 1;
    std::puts("pars_format_main: all checks passed");
    return 0;
}
