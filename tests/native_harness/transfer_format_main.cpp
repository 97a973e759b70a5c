// transfer_format_main.cpp -- a stand-alone program around kaptive_amd/csrc/kp_transfer.h and kp_format_nj_transfer, for a run under the
// host sanitizers (no GPU, nothing loaded into an interpreter):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -o transfer_format_main
//       tests/native_harness/transfer_format_main.cpp kaptive_amd/csrc/kp_rows.cpp && ./transfer_format_main
// Every table is a heap block of exactly the size the call may read or write: an access past an end stops the program.  It checks the
// distance of two splits from either side, the spec's known answer through kp_transfer_host, the transfer distances of kp_nj_host's
// trees against a set loop of its own, a record list with ids out of range, the label's thousandths at their edges, and the
// formatter: sized with cap 0, filled into a buffer of exactly the size returned, labels at the inner edges only, every refusal of its
// own.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../include/kaptive_amd.h"
#include "../../kaptive_amd/csrc/kp_transfer.h"

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

static int64_t format(const std::vector<std::string> &names, const std::vector<int32_t> &taxa, const std::vector<kp_nj_node> &nodes, const std::vector<int64_t> &transfer,
                      int32_t replicates, std::string *text) {
    std::vector<char> blob;
    std::vector<int64_t> off{0};
    for (const std::string &n : names) { blob.insert(blob.end(), n.begin(), n.end()); off.push_back((int64_t)blob.size()); }
    Exact<char> nb(blob);
    Exact<int64_t> no(off), tr(transfer);
    Exact<int32_t> tx(taxa);
    Exact<kp_nj_node> nd(nodes);
    const auto call = [&](char *out, int64_t cap) {
        return kp_format_nj_transfer("L", 1, nb.p, no.p, (int32_t)names.size(), nullptr, tx.p, (int32_t)taxa.size(), nd.p, (int64_t)nodes.size(), tr.p, replicates, out, cap);
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

// the sets below every record's node, for the loop that restates phi
static std::vector<std::set<int32_t>> below_sets(const kp_nj_node *rec, int32_t n) {
    std::vector<std::set<int32_t>> below((size_t)(2 * n));
    for (int32_t k = 0; k < n; ++k) below[(size_t)k] = {k};
    for (int32_t t = 0; t < n - 3; ++t) {
        below[(size_t)(n + t)] = below[(size_t)rec[t].a];
        below[(size_t)(n + t)].insert(below[(size_t)rec[t].b].begin(), below[(size_t)rec[t].b].end());
    }
    return below;
}

int main() {
    // ---- depth and distance
    CHECK(kp_transfer_depth(2, 6) == 2 && kp_transfer_depth(4, 6) == 2 && kp_transfer_depth(3, 6) == 3 && kp_transfer_depth(8192, 16384) == 8192);
    CHECK(kp_transfer_delta(4, 4, 3, 6) == 2 && kp_transfer_delta(2, 4, 1, 6) == 2 && kp_transfer_delta(4, 2, 1, 6) == 2 && kp_transfer_delta(2, 2, 1, 6) == 2);  // {2,3,4,5} and {1,2,4,5}, every side
    CHECK(kp_transfer_delta(3, 3, 3, 8) == 0 && kp_transfer_delta(3, 5, 0, 8) == 0 && kp_transfer_delta(8192, 8192, 0, 16384) == 0 && kp_transfer_delta(8192, 8192, 4096, 16384) == 8192);
    // ---- the known answer of the spec
    {
        Exact<kp_nj_node> ref(std::vector<kp_nj_node>{node(0, 1, -1, 0, 0, 0), node(6, 2, -1, 0, 0, 0), node(7, 3, -1, 0, 0, 0), node(8, 4, 5, 0, 0, 0)});
        Exact<kp_nj_node> rep(std::vector<kp_nj_node>{node(0, 3, -1, 0, 0, 0), node(6, 1, -1, 0, 0, 0), node(7, 2, -1, 0, 0, 0), node(8, 4, 5, 0, 0, 0)});
        Exact<int32_t> phi(std::vector<int32_t>(3, -9)), size(std::vector<int32_t>(3, -9));
        kp_transfer_host(ref.p, rep.p, 6, phi.p);
        CHECK(phi.p[0] == 1 && phi.p[1] == 1 && phi.p[2] == 0);
        kp_transfer_host(ref.p, ref.p, 6, phi.p);
        CHECK(phi.p[0] == 0 && phi.p[1] == 0 && phi.p[2] == 0);
        kp_transfer_sizes(ref.p, 6, size.p);
        CHECK(size.p[0] == 2 && size.p[1] == 3 && size.p[2] == 4);
        CHECK(kp_transfer_label(1, 1, 2) == 0 && kp_transfer_label(1, 1, 3) == 500 && kp_transfer_label(0, 1, 2) == 1000);
    }
    // ---- the transfer distances of kp_nj_host's trees against sets
    for (int32_t n : {4, 5, 9, 70}) {
        std::vector<Exact<kp_nj_node> *> trees;
        for (uint64_t salt : {1ull, 2ull}) {
            std::vector<double> D((size_t)n * (size_t)n, 0.0);
            uint64_t x = (uint64_t)n * salt;
            for (int32_t a = 0; a < n; ++a)
                for (int32_t b = a + 1; b < n; ++b) { x = kp_boot_mix(x); D[(size_t)a * n + b] = D[(size_t)b * n + a] = (double)(x % 12) / (double)(40 + x % 4); }
            Exact<double> ed(D);
            trees.push_back(new Exact<kp_nj_node>(std::vector<kp_nj_node>((size_t)n - 2)));
            CHECK(kp_nj_host(ed.p, n, trees.back()->p) == n - 2);
        }
        Exact<int32_t> phi(std::vector<int32_t>((size_t)n - 3, -9));
        kp_transfer_host(trees[0]->p, trees[1]->p, n, phi.p);
        const std::vector<std::set<int32_t>> ours = below_sets(trees[0]->p, n), theirs = below_sets(trees[1]->p, n);
        for (int32_t t = 0; t < n - 3; ++t) {
            const std::set<int32_t> &A = ours[(size_t)(n + t)];
            const int32_t s = (int32_t)A.size();
            int32_t best = std::min(s, n - s) - 1;
            for (int32_t u = 0; u < n - 3; ++u) {
                int32_t h = 0;
                for (int32_t k = 0; k < n; ++k) h += (A.count(k) != 0) != (theirs[(size_t)(n + u)].count(k) != 0);
                best = std::min(best, std::min(h, n - h));
            }
            CHECK(phi.p[t] == best);
        }
        for (Exact<kp_nj_node> *t : trees) delete t;
    }
    {  // a record list with ids out of range is walked without a read outside it
        Exact<kp_nj_node> bad(std::vector<kp_nj_node>{node(-1, 99, -1, 0, 0, 0), node(5, 7, -1, 0, 0, 0), node(0, 1, 2, 0, 0, 0)});
        Exact<kp_nj_node> good(std::vector<kp_nj_node>{node(0, 1, -1, 0, 0, 0), node(5, 2, -1, 0, 0, 0), node(6, 3, 4, 0, 0, 0)});
        Exact<int32_t> phi(std::vector<int32_t>(2, -9)), size(std::vector<int32_t>(2, -9));
        kp_transfer_sizes(bad.p, 5, size.p);
        CHECK(size.p[0] == 0 && size.p[1] == 0);
        kp_transfer_host(good.p, bad.p, 5, phi.p);
        CHECK(phi.p[0] == 1 && phi.p[1] == 1);  // (empty sets are a whole light side away: the cap, depth - 1, stands)
    }
    // ---- the label at its edges
    CHECK(kp_transfer_label(0, 7, 3) == 1000 && kp_transfer_label(14, 7, 3) == 0 && kp_transfer_label(7, 7, 3) == 500);
    CHECK(kp_transfer_label(7, 5, 4) == 533 && kp_transfer_label(8, 5, 4) == 467);  // D = 15: 2 * transfer = D - 1, D + 1
    CHECK(kp_transfer_label(0, 10000, 8192) == 1000 && kp_transfer_label(81910000, 10000, 8192) == 0 && kp_transfer_label(40955000, 10000, 8192) == 500);
    CHECK(kp_transfer_label(40955, 10000, 8192) == 1000 && kp_transfer_label(40956, 10000, 8192) == 999);  // 0.9995 rounds up; beyond it down
    // ---- the formatter
    const std::vector<std::string> five{"a", "b", "c", "d", "e"};
    const std::vector<int32_t> all5{0, 1, 2, 3, 4};
    const std::vector<kp_nj_node> known{node(0, 1, -1, 2, 3, 0), node(5, 2, -1, 3, 4, 0), node(6, 4, 3, 2, 1, 2)};  // depths 2, 2
    std::string text;
    CHECK(format(five, all5, known, {13, 0, -1}, 100, &text) > 0 && text == "L\t5\t5\t100\t(((a:2,b:3)0.870:3,c:4)1.000:2,e:1,d:2);\n");
    CHECK(format(five, all5, known, {10000, 1, -1}, 10000, &text) > 0 && text == "L\t5\t5\t10000\t(((a:2,b:3)0.000:3,c:4)1.000:2,e:1,d:2);\n");
    const std::vector<std::string> six{"a", "b", "c", "d", "e", "f"};
    const std::vector<kp_nj_node> ref6{node(0, 1, -1, 0, 0, 0), node(6, 2, -1, 0, 0, 0), node(7, 3, -1, 0, 0, 0), node(8, 4, 5, 0, 0, 0)};  // depths 2, 3, 2
    CHECK(format(six, {0, 1, 2, 3, 4, 5}, ref6, {1, 1, 0, -1}, 1, &text) > 0 && text == "L\t6\t6\t1\t((((a:0,b:0)0.000:0,c:0)0.500:0,d:0)1.000:0,e:0,f:0);\n");
    CHECK(format(six, {0, 1, 2, 3, 4, 5}, ref6, {3, 6, 3, -1}, 3, nullptr) > 0);
    CHECK(format(six, {0, 1, 2, 3, 4, 5}, ref6, {4, 6, 3, -1}, 3, nullptr) == KP_EINVAL && format(six, {0, 1, 2, 3, 4, 5}, ref6, {3, 7, 3, -1}, 3, nullptr) == KP_EINVAL);
    CHECK(format({"x", "y"}, {0, 1}, {node(0, 1, -1, 0.5, 0.5, 0)}, {-1}, 3, &text) > 0 && text == "L\t2\t2\t3\t(x:0.5,y:0.5);\n");
    CHECK(format({"x", "y", "z"}, {0, 1, 2}, {node(0, 1, 2, 1, 2, 3)}, {-1}, 1, &text) > 0 && text == "L\t3\t3\t1\t(x:1,y:2,z:3);\n");
    CHECK(format({"x"}, {0}, {}, {}, 5, &text) == 0);
    CHECK(format(five, all5, known, {1, 1, -1}, 0, nullptr) == KP_EINVAL && format(five, all5, known, {1, 1, -1}, 10001, nullptr) == KP_EINVAL);
    CHECK(format(five, all5, known, {5, 1, -1}, 4, nullptr) == KP_EINVAL && format(five, all5, known, {-1, 1, -1}, 4, nullptr) == KP_EINVAL);
    CHECK(format(five, all5, known, {1, 1, 0}, 4, nullptr) == KP_EINVAL && format(five, {0, 1, 2, 3}, known, {1, 1, -1}, 4, nullptr) == KP_EINVAL);
    CHECK(format(five, all5, {node(0, 1, -1, 0, 0, 0), node(5, 5, -1, 0, 0, 0), node(6, 4, 3, 0, 0, 0)}, {1, 1, -1}, 4, nullptr) == KP_EINVAL);  // a node that is a child twice
    CHECK(kp_format_nj_transfer("x", 1, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, 3, nullptr, 5) == KP_EINVAL);  // room without a buffer
    {
        Exact<kp_nj_node> nd(known);
        Exact<int32_t> tx(all5);
        Exact<int64_t> no(std::vector<int64_t>{0, 1, 2, 3, 4, 5});
        Exact<char> nb(std::vector<char>{'a', 'b', 'c', 'd', 'e'});
        CHECK(kp_format_nj_transfer("x", 1, nb.p, no.p, 5, nullptr, tx.p, 5, nd.p, 3, nullptr, 3, nullptr, 0) == KP_EINVAL);  // records without sums
    }
    if (fails) return 1;
    std::puts("transfer_format_main: all checks passed");
    return 0;
}
