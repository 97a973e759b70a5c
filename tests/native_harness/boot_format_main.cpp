// boot_format_main.cpp -- a stand-alone program around kaptive_amd/csrc/kp_boot.h and kp_format_nj_support, for a run under the host
// sanitizers (no GPU, nothing loaded into an interpreter):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -o boot_format_main
//       tests/native_harness/boot_format_main.cpp kaptive_amd/csrc/kp_rows.cpp && ./boot_format_main
// Every table is a heap block of exactly the size the call may read or write: an access past an end stops the program.  It checks the
// mixer's known answer, the draws and weights at one block and at a ragged last plane word, the weight planes, the weighted counts
// against a column loop, the walk over the records of kp_nj_host's trees against sets, the batch rule at its edges, and the formatter:
// sized with cap 0, filled into a buffer of exactly the size returned, labels at the inner edges only, and every refusal of its own.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../include/kaptive_amd.h"
#include "../../kaptive_amd/csrc/kp_boot.h"

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

static int64_t format(const std::vector<std::string> &names, const std::vector<int32_t> &taxa, const std::vector<kp_nj_node> &nodes, const std::vector<int32_t> &support,
                      int32_t replicates, std::string *text) {
    std::vector<char> blob;
    std::vector<int64_t> off{0};
    for (const std::string &n : names) { blob.insert(blob.end(), n.begin(), n.end()); off.push_back((int64_t)blob.size()); }
    Exact<char> nb(blob);
    Exact<int64_t> no(off);
    Exact<int32_t> tx(taxa), sp(support);
    Exact<kp_nj_node> nd(nodes);
    const auto call = [&](char *out, int64_t cap) {
        return kp_format_nj_support("L", 1, nb.p, no.p, (int32_t)names.size(), nullptr, tx.p, (int32_t)taxa.size(), nd.p, (int64_t)nodes.size(), sp.p, replicates, out, cap);
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
    // ---- the mixer: SplitMix64's first output for the state 0
    CHECK(kp_boot_mix(0) == 0xe220a8397b1dcdafull);
    CHECK(kp_boot_mulhi64(~0ull, 16) == 15 && kp_boot_mulhi64(0, 16) == 0 && kp_boot_mulhi64(1ull << 63, 528) == 264);
    // ---- draws, weights and planes
    for (int64_t W : {16, 64, 80, 16 * 33}) {
        for (uint64_t seed : {0ull, 1ull, ~0ull}) {
            Exact<uint8_t> w(std::vector<uint8_t>((size_t)W, 9));
            kp_boot_weights_host(seed, 9999, W, w.p);
            int64_t sum = 0;
            for (int64_t c = 0; c < W; ++c) sum += w.p[c];
            CHECK(sum == W);
            const uint64_t stream = kp_boot_stream(seed, 9999);
            for (int64_t t = 0; t < W; ++t) { const int64_t c = kp_boot_draw(stream, (uint64_t)t, W); CHECK(c >= 0 && c < W); }
            for (int64_t word = 0; word < (W + 63) / 64; ++word) {
                uint64_t M[KP_BOOT_PLANES];
                const int top = kp_boot_word_planes(w.p, W, word, M);
                for (int b = 0; b < 64; ++b) {
                    uint32_t v = 0;
                    for (int k = 0; k < KP_BOOT_PLANES; ++k) v |= (uint32_t)((M[k] >> b) & 1) << k;
                    CHECK(v == (64 * word + b < W ? w.p[64 * word + b] : 0u) && (v >> top) == 0);
                }
            }
        }
    }
    CHECK(kp_boot_weight(254) == 254 && kp_boot_weight(255) == 255 && kp_boot_weight(256) == 255 && kp_boot_weight(1000) == 255 && kp_boot_weight(0) == 0);
    // ---- weighted counts of two rows of five blocks against a column loop
    {
        const int64_t nb = 5, W = 16 * nb;
        std::vector<uint64_t> a((size_t)nb), b((size_t)nb);
        uint64_t x = 7;
        for (int64_t k = 0; k < nb; ++k) {
            x = kp_boot_mix(x); a[(size_t)k] = (x & 0xffffffffull) | ((x >> 40 & 0x0101ull) << 32) | ((x >> 50 & 0x8001ull) << 48);
            x = kp_boot_mix(x); b[(size_t)k] = (x & 0xffffffffull) | ((x >> 40 & 0x1010ull) << 32) | ((x >> 50 & 0x4002ull) << 48);
        }
        Exact<uint64_t> ea(a), eb(b);
        std::vector<uint8_t> w((size_t)W);
        for (int64_t c = 0; c < W; ++c) w[(size_t)c] = (uint8_t)(kp_boot_mix((uint64_t)c) % 256);
        Exact<uint8_t> ew(w);
        int32_t cmp = 0, dif = 0;
        for (int64_t c = 0; c < W; ++c) {
            const auto code = [c](const std::vector<uint64_t> &r) {
                const uint64_t v = r[(size_t)(c / 16)];
                const int j = (int)(c % 16);
                return ((v >> (32 + j)) & 1) || ((v >> (48 + j)) & 1) ? -1 : (int)((v >> (2 * j)) & 3);
            };
            const int ca = code(a), cb = code(b);
            if (ca >= 0 && cb >= 0) { cmp += w[(size_t)c]; if (ca != cb) dif += w[(size_t)c]; }
        }
        const KpDistCounts got = kp_boot_row_counts(ea.p, eb.p, nb, ew.p);
        CHECK(got.compared == cmp && got.differences == dif && cmp > 0 && dif > 0);
    }
    // ---- the walk against sets, on the trees of kp_nj_host
    for (int32_t n : {4, 5, 9, 70}) {
        std::vector<double> D((size_t)n * (size_t)n, 0.0);
        uint64_t x = (uint64_t)n;
        for (int32_t a = 0; a < n; ++a)
            for (int32_t b = a + 1; b < n; ++b) { x = kp_boot_mix(x); D[(size_t)a * n + b] = D[(size_t)b * n + a] = (double)(x % 12) / (double)(40 + x % 4); }
        Exact<double> ed(D);
        Exact<kp_nj_node> rec(std::vector<kp_nj_node>((size_t)n - 2));
        CHECK(kp_nj_host(ed.p, n, rec.p) == n - 2);
        Exact<KpBootSplit> out(std::vector<KpBootSplit>((size_t)n - 3));
        const uint64_t total = kp_boot_total_key(n);
        kp_boot_walk(rec.p, n, total, out.p);
        std::vector<std::set<int32_t>> below((size_t)(2 * n));
        for (int32_t k = 0; k < n; ++k) below[(size_t)k] = {k};
        for (int32_t t = 0; t < n - 3; ++t) {
            std::set<int32_t> s = below[(size_t)rec.p[t].a];
            s.insert(below[(size_t)rec.p[t].b].begin(), below[(size_t)rec.p[t].b].end());
            below[(size_t)(n + t)] = s;
            const bool has0 = s.count(0) != 0;
            uint64_t key = 0;
            int32_t size = 0;
            for (int32_t k = 0; k < n; ++k)
                if ((s.count(k) != 0) != has0) { key += kp_boot_taxon_key(k); ++size; }
            CHECK(out.p[t].key == key && out.p[t].size == size && out.p[t].has0 == (has0 ? 1 : 0));
        }
    }
    {  // a record list with ids out of range is walked without a read outside it
        Exact<kp_nj_node> bad(std::vector<kp_nj_node>{node(-1, 99, -1, 0, 0, 0), node(5, 7, -1, 0, 0, 0), node(0, 1, 2, 0, 0, 0)});
        Exact<KpBootSplit> out(std::vector<KpBootSplit>(2));
        kp_boot_walk(bad.p, 5, kp_boot_total_key(5), out.p);
        CHECK(out.p[0].size == 0 && out.p[1].size == 0);
    }
    // ---- the batch rule
    CHECK(kp_boot_batch(16384, 100, 0) == 1 && kp_boot_batch(11585, 100, 0) == 2 && kp_boot_batch(11586, 100, 0) == 1 && kp_boot_batch(4, 10000, 0) == 10000);
    CHECK(kp_boot_batch(1024, 10000, 0) == 256 && kp_boot_batch(1024, 100, 7) == 7 && kp_boot_batch(0, 5, 0) == 5 && kp_boot_batch(20000, 5, 0) == 1);
    // ---- the formatter
    const std::vector<std::string> five{"a", "b", "c", "d", "e"};
    const std::vector<int32_t> all5{0, 1, 2, 3, 4};
    const std::vector<kp_nj_node> known{node(0, 1, -1, 2, 3, 0), node(5, 2, -1, 3, 4, 0), node(6, 4, 3, 2, 1, 2)};
    std::string text;
    CHECK(format(five, all5, known, {87, 0, -1}, 100, &text) > 0 && text == "L\t5\t5\t100\t(((a:2,b:3)87:3,c:4)0:2,e:1,d:2);\n");
    CHECK(format(five, all5, known, {10000, 10000, -1}, 10000, &text) > 0 && text == "L\t5\t5\t10000\t(((a:2,b:3)10000:3,c:4)10000:2,e:1,d:2);\n");
    CHECK(format({"x", "y"}, {0, 1}, {node(0, 1, -1, 0.5, 0.5, 0)}, {-1}, 3, &text) > 0 && text == "L\t2\t2\t3\t(x:0.5,y:0.5);\n");
    CHECK(format({"x", "y", "z"}, {0, 1, 2}, {node(0, 1, 2, 1, 2, 3)}, {-1}, 1, &text) > 0 && text == "L\t3\t3\t1\t(x:1,y:2,z:3);\n");
    CHECK(format({"x"}, {0}, {}, {}, 5, &text) == 0);
    CHECK(format(five, all5, known, {1, 1, -1}, 0, nullptr) == KP_EINVAL && format(five, all5, known, {1, 1, -1}, 10001, nullptr) == KP_EINVAL);
    CHECK(format(five, all5, known, {5, 1, -1}, 4, nullptr) == KP_EINVAL && format(five, all5, known, {-1, 1, -1}, 4, nullptr) == KP_EINVAL);
    CHECK(format(five, all5, known, {1, 1, 0}, 4, nullptr) == KP_EINVAL && format(five, {0, 1, 2, 3}, known, {1, 1, -1}, 4, nullptr) == KP_EINVAL);
    CHECK(kp_format_nj_support("x", 1, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, 3, nullptr, 5) == KP_EINVAL);  // room without a buffer
    {
        Exact<kp_nj_node> nd(known);
        Exact<int32_t> tx(all5);
        Exact<int64_t> no(std::vector<int64_t>{0, 1, 2, 3, 4, 5});
        Exact<char> nb(std::vector<char>{'a', 'b', 'c', 'd', 'e'});
        CHECK(kp_format_nj_support("x", 1, nb.p, no.p, 5, nullptr, tx.p, 5, nd.p, 3, nullptr, 3, nullptr, 0) == KP_EINVAL);  // records without support
    }
    if (fails) return 1;
    std::puts("boot_format_main: all checks passed");
    return 0;
}
