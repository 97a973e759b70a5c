// cigar_harness.cpp -- test infrastructure for tests/test_cigar_cpu.py and tests/test_gpu_cigar.py (g++, no GPU):
//   * kpy_band: the banded local alignment of include/kp_spec.h ("banded local alignment") restated cell by cell, with its
//     tie rules and the traceback, returning the result fields AND the run-length ops of the path -- the yardstick the
//     device's CIGARs are compared with.  It shares no code with the kernels or with oracle/kp_oracle.c: three full
//     matrices, one scalar loop.
//   * kpy_cigar_*: the CIGAR part of the buffer-size policy (kaptive_amd/csrc/kp_caps.h).
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kp_spec.h"
#include "../../kaptive_amd/csrc/kp_caps.h"

namespace {

constexpr int NEG = -(1 << 28);

inline int sub_score(int q, int t) { return (q > 3 || t > 3) ? KP_SC_N : (q == t ? KP_SC_MATCH : KP_SC_MISMATCH); }

}  // namespace

extern "C" {

// gene: codes 0..4 of the query AS ALIGNED (the reverse complement for strand -1); asm_codes: codes 0..4 of the assembly's
// padded coordinate space (N runs as 4).  Cell (row r, band index bi) sits on column lo + r + bi.  out7: score, q_start,
// q_end, t_start, t_end (assembly coordinates), matches, block_len -- zeros behind the score when it is below
// KP_MIN_DP_SCORE.  Returns the number of ops (written to `ops` while they fit), ops in the order of increasing target position.
int kpy_band(const uint8_t *gene, int qlen, const uint8_t *asm_codes, int lo, int width, int cstart, int cend, int32_t *out7,
             uint32_t *ops, int ops_cap) {
    const int W = width, OE = KP_GAP_OPEN + KP_GAP_EXT, EX = KP_GAP_EXT;
    std::vector<int> H((size_t)qlen * W, 0), E((size_t)qlen * W, NEG), F((size_t)qlen * W, NEG);
    std::vector<uint8_t> src((size_t)qlen * W, 3);  // 0 diagonal, 1 E, 2 F, 3 restart; bit 2: E extended, bit 3: F extended
    auto at = [&](int r, int bi) { return (size_t)r * W + bi; };
    auto inside = [&](int r, int bi) { const int t = lo + r + bi; return r >= 0 && r < qlen && bi >= 0 && bi < W && t >= cstart && t < cend; };
    int best = 0, best_r = -1, best_b = -1;
    for (int r = 0; r < qlen; ++r)
        for (int bi = 0; bi < W; ++bi) {  // (row, column) order: the column grows with bi
            if (!inside(r, bi)) continue;
            const int t = lo + r + bi;
            // neighbours outside the band or the contig read as H = 0, E = F = -inf
            const int h_left = inside(r, bi - 1) ? H[at(r, bi - 1)] : 0, e_left = inside(r, bi - 1) ? E[at(r, bi - 1)] : NEG;
            const int h_up = inside(r - 1, bi + 1) ? H[at(r - 1, bi + 1)] : 0, f_up = inside(r - 1, bi + 1) ? F[at(r - 1, bi + 1)] : NEG;
            const int h_diag = inside(r - 1, bi) ? H[at(r - 1, bi)] : 0;
            const int e_open = h_left - OE, e_ext = e_left - EX, f_open = h_up - OE, f_ext = f_up - EX;
            const int e = std::max(e_open, e_ext), f = std::max(f_open, f_ext);
            uint8_t flags = 0;
            if (e_ext > e_open) flags |= 4;  // opening wins ties against extending
            if (f_ext > f_open) flags |= 8;
            const int d = h_diag + sub_score(gene[r], asm_codes[t]);
            int h = d;
            uint8_t s = 0;  // the diagonal wins ties against E, E against F
            if (e > h) { h = e; s = 1; }
            if (f > h) { h = f; s = 2; }
            if (h <= 0) { h = 0; s = 3; }
            H[at(r, bi)] = h; E[at(r, bi)] = e; F[at(r, bi)] = f; src[at(r, bi)] = s | flags;
            if (h > best) { best = h; best_r = r; best_b = bi; }  // first maximum in (row, column) order
        }
    std::memset(out7, 0, 7 * sizeof(int32_t));
    out7[0] = best;
    if (best < KP_MIN_DP_SCORE) return 0;
    // traceback: the path starts where the diagonal predecessor's H is not positive
    std::vector<uint32_t> rev;  // ops in walking order (end to start)
    auto push = [&](uint32_t op) {
        if (!rev.empty() && (rev.back() & 15u) == op) rev.back() += 1u << KP_CIGAR_SHIFT;
        else rev.push_back((1u << KP_CIGAR_SHIFT) | op);
    };
    int r = best_r, bi = best_b, state = 0, matches = 0, cols = 0, gap = 0, credit = 0, sr = r, sb = bi;
    for (;;) {
        const uint8_t s = src[at(r, bi)];
        if (state == 0) {
            if ((s & 3) == 0) {
                ++cols; push(KP_CIGAR_M);
                const int t = lo + r + bi;
                if (gene[r] < 4 && gene[r] == asm_codes[t]) ++matches;
                sr = r; sb = bi;
                const int h_diag = inside(r - 1, bi) ? H[at(r - 1, bi)] : 0;
                if (h_diag <= 0) break;
                --r;
            } else if ((s & 3) == 3) {
                return -1;  // a path never reaches a restart cell
            } else state = s & 3;
        } else if (state == 1) {  // E: one column along the target
            ++cols; ++gap; push(KP_CIGAR_D);
            const bool opened = !(s & 4);
            --bi;
            if (opened) { state = 0; credit += std::max(gap - KP_GAP_LONG, 0); gap = 0; }
        } else {  // F: one column along the query
            ++cols; ++gap; push(KP_CIGAR_I);
            const bool opened = !(s & 8);
            --r; ++bi;
            if (opened) { state = 0; credit += std::max(gap - KP_GAP_LONG, 0); gap = 0; }
        }
    }
    out7[0] = best + credit;
    out7[1] = sr; out7[2] = best_r + 1;
    out7[3] = sr + lo + sb; out7[4] = best_r + lo + best_b + 1;
    out7[5] = matches; out7[6] = cols;
    const int n = (int)rev.size();
    for (int i = 0; i < n && i < ops_cap; ++i) ops[i] = rev[(size_t)n - 1 - i];
    return n;
}

// ---- buffer policy of the CIGAR ops (kp_caps.h) -----------------------------------------------------------------------------
void kpy_layout(int32_t *out3) {
    out3[0] = (int32_t)sizeof(KpCapOptions); out3[1] = (int32_t)sizeof(KpLearnt); out3[2] = (int32_t)KpCapOptions().cigar_ops_per_hit;
}
// state3: option cigar_ops_per_hit, learnt cigar_ops_per_hit, (unused)
uint64_t kpy_cigar_size(uint32_t *state3, uint64_t total_hits) {
    KpCapOptions o; KpLearnt L;
    o.cigar_ops_per_hit = state3[0]; L.cigar_ops_per_hit = state3[1];
    const uint64_t cap = kp_caps_cigar_size(o, L, total_hits);
    state3[1] = L.cigar_ops_per_hit;
    return cap;
}
// returns 1 when the ops fitted, 0 when *cap grew and the ops are to be written again
int kpy_cigar_after(uint32_t *state3, uint64_t *cap, uint64_t total_hits, uint64_t need) {
    KpLearnt L;
    L.cigar_ops_per_hit = state3[1];
    const bool ok = kp_caps_after_cigar(L, *cap, total_hits, need);
    state3[1] = L.cigar_ops_per_hit;
    return ok ? 1 : 0;
}
// kp_ctx_set_option of a buffer-size option: returns 1 when `name` is one; state3 as above, other_learnt: L.hit_cap before / after
int kpy_set_option(uint32_t *state3, uint32_t *other_learnt, const char *name, int64_t value) {
    KpCapOptions o; KpLearnt L;
    std::vector<KpRunCaps> runs;
    o.cigar_ops_per_hit = state3[0]; L.cigar_ops_per_hit = state3[1]; L.hit_cap = *other_learnt;
    const bool ok = kp_caps_set_option(o, L, runs, name, value);
    state3[0] = o.cigar_ops_per_hit; state3[1] = L.cigar_ops_per_hit; *other_learnt = L.hit_cap;
    return ok ? 1 : 0;
}

}  // extern "C"
