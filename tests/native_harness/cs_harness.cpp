// cs_harness.cpp -- test infrastructure for tests/test_cs_cpu.py (g++, no GPU):
//   * kpy_cs: kp_cs_hit of kaptive_amd/csrc/kp_cs.h -- the function the device kernels give a lane per hit -- on host arrays,
//     with the counting sink (buf == null) or the writing sink on a buffer of `cap` bytes.
//   * kpy_cs_*: the cs part of the buffer-size policy (kaptive_amd/csrc/kp_caps.h).
#include <cstdint>
#include <string>
#include <vector>

#include "../../kaptive_amd/csrc/kp_caps.h"
#include "../../kaptive_amd/csrc/kp_cs.h"

extern "C" {

// returns the bytes of the string (the writing sink's final position: it keeps counting past cap)
int64_t kpy_cs(const uint32_t *ops, int64_t n_ops, const uint32_t *nib, int qlen, const uint32_t *words, int n_words, const int32_t *runs, int n_runs,
               int cstart, int cend, int q0, int t0, char *buf, int64_t cap) {
    KpTaskSeqs s;
    s.q.nib = nib; s.q.len = qlen;
    s.t.words = words; s.t.n_words = n_words; s.t.runs = runs; s.t.n_runs = n_runs; s.t.cstart = cstart; s.t.cend = cend;
    if (!buf) {
        KpCsCount out;
        kp_cs_hit(ops, n_ops, s, q0, t0, out);
        return out.n;
    }
    KpCsWrite out{buf, 0, cap};
    kp_cs_hit(ops, n_ops, s, q0, t0, out);
    return out.pos;
}

void kpy_cs_layout(int32_t *out1) { out1[0] = (int32_t)KpCsCaps().bytes_per_hit; }
// state2: option cs_bytes_per_hit, learnt bytes per hit
uint64_t kpy_cs_size(uint32_t *state2, uint64_t total_hits) {
    KpCsCaps c{state2[0], state2[1]};
    const uint64_t cap = kp_caps_cs_size(c, total_hits);
    state2[0] = c.bytes_per_hit; state2[1] = c.learnt;
    return cap;
}
// returns 1 when the bytes fitted, 0 when *cap grew and the bytes are to be written again
int kpy_cs_after(uint32_t *state2, uint64_t *cap, uint64_t total_hits, uint64_t need) {
    KpCsCaps c{state2[0], state2[1]};
    const bool ok = kp_caps_after_cs(c, *cap, total_hits, need);
    state2[0] = c.bytes_per_hit; state2[1] = c.learnt;
    return ok ? 1 : 0;
}
// kp_ctx_set_option as kp_ctx.hip dispatches it: the buffer-size options of kp_caps_set_option first, then the cs option; returns 1
// when `name` is either.  other_learnt: KpLearnt::cigar_ops_per_hit before / after
int kpy_cs_set_option(uint32_t *state2, uint32_t *other_learnt, const char *name, int64_t value) {
    KpCapOptions o; KpLearnt L;
    std::vector<KpRunCaps> runs;
    KpCsCaps c{state2[0], state2[1]};
    L.cigar_ops_per_hit = *other_learnt;
    const bool ok = kp_caps_set_option(o, L, runs, name, value) || kp_caps_set_cs_option(c, name, value);
    state2[0] = c.bytes_per_hit; state2[1] = c.learnt; *other_learnt = L.cigar_ops_per_hit;
    return ok ? 1 : 0;
}

}  // extern "C"
