// variants_harness.cpp -- test infrastructure for tests/test_variants_cpu.py (g++, no GPU):
//   * kpy_variants: kp_variants_hit of kaptive_amd/csrc/kp_variants.h -- the function the device kernels give a lane per kept
//     record -- on host arrays, with the counting sink (buf == null) or the storing sink on a buffer of `cap` records.
//   * kpy_codon_table: the 125-entry table the header is given on the device (kp_fill_codon_table).
//   * kpy_var_*: the variants part of the buffer-size policy (kaptive_amd/csrc/kp_caps.h).
#include <cstdint>
#include <string>
#include <vector>

#include "../../kaptive_amd/csrc/kp_caps.h"
#include "../../kaptive_amd/csrc/kp_reduce_core.h"
#include "../../kaptive_amd/csrc/kp_variants.h"

extern "C" {

// returns the records of the hit (the storing sink's count: it keeps counting whatever it could store).  nib: the gene as
// aligned, fwd_nib: its forward strand; base, n: the hit's range of the buffer (its offset and its count)
int64_t kpy_variants(const uint32_t *ops, int64_t n_ops, const uint32_t *nib, const uint32_t *fwd_nib, int qlen, const uint32_t *words, int n_words,
                     const int32_t *runs, int n_runs, int cstart, int cend, int q0, int t0, int rev, int32_t kept, kp_variant *buf, int64_t base,
                     int64_t n, int64_t cap) {
    KpTaskSeqs s;
    s.q.nib = nib; s.q.len = qlen;
    s.t.words = words; s.t.n_words = n_words; s.t.runs = runs; s.t.n_runs = n_runs; s.t.cstart = cstart; s.t.cend = cend;
    const KpQuerySeq fwd{fwd_nib, qlen};
    uint8_t codon[125];
    kp_fill_codon_table(codon);
    if (!buf) {
        KpVarCount out;
        kp_variants_hit(ops, n_ops, s, fwd, q0, t0, rev != 0, kept, codon, out);
        return out.n;
    }
    KpVarStore out{buf, base, n, cap, rev != 0};
    kp_variants_hit(ops, n_ops, s, fwd, q0, t0, rev != 0, kept, codon, out);
    return out.k;
}

void kpy_codon_table(uint8_t *out125) { kp_fill_codon_table(out125); }

void kpy_var_layout(int32_t *out2) { out2[0] = (int32_t)KpVarCaps().per_kept; out2[1] = (int32_t)sizeof(kp_variant); }
// state2: option variants_per_kept, learnt records per kept record
uint64_t kpy_var_size(uint32_t *state2, uint64_t total_kept) {
    KpVarCaps c{state2[0], state2[1]};
    const uint64_t cap = kp_caps_variants_size(c, total_kept);
    state2[0] = c.per_kept; state2[1] = c.learnt;
    return cap;
}
// returns 1 when the records fitted, 0 when *cap grew and the records are to be stored again
int kpy_var_after(uint32_t *state2, uint64_t *cap, uint64_t total_kept, uint64_t need) {
    KpVarCaps c{state2[0], state2[1]};
    const bool ok = kp_caps_after_variants(c, *cap, total_kept, need);
    state2[0] = c.per_kept; state2[1] = c.learnt;
    return ok ? 1 : 0;
}
// kp_ctx_set_option as kp_ctx.hip dispatches it: the buffer-size options of kp_caps_set_option first, then the cs option, then the
// variants option; returns 1 when `name` is any of them.  others2: KpLearnt::cigar_ops_per_hit and KpCsCaps::learnt before / after
int kpy_var_set_option(uint32_t *state2, uint32_t *others2, const char *name, int64_t value) {
    KpCapOptions o; KpLearnt L;
    std::vector<KpRunCaps> runs;
    KpCsCaps cs; KpVarCaps c{state2[0], state2[1]};
    L.cigar_ops_per_hit = others2[0]; cs.learnt = others2[1];
    const bool ok = kp_caps_set_option(o, L, runs, name, value) || kp_caps_set_cs_option(cs, name, value) || kp_caps_set_variants_option(c, name, value);
    state2[0] = c.per_kept; state2[1] = c.learnt; others2[0] = L.cigar_ops_per_hit; others2[1] = cs.learnt;
    return ok ? 1 : 0;
}

}  // extern "C"
