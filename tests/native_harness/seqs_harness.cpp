// seqs_harness.cpp -- test infrastructure for tests/test_seqs_cpu.py (g++, no GPU): the N-run and base-code look-ups of
// kaptive_amd/csrc/kp_seqs.h, the one statement every fill and walk of the device reads its sequences through.
#include "../../kaptive_amd/csrc/kp_seqs.h"

extern "C" {

int kps_first_run_after(const int32_t *runs, int n_runs, int32_t t) { return kp_first_run_after(runs, n_runs, t); }
int kps_in_n_run(const int32_t *runs, int n_runs, int32_t t) { return kp_in_n_run(runs, n_runs, t) ? 1 : 0; }
int kps_code_at(const uint32_t *words, const int32_t *runs, int n_runs, int32_t t) { return kp_code_at(words, runs, n_runs, t); }
uint32_t kps_n_mask(const int32_t *runs, int n_runs, int32_t t0, int width) { return kp_n_mask(runs, n_runs, t0, width); }
int kps_sub_score(int qc, int tc) { return kp_sub_score(qc, tc); }
// the views: a contig [cstart, cend) of the assembly, a gene of qlen rows
int kps_target_code(const uint32_t *words, int n_words, const int32_t *runs, int n_runs, int cstart, int cend, int t) {
    const KpTargetSeq s{words, runs, n_words, n_runs, cstart, cend};
    return s.code(t);
}
int kps_query_code(const uint32_t *nib, int qlen, int r) {
    const KpQuerySeq q{nib, qlen};
    return q.code(r);
}

}  // extern "C"
