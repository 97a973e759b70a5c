// nj_harness.cpp -- test infrastructure for tests/test_nj_cpu.py (g++, no GPU): the functions of kaptive_amd/csrc/kp_nj.h -- the ones
// the NJ kernels call, in their host bodies -- on host arrays.
//   * kpy_nj_max_taxa, kpy_nj_node_size: the constants the Python side mirrors.
//   * kpy_nj_taxon, kpy_nj_row_bases: the taxon predicate and a row's bases.
//   * kpy_nj_sum64: SUM64.
//   * kpy_nj_q, kpy_nj_lengths, kpy_nj_update: the Q, length and update expressions.
//   * kpy_nj_host: the tree of a dense matrix by the serial loop of the header.
//   * kpy_nj_matrix_host: the taxa and the dense matrix of a matrix of blocks.
#include <cstddef>
#include <cstdint>

#include "../../kaptive_amd/csrc/kp_nj.h"

extern "C" {

int32_t kpy_nj_max_taxa(void) { return KP_NJ_MAX_TAXA; }
int32_t kpy_nj_node_size(void) { return (int32_t)sizeof(kp_nj_node); }
int kpy_nj_taxon(int64_t bases, int64_t W, int32_t min_compared) { return kp_nj_taxon(bases, W, min_compared) ? 1 : 0; }
int64_t kpy_nj_row_bases(const uint64_t *row, int64_t nb) { return kp_nj_row_bases(row, nb); }
double kpy_nj_sum64(const double *v, int64_t m) { return kp_nj_sum64(v, m); }
double kpy_nj_q(double f, double d, double ra, double rb) { return kp_nj_q(f, d, ra, rb); }
void kpy_nj_lengths(double dij, double ri, double rj, double f, double *out2) { kp_nj_lengths(dij, ri, rj, f, out2, out2 + 1); }
// out2: u_k, then the new R_k
void kpy_nj_update(double rk, double dik, double djk, double dij, double *out2) {
    out2[0] = kp_nj_u(dik, djk, dij);
    out2[1] = kp_nj_r(rk, dik, djk, out2[0]);
}
int64_t kpy_nj_host(const double *D, int32_t n, kp_nj_node *out) { return kp_nj_host(D, n, out); }
int32_t kpy_nj_matrix_host(const uint64_t *blocks, int32_t R, int64_t nb, int32_t min_compared, int32_t *taxa, double *D) {
    return kp_nj_matrix_host(blocks, R, nb, min_compared, taxa, D);
}

}  // extern "C"
