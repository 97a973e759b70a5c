// transfer_harness.cpp -- test infrastructure for tests/test_nj_transfer_cpu.py (g++, no GPU): the functions of
// kaptive_amd/csrc/kp_transfer.h -- the ones the transfer kernels and the formatter call, in their host bodies -- on host arrays.
//   * kpy_transfer_depth, kpy_transfer_delta: the depth of a split; the distance of two splits from their sizes and their overlap.
//   * kpy_transfer_label: the thousandths of a label.
//   * kpy_transfer_sizes: the taxa below the node of every record with an inner edge.
//   * kpy_transfer_phi: the transfer distances of one replicate's tree (kp_transfer_host).
#include <stdint.h>

#include "../../kaptive_amd/csrc/kp_transfer.h"

extern "C" {

int32_t kpy_transfer_depth(int32_t s, int32_t n) { return kp_transfer_depth(s, n); }
int32_t kpy_transfer_delta(int32_t s, int32_t z, int32_t c, int32_t n) { return kp_transfer_delta(s, z, c, n); }
int64_t kpy_transfer_label(int64_t transfer, int64_t replicates, int64_t depth) { return kp_transfer_label(transfer, replicates, depth); }
void kpy_transfer_sizes(const kp_nj_node *rec, int32_t n, int32_t *out) { kp_transfer_sizes(rec, n, out); }
void kpy_transfer_phi(const kp_nj_node *ref, const kp_nj_node *replicate, int32_t n, int32_t *phi) { kp_transfer_host(ref, replicate, n, phi); }

}  // extern "C"
