// boot_harness.cpp -- test infrastructure for tests/test_nj_boot_cpu.py (g++, no GPU): the functions of kaptive_amd/csrc/kp_boot.h -- the
// ones the bootstrap kernels call, in their host bodies -- on host arrays.
//   * kpy_boot_caps: the constants the Python side mirrors.
//   * kpy_boot_mix, kpy_boot_draws, kpy_boot_weights: the mixer, the draws of a replicate and its weights.
//   * kpy_boot_clamp: the clamp of a table of counts.
//   * kpy_boot_row_counts: the weighted counts of two rows of blocks; kpy_boot_word_planes: the weight planes of a plane word.
//   * kpy_boot_key, kpy_boot_total: the key of a set of taxa and of all of them.
//   * kpy_boot_walk: the splits of a record list; kpy_boot_batch: the batch rule.
#include <stdint.h>

#include "../../kaptive_amd/csrc/kp_boot.h"

extern "C" {

void kpy_boot_caps(int64_t *out4) {
    out4[0] = KP_BOOT_MAX_REPLICATES; out4[1] = KP_BOOT_MATRIX_BYTES; out4[2] = KP_BOOT_MAX_BATCH; out4[3] = KP_BOOT_PLANES;
}
uint64_t kpy_boot_mix(uint64_t x) { return kp_boot_mix(x); }
void kpy_boot_draws(uint64_t seed, int64_t r, int64_t W, int64_t *out) {
    const uint64_t stream = kp_boot_stream(seed, (uint64_t)r);
    for (int64_t t = 0; t < W; ++t) out[t] = kp_boot_draw(stream, (uint64_t)t, W);
}
void kpy_boot_weights(uint64_t seed, int64_t r, int64_t W, uint8_t *out) { kp_boot_weights_host(seed, r, W, out); }
void kpy_boot_clamp(const uint32_t *count, int64_t n, uint32_t *out) {
    for (int64_t i = 0; i < n; ++i) out[i] = kp_boot_weight(count[i]);
}
void kpy_boot_row_counts(const uint64_t *a, const uint64_t *b, int64_t nb, const uint8_t *weight, int32_t *out2) {
    const KpDistCounts c = kp_boot_row_counts(a, b, nb, weight);
    out2[0] = c.compared; out2[1] = c.differences;
}
int kpy_boot_word_planes(const uint8_t *weight, int64_t W, int64_t w, uint64_t *out8) {
    uint64_t M[KP_BOOT_PLANES];
    const int top = kp_boot_word_planes(weight, W, w, M);
    for (int k = 0; k < KP_BOOT_PLANES; ++k) out8[k] = M[k];
    return top;
}
uint64_t kpy_boot_key(const int32_t *taxa, int64_t n) {
    uint64_t s = 0;
    for (int64_t i = 0; i < n; ++i) s += kp_boot_taxon_key(taxa[i]);
    return s;
}
uint64_t kpy_boot_total(int32_t n) { return kp_boot_total_key(n); }
// out: n - 3 triples (key, size, has0) as uint64
void kpy_boot_walk(const kp_nj_node *rec, int32_t n, uint64_t *out) {
    std::vector<KpBootSplit> s((size_t)kp_boot_splits(n));
    kp_boot_walk(rec, n, kp_boot_total_key(n), s.data());
    for (size_t t = 0; t < s.size(); ++t) { out[3 * t] = s[t].key; out[3 * t + 1] = (uint64_t)s[t].size; out[3 * t + 2] = (uint64_t)s[t].has0; }
}
int32_t kpy_boot_batch(int64_t n, int64_t replicates, int64_t max_batch) { return kp_boot_batch(n, replicates, max_batch); }

}  // extern "C"
