// pars_harness.cpp -- test infrastructure for tests/test_parsimony_cpu.py (g++, no GPU): the functions of kaptive_amd/csrc/kp_pars.h --
// the ones the parsimony kernels and the formatters call, in their host bodies -- on host arrays.
//   * kpy_pars_host: the whole pass over a matrix of blocks (kp_pars_host); with null tables it only counts.
//   * kpy_pars_tree_ok: the check of a record list.
//   * kpy_pars_join2 / kpy_pars_join3 / kpy_pars_pick / kpy_pars_child: the set rule, the smallest code and a child's state, on the
//     four words of every set: out gets the node's four words and then the step masks, or the state's two and the change mask.
//   * kpy_pars_step_planes, kpy_pars_node_planes: the counter's planes, the place of a node in the node table.
#include <stdint.h>
#include <string.h>

#include "../../kaptive_amd/csrc/kp_pars.h"

extern "C" {

int64_t kpy_pars_host(const uint64_t *blocks, int64_t nb, const int32_t *taxa, int32_t n, const kp_nj_node *rec, int64_t n_ref, kp_pars_site *sites, int64_t cap_sites,
                      kp_pars_change *changes, int64_t cap_changes, int64_t *n_sites, int64_t *n_changes) {
    std::vector<kp_pars_site> s;
    std::vector<kp_pars_change> c;
    kp_pars_host(blocks, nb, taxa, n, rec, n_ref, &s, &c);
    *n_sites = (int64_t)s.size();
    *n_changes = (int64_t)c.size();
    if (sites && cap_sites >= *n_sites && !s.empty()) memcpy(sites, s.data(), s.size() * sizeof(kp_pars_site));
    if (changes && cap_changes >= *n_changes && !c.empty()) memcpy(changes, c.data(), c.size() * sizeof(kp_pars_change));
    return 0;
}
int32_t kpy_pars_tree_ok(const kp_nj_node *rec, int64_t n_ref, int32_t n) { return kp_pars_tree_ok(rec, n_ref, n, nullptr) ? 1 : 0; }
void kpy_pars_join2(const uint64_t *x, const uint64_t *y, uint64_t *out) {
    const KpParsSet q = kp_pars_join2(KpParsSet{{x[0], x[1], x[2], x[3]}}, KpParsSet{{y[0], y[1], y[2], y[3]}}, out + 4);
    for (int k = 0; k < 4; ++k) out[k] = q.s[k];
}
void kpy_pars_join3(const uint64_t *x, const uint64_t *y, const uint64_t *z, uint64_t *out) {
    const KpParsSet q = kp_pars_join3(KpParsSet{{x[0], x[1], x[2], x[3]}}, KpParsSet{{y[0], y[1], y[2], y[3]}}, KpParsSet{{z[0], z[1], z[2], z[3]}}, out + 4, out + 5);
    for (int k = 0; k < 4; ++k) out[k] = q.s[k];
}
void kpy_pars_pick(const uint64_t *x, uint64_t *out) {
    const KpParsState t = kp_pars_pick(KpParsSet{{x[0], x[1], x[2], x[3]}});
    out[0] = t.lo; out[1] = t.hi;
}
void kpy_pars_child(const uint64_t *x, uint64_t lo, uint64_t hi, uint64_t *out) {
    const KpParsState t = kp_pars_child(KpParsSet{{x[0], x[1], x[2], x[3]}}, KpParsState{lo, hi}, out + 2);
    out[0] = t.lo; out[1] = t.hi;
}
int32_t kpy_pars_step_planes(void) { return KP_PARS_STEP_PLANES; }
int64_t kpy_pars_node_planes(int64_t v, int64_t n) { return kp_pars_node_planes(v, n); }

}  // extern "C"
