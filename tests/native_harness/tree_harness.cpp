// tree_harness.cpp -- test infrastructure for tests/test_tree_cpu.py (g++, no GPU): the functions of kaptive_amd/csrc/kp_tree.h -- the
// ones the tree kernels call, in their host bodies -- on host arrays.
//   * kpy_tree_layout: the constants the Python side mirrors.
//   * kpy_tree_key, kpy_tree_key_none, kpy_tree_unpack: the packed edge key.
//   * kpy_tree_fits, kpy_tree_max_rounds: the matrix that fits the key, the bound on the rounds.
//   * kpy_tree_unite: an edge list united in the order given by the union that names the root it moved.
//   * kpy_tree_host: the forest of a matrix of blocks by the serial Boruvka of the header.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../kaptive_amd/csrc/kp_tree.h"

extern "C" {

void kpy_tree_layout(int64_t *out4) {
    out4[0] = KP_TREE_ROW_BITS; out4[1] = KP_TREE_DIFF_BITS; out4[2] = KP_TREE_MAX_COLUMNS; out4[3] = KP_DIST_MAX_ROWS;
}

uint64_t kpy_tree_key(int32_t differences, int32_t a, int32_t b) { return kp_tree_key(differences, a, b); }
uint64_t kpy_tree_key_none(void) { return KP_TREE_KEY_NONE; }
void kpy_tree_unpack(uint64_t key, int32_t *out3) { out3[0] = kp_tree_key_differences(key); out3[1] = kp_tree_key_a(key); out3[2] = kp_tree_key_b(key); }
int kpy_tree_fits(int64_t n_blocks) { return kp_tree_fits(n_blocks) ? 1 : 0; }
int32_t kpy_tree_max_rounds(int64_t n_rows) { return kp_tree_max_rounds(n_rows); }

// edges [n][2]; moved [n]: the root every union moved, -1 for none.  label [R]: every row's root afterwards.
void kpy_tree_unite(int32_t R, const int32_t *edges, int64_t n, int32_t *moved, int32_t *label) {
    std::vector<int32_t> parent((size_t)R);
    for (int32_t r = 0; r < R; ++r) parent[(size_t)r] = r;
    for (int64_t i = 0; i < n; ++i) moved[i] = kp_clust_unite_root(parent.data(), edges[2 * i], edges[2 * i + 1]);
    for (int32_t r = 0; r < R; ++r) label[r] = kp_clust_find(parent.data(), r);
}

int64_t kpy_tree_host(const uint64_t *blocks, int32_t R, int64_t nb, int32_t min_compared, kp_dist_pair *edges, int32_t *component, int32_t *rounds) {
    return kp_tree_host(blocks, R, nb, min_compared, edges, component, rounds);
}

}  // extern "C"
