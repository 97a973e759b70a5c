// dist_harness.cpp -- test infrastructure for tests/test_distances_cpu.py (g++, no GPU): the functions of kaptive_amd/csrc/kp_dist.h --
// the ones the device kernels call -- on host arrays.
//   * kpy_dist_layout: the record's size and the constants the Python side mirrors.
//   * kpy_dist_pad_mask, kpy_dist_block_planes, kpy_dist_word_planes: padding and planes.
//   * kpy_dist_pair_counts: the three counts of a pair of rows, plane word by plane word, as a lane of the pair kernel adds them.
//   * kpy_dist_listed, kpy_dist_tile_of: the listing predicate and the tile a workgroup owns.
#include <cstddef>
#include <cstdint>

#include "../../kaptive_amd/csrc/kp_caps.h"
#include "../../kaptive_amd/csrc/kp_dist.h"

extern "C" {

void kpy_dist_layout(int32_t *out8) {
    out8[0] = (int32_t)sizeof(kp_dist_pair); out8[1] = KP_DIST_TILE; out8[2] = KP_DIST_CHUNK; out8[3] = KP_DIST_WORD_BLOCKS;
    out8[4] = KP_DIST_MAX_DIFF; out8[5] = KP_DIST_MIN_COMPARED; out8[6] = KP_DIST_MAX_ROWS; out8[7] = KP_DIST_REG;
}

uint64_t kpy_dist_pad_mask(int64_t Lq) { return kp_dist_pad_mask(Lq); }

void kpy_dist_block_planes(uint64_t v, uint32_t *out4) {
    const KpDistPlanes16 p = kp_dist_block_planes(v);
    out4[0] = p.lo; out4[1] = p.hi; out4[2] = p.valid; out4[3] = p.present;
}

// the four plane words of every word of a row: out[4 * w + (lo, hi, valid, present)]
void kpy_dist_word_planes(const uint64_t *row, int64_t nb, uint64_t *out) {
    for (int64_t w = 0; w < kp_dist_words(nb); ++w) {
        const KpDistWord q = kp_dist_word_planes(row, nb, w);
        out[4 * w] = q.lo; out[4 * w + 1] = q.hi; out[4 * w + 2] = q.valid; out[4 * w + 3] = q.present;
    }
}

void kpy_dist_pair_counts(const uint64_t *a, const uint64_t *b, int64_t nb, int32_t *out3) {
    const KpDistCounts n = kp_dist_row_counts(a, b, nb);
    out3[0] = n.compared; out3[1] = n.differences; out3[2] = n.unshared;
}

int kpy_dist_listed(int32_t compared, int32_t differences, int32_t max_diff, int32_t min_compared) {
    return kp_dist_listed(compared, differences, max_diff, min_compared) ? 1 : 0;
}

int64_t kpy_dist_tiles(int64_t nt) { return kp_dist_tiles(nt); }
void kpy_dist_tile_of(int64_t t, int64_t nt, int32_t *out2) { kp_dist_tile_of(t, nt, &out2[0], &out2[1]); }

}  // extern "C"
