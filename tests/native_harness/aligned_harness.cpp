// aligned_harness.cpp -- test infrastructure for tests/test_aligned_cpu.py (g++, no GPU): kaptive_amd/csrc/kp_aligned.h on host
// arrays.
//   * kpy_aligned_row: kp_aligned_row_blocks -- the row of one kept record made one op after the other.  rec4: gene_len, covered,
//     inserted, n_ins.  Returns 1 for a valid walk.
//   * kpy_aln_layout: sizeof(kp_aligned_row), the columns of a block, the bit of the gap mask.
#include <cstddef>
#include <cstdint>

#include "../../kaptive_amd/csrc/kp_aligned.h"

extern "C" {

int kpy_aligned_row(const uint32_t *ops, int64_t n_ops, int found, const uint32_t *words, int n_words, const int32_t *runs, int n_runs, int cstart,
                    int clen, int Lq, int q_start, int q_end, int t_start, int strand, uint64_t *blocks, int32_t *rec4) {
    KpTargetSeq t;
    t.words = words; t.n_words = n_words; t.runs = runs; t.n_runs = n_runs; t.cstart = cstart; t.cend = cstart + clen;
    kp_aligned_row row;
    row.off = 0;
    const bool ok = kp_aligned_row_blocks(ops, n_ops, found != 0, t, Lq, q_start, q_end, t_start, strand, blocks, &row);
    rec4[0] = row.gene_len; rec4[1] = row.covered; rec4[2] = row.inserted; rec4[3] = row.n_ins;
    return ok ? 1 : 0;
}

void kpy_aln_layout(int32_t *out3) { out3[0] = (int32_t)sizeof(kp_aligned_row); out3[1] = KP_ALN_COLS; out3[2] = KP_ALN_GAP_SHIFT; }

}  // extern "C"
