// breakpoints_harness.cpp -- test infrastructure for tests/test_breakpoints_cpu.py (g++, no GPU):
//   * kpy_breakpoints: the records of one kept list from the functions of kaptive_amd/csrc/kp_breakpoints.h -- the ones the device
//     kernel gives a lane per b -- on host arrays: every b in ascending order, its candidates offered in tiles of `tile` records as
//     the kernel offers them from LDS, the records stored with kp_breakpoint_store one behind the other.
//   * kpy_bp_layout: sizes and constants the Python side restates.
#include <cstdint>
#include <vector>

#include "../../kaptive_amd/csrc/kp_breakpoints.h"

extern "C" {

// returns the number of records (out holds n_kept of them at the most); words / runs: the assembly's packed bases and N runs
int64_t kpy_breakpoints(const kp_kept *kept, int n_kept, int n_ctg, const int32_t *ctg_start, const int32_t *ctg_len, const uint32_t *words, int n_words,
                        const int32_t *runs, int n_runs, int tile, kp_breakpoint *out) {
    std::vector<KpBpFrag> frags((size_t)n_kept);
    for (int i = 0; i < n_kept; ++i) frags[(size_t)i] = kp_bp_frag(kept[i], n_ctg, ctg_len);
    const auto frag = [&](int i) { return frags[(size_t)i]; };
    if (tile < 1) tile = 1;
    int64_t n_out = 0;
    for (int ib = 0; ib < n_kept; ++ib) {
        KpBpBest best;
        for (int t0 = 0; t0 < n_kept; t0 += tile) kp_bp_select(frag, t0, t0 + tile < n_kept ? t0 + tile : n_kept, frags[(size_t)ib], ib, best);
        if (best.a < 0) continue;
        KpTargetSeq t;
        t.words = words; t.n_words = n_words; t.runs = runs; t.n_runs = n_runs;
        t.cstart = ctg_start[frags[(size_t)ib].contig];
        t.cend = t.cstart + frags[(size_t)ib].ctg_len;
        kp_breakpoint_store(out + n_out++, kp_bp_record(best, ib, t));
    }
    return n_out;
}

void kpy_bp_layout(int32_t *out4) {
    out4[0] = (int32_t)sizeof(kp_breakpoint); out4[1] = KP_BP_MAX_OVERLAP; out4[2] = KP_BP_IR_COLS; out4[3] = (int32_t)sizeof(KpBpFrag) / 4;
}

}  // extern "C"
