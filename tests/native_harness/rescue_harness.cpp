// rescue_harness.cpp -- test infrastructure for tests/test_rescue_cpu.py (g++, no GPU): the functions of kaptive_amd/csrc/kp_rescue.h --
// the ones the device kernels call -- on host arrays.
//   * kpy_rs_window: the window of a piece and the lengths of its three frame texts.
//   * kpy_rs_text: a whole frame text, residue by residue, as the fill kernel's lanes translate it (with and without the shortcut for
//     windows that no N run touches: both must agree where the shortcut applies).
//   * kpy_rs_coords: an aligned stretch back on the contig, and its edge bits.
//   * kpy_rs_layout: the record's size, the frames per unit and the strip limits.
//   * kpy_rs_lanes: KP_RS_LANES -- the rows a wave takes per turn (tests/rescue_paths_util.py restates it as ROW_CHUNK).
#include <cstddef>
#include <cstdint>

#include "../../kaptive_amd/csrc/kp_reduce_core.h"
#include "../../kaptive_amd/csrc/kp_rescue.h"

extern "C" {

int kpy_rs_window(int start, int end, int ctg_len, int flank, int32_t *out5) {
    int32_t ws, we;
    const bool ok = kp_rs_window(start, end, ctg_len, flank, &ws, &we);
    out5[0] = ws; out5[1] = we;
    for (int f = 0; f < 3; ++f) out5[2 + f] = kp_rs_frame_len(ws, we, f);
    return ok ? 1 : 0;
}

// returns A and writes the A residues; -1 when the shortcut for clear windows disagrees with the searched run list
int kpy_rs_text(const uint32_t *words, int n_words, const int32_t *runs, int n_runs, int cstart, int clen, int ws, int we, int sf, uint8_t *out) {
    KpTargetSeq t;
    t.words = words; t.n_words = n_words; t.runs = runs; t.n_runs = n_runs; t.cstart = cstart; t.cend = cstart + clen;
    uint8_t codon[125];
    kp_fill_codon_table(codon);
    const int strand = kp_rs_task_strand(sf), f = kp_rs_task_frame(sf);
    const int32_t A = kp_rs_frame_len(ws, we, f);
    const bool clear = kp_rs_clear_of_runs(t, ws, we);
    for (int32_t a = 0; a < A; ++a) {
        out[a] = kp_rs_residue(t, codon, ws, we, strand, f, a, false);
        if (clear && kp_rs_residue(t, codon, ws, we, strand, f, a, true) != out[a]) return -1;
    }
    return A;
}

void kpy_rs_coords(int ws, int we, int sf, int a0, int a1, int ctg_len, int tol, int32_t *out3) {
    kp_rs_coords(ws, we, kp_rs_task_strand(sf), kp_rs_task_frame(sf), a0, a1, &out3[0], &out3[1]);
    out3[2] = kp_rs_edge(out3[0], out3[1], ctg_len, tol);
}

int kpy_rs_task(int piece, int strand, int f) { return kp_rs_task(piece, strand, f); }

void kpy_rs_layout(int32_t *out8) {
    out8[0] = (int32_t)sizeof(kp_rescue); out8[1] = KP_RS_FRAMES; out8[2] = KP_RS_LANES * KP_RS_NC_SMALL; out8[3] = KP_RS_LANES * KP_RS_NC_MID;
    out8[4] = KP_RS_LANES * KP_RS_NC_WIDE; out8[5] = KP_RESCUE_FLANK; out8[6] = KP_RESCUE_MIN_SCORE; out8[7] = KP_RESCUE_FLANK_MAX;
}

int kpy_rs_lanes() { return KP_RS_LANES; }

}  // extern "C"
