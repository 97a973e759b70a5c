// kp_rescue.h -- geometry of the translated search of the missing genes (kp_spec.h, RESCUE), written once as plain functions: the window
// of a piece, the length of a frame text, residue a of a frame text read from the packed words and the N runs, the mapping of an
// aligned stretch back to the contig, the task index and the edge bits.  The device kernels (kp_rescue.hip) and the tests' harness
// call the same functions.  Base codes are read through kp_seqs.h only: a residue touches the words of its three bases and nothing
// else -- never a word beyond the assembly's last.  No HIP header: tests/native_harness compiles it with g++.
#pragma once

#include "kp_seqs.h"

#define KP_RS_FRAMES 6 /* tasks per (subject, piece): two strands x three frames */

// window of the piece [start, end) on a contig of ctg_len bases, contig coordinates; false (and an empty window) for a piece that does
// not lie inside its contig
KP_HD bool kp_rs_window(int32_t start, int32_t end, int32_t ctg_len, int32_t flank, int32_t *ws, int32_t *we) {
    *ws = 0; *we = 0;
    if (start < 0 || end < start || end > ctg_len || flank < 0) return false;
    *ws = start > flank ? start - flank : 0;
    *we = (int64_t)end + flank < ctg_len ? end + flank : ctg_len;
    return true;
}

// A: residues of the frame text of window [ws, we) in frame f
KP_HD int32_t kp_rs_frame_len(int32_t ws, int32_t we, int f) { return we - ws - f >= 3 ? (we - ws - f) / 3 : 0; }

// task index of (piece, strand, frame) within a subject, and its two halves
KP_HD int32_t kp_rs_task(int32_t piece, int strand, int f) { return (piece * 2 + (strand < 0 ? 1 : 0)) * 3 + f; }
KP_HD int kp_rs_task_strand(int32_t sf) { return sf >= 3 ? -1 : 1; }  // sf = task index % KP_RS_FRAMES
KP_HD int kp_rs_task_frame(int32_t sf) { return sf % 3; }

// contig position of the first base (in reading order) of residue a, and the step to the next base
KP_HD int32_t kp_rs_codon_pos(int32_t ws, int32_t we, int strand, int f, int32_t a) { return strand >= 0 ? ws + f + 3 * a : we - 1 - f - 3 * a; }

// Residue a < A of the frame text: the amino acid of its codon by the 125-entry table of kp_fill_codon_table.  t: the assembly's words
// and runs and the contig's bounds; the window lies inside the contig, so every base read lies inside the assembly's words.
// clear_of_runs: no N run touches the window (kp_rs_clear_of_runs): the run list is not searched.
KP_HD uint8_t kp_rs_residue(const KpTargetSeq &t, const uint8_t *codon, int32_t ws, int32_t we, int strand, int f, int32_t a, bool clear_of_runs) {
    const int32_t p0 = t.cstart + kp_rs_codon_pos(ws, we, strand, f, a), step = strand >= 0 ? 1 : -1;
    int code[3];
    for (int x = 0; x < 3; ++x) {
        const int32_t p = p0 + step * x;
        const int v = clear_of_runs ? (int)((t.words[p >> 4] >> (2 * (p & 15))) & 3u) : t.at(p);
        code[x] = strand >= 0 ? v : (v > 3 ? 4 : 3 - v);
    }
    return codon[code[0] * 25 + code[1] * 5 + code[2]];
}

// no N run touches the window [ws, we) of the contig
KP_HD bool kp_rs_clear_of_runs(const KpTargetSeq &t, int32_t ws, int32_t we) {
    const int a = kp_first_run_after(t.runs, t.n_runs, t.cstart + ws);
    return a >= t.n_runs || t.runs[2 * a] >= t.cstart + we;
}

// the residues [a0, a1) of a frame text on the contig's forward strand, half-open
KP_HD void kp_rs_coords(int32_t ws, int32_t we, int strand, int f, int32_t a0, int32_t a1, int32_t *t_start, int32_t *t_end) {
    if (strand >= 0) { *t_start = ws + f + 3 * a0; *t_end = ws + f + 3 * a1; }
    else { *t_start = we - f - 3 * a1; *t_end = we - f - 3 * a0; }
}

KP_HD uint8_t kp_rs_edge(int32_t t_start, int32_t t_end, int32_t ctg_len, int32_t tol) {
    return (uint8_t)((t_start <= tol ? 1 : 0) | (t_end >= ctg_len - tol ? 2 : 0));
}

// ---- the strips of the fill (kp_rescue.hip) ----------------------------------------------------------------------------------------
// A wave holds KP_RS_LANES x NC columns of the protein, NC one of the three below: the smallest that holds the protein, or strips of
// the widest.  (tests/rescue_util.py restates the limits as STRIP_LIMITS: change them together.)
#define KP_RS_LANES 64
#define KP_RS_NC_SMALL 2
#define KP_RS_NC_MID 4
#define KP_RS_NC_WIDE 6
KP_HD int kp_rs_cols_per_lane(int32_t prot_len) {
    return prot_len <= KP_RS_LANES * KP_RS_NC_SMALL ? KP_RS_NC_SMALL : (prot_len <= KP_RS_LANES * KP_RS_NC_MID ? KP_RS_NC_MID : KP_RS_NC_WIDE);
}
KP_HD bool kp_rs_needs_strips(int32_t prot_len) { return prot_len > KP_RS_LANES * KP_RS_NC_WIDE; }
