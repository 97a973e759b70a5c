// kp_seqs.h -- what an alignment reads of its two sequences, stated once: the base code at a position of a packed assembly
// with its list of N runs, the code of a gene's row, and the substitution score of the two (kp_spec.h).  The fills (kp_sw.hip,
// kp_join.hip), the walks (kp_walk.h), the extraction (kp_reduce_core.h) and the sketches' run cursors (kp_chain.hip,
// kp_scan.hip) all ask here, so they cannot disagree.  No HIP header: tests/native_harness compiles it with g++.
#pragma once

#include <stdint.h>

#include "../../include/kp_spec.h"

#if defined(__HIPCC__)
#define KP_HD __host__ __device__ __forceinline__
#else
#define KP_HD inline
#endif

// ---- N runs: `runs` holds n_runs pairs (start, end), ascending and disjoint, in the assembly's padded space ------------------
// index of the first run whose end is > t (n_runs: none)
KP_HD int kp_first_run_after(const int32_t *runs, int n_runs, int32_t t) {
    int a = 0, z = n_runs;
    while (a < z) {
        const int mid = (a + z) >> 1;
        if (runs[2 * mid + 1] <= t) a = mid + 1; else z = mid;
    }
    return a;
}

KP_HD bool kp_in_n_run(const int32_t *runs, int n_runs, int32_t t) {
    const int a = kp_first_run_after(runs, n_runs, t);
    return a < n_runs && runs[2 * a] <= t;
}

// base code at assembly position t: 0..3, or 4 inside an N run
KP_HD int kp_code_at(const uint32_t *words, const int32_t *runs, int n_runs, int32_t t) {
    if (kp_in_n_run(runs, n_runs, t)) return 4;
    return (int)((words[t >> 4] >> (2 * (t & 15))) & 3u);
}

// bit j set when column t0 + j lies in a run, j < width <= 32
KP_HD uint32_t kp_n_mask(const int32_t *runs, int n_runs, int32_t t0, int width) {
    uint32_t mask = 0;
    for (int a = kp_first_run_after(runs, n_runs, t0); a < n_runs && runs[2 * a] < t0 + width; ++a) {
        const int s = runs[2 * a] > t0 ? runs[2 * a] - t0 : 0, e = runs[2 * a + 1] - t0 < width ? runs[2 * a + 1] - t0 : width;
        if (e > s) mask |= (e >= 32 ? ~0u : (1u << e) - 1u) & ~((1u << s) - 1u);
    }
    return mask;
}

// ---- codes and their score ---------------------------------------------------------------------------------------------------
KP_HD unsigned kp_nib(unsigned word, int i) { return (word >> (4 * i)) & 15u; }

// query code against target code: anything above 3 (N, a row or column outside) scores as N
KP_HD int kp_sub_score(int qc, int tc) { return (qc > 3 || tc > 3) ? KP_SC_N : (qc == tc ? KP_SC_MATCH : KP_SC_MISMATCH); }

// the assembly side: packed words and N runs of the assembly, bounds of the contig
struct KpTargetSeq {
    const uint32_t *words;
    const int32_t *runs;
    int n_words, n_runs, cstart, cend;
    KP_HD int at(int t) const { return kp_code_at(words, runs, n_runs, t); }                  // t inside the contig
    KP_HD int code(int t) const { return (t < cstart || t >= cend) ? 5 : at(t); }  // 0..3, 4 = N, 5 = outside the contig
};

// the gene side: 4-bit codes (0..3, 4 = N) of one strand, eight per word
struct KpQuerySeq {
    const uint32_t *nib;
    int len;
    KP_HD int code(int r) const { return (int)kp_nib(nib[r >> 3], r & 7); }
};

// the two sequences of a band task, a join or a finished hit: the gene's strand as aligned and the contig (kp_walk.h: kp_task_seqs)
struct KpTaskSeqs {
    KpQuerySeq q;
    KpTargetSeq t;
};
