// kp_hits.h -- which band task and which piece of a join becomes a hit, and the raw record it becomes.  The hit compaction
// (kp_reduce.hip) appends these records; the CIGAR kernels (kp_cigar.hip) find a finished hit's source by building the same
// record again, so both ask here.  Device code only.
#pragma once

#include "kp_internal.h"
#include "kp_reduce_core.h"

// a band task: at or above the score cut-off and not consumed by a chain (`dropped`: task_drop, kp_join.hip)
__device__ __forceinline__ bool kp_task_hit(const KpBatchView &b, const int32_t *gene_len, const KpTask &t, const KpSwResult &r, bool dropped,
                                            kp_hit *hit) {
    if (r.score < KP_MIN_DP_SCORE || dropped) return false;
    const int32_t cs = b.ctg_start[b.asm_first_ctg[t.asm_id] + t.contig];
    *hit = kp_make_hit(t.gs, t.contig, cs, gene_len[t.gs >> 1], r.score, r.q_start, r.q_end, r.t_start, r.t_end, r.matches, r.block_len,
                       t.n_anchors, t.chain_score);
    return true;
}

// piece k of a join: the walk-back settled on the path that ends in it (state 1; res: kp_join_trace_kernel)
__device__ __forceinline__ bool kp_join_piece_hit(const KpBatchView &b, const int32_t *gene_len, const KpJoin &J, int k, kp_hit *hit) {
    if (J.state[k] != 1) return false;
    const int32_t cs = b.ctg_start[b.asm_first_ctg[J.asm_id] + J.contig];
    const int32_t *r = J.res[k];
    *hit = kp_make_hit(J.gs, J.contig, cs, gene_len[J.gs >> 1], (int)((uint32_t)r[7] | ((uint32_t)r[8] << KP_HIT_BONUS_SHIFT)), r[1], r[2], r[3],
                       r[4], r[5], r[6], J.n_anchors, J.chain_score);
    return true;
}
