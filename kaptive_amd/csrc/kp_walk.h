// kp_walk.h -- the two walks back along an alignment path, over the direction bits the fill kernels left: the band tasks'
// (kp_sw.hip: kp_sw_kernel / kp_sw_long_kernel) and the joins' (kp_join.hip: kp_join_fill_kernel).  Each is written once and
// takes a VISITOR that is told every run of columns the path makes, in walking order (from the path's end to its start):
// the tracebacks that reduce a path to the fields of its hit pass KpNoVisit, the CIGAR kernels (kp_cigar.hip) one that
// counts or writes run-length ops.  Ahead of them: the view of a task's two sequences that fills and walks read (kp_seqs.h) and
// the two steps the scalar fills share.  Device code only.
#pragma once

#include "kp_internal.h"
#include "kp_seqs.h"

#ifndef KP_TRACE_GROUP
#define KP_TRACE_GROUP 2
#endif

// Kinds of column, numbered as the ops of a CIGAR (kp_spec.h, CIGAR): a diagonal step, a step in state F (gap in the target,
// moves along the query) and a step in state E (gap in the query, moves along the target).
enum { KP_COL_M = 0, KP_COL_I = 1, KP_COL_D = 2 };

struct KpNoVisit {
    __device__ __forceinline__ void run(int, int) {}
};

// ---- the two sequences of a band task or a join ------------------------------------------------------------------------------
// (KpTaskSeqs itself: kp_seqs.h)
__device__ __forceinline__ KpTaskSeqs kp_task_seqs(const KpBatchView &b, const KpGenes &genes, int asm_id, int gs, int contig) {
    KpTaskSeqs s;
    const int gene = gs >> 1, c_abs = b.asm_first_ctg[asm_id] + contig, r0 = b.asm_first_nrun[asm_id];
    s.q.nib = genes.nib + genes.word_off[(gs & 1) ? genes.n_genes + gene : gene];
    s.q.len = genes.len[gene];
    s.t.words = b.words + b.asm_word_off[asm_id];
    s.t.n_words = (int)(b.asm_word_off[asm_id + 1] - b.asm_word_off[asm_id]);
    s.t.runs = b.n_runs + 2 * (size_t)r0;
    s.t.n_runs = b.asm_first_nrun[asm_id + 1] - r0;
    s.t.cstart = b.ctg_start[c_abs];
    s.t.cend = s.t.cstart + b.ctg_len[c_abs];
    return s;
}

// ---- shared by the fills: a task (a pair of them in the packed fill) belongs to a group of P lanes -----------------------------
// Room in the trace buffer: the group's leader (lane `leader` of the wave; `takes` is set in that lane alone) bumps the counter
// by `want` 16-byte units and every lane of the group gets the offset.
__device__ __forceinline__ unsigned long long kp_trace_take(unsigned long long *trace_top, bool takes, unsigned long long want, int leader) {
    unsigned long long toff = 0;
    if (takes) toff = atomicAdd(trace_top, want);
    return ((unsigned long long)__shfl((unsigned)(toff >> 32), leader) << 32) | __shfl((unsigned)toff, leader);
}
// Best cell over the group's lanes (the scalar fills; the packed one reduces a key): the largest score, then the first row, then the first column.
template <int P>
__device__ __forceinline__ void kp_group_best(int &best, int &best_r, int &best_b) {
#pragma unroll
    for (int o = 1; o < P; o <<= 1) {
        const int s2 = __shfl_xor(best, o), r2 = __shfl_xor(best_r, o), b2 = __shfl_xor(best_b, o);
        if (s2 > best || (s2 == best && (r2 < best_r || (r2 == best_r && b2 < best_b)))) { best = s2; best_r = r2; best_b = b2; }
    }
}

__device__ __forceinline__ uint32_t kp_piece_word(const uint4 &v, int k) {  // cell k's word of a piece, in registers' terms
    const uint32_t lo = (k & 1) ? v.y : v.x, hi = (k & 1) ? v.w : v.z;
    return (k & 2) ? hi : lo;
}

// ---- a band task's block of the trace buffer: the one rule both fills and every walk take its sizes and offsets from ----------
// P lane streams of `pieces` 16-byte pieces (8 steps x 4 cells; piece j of lane l at [j / TG][l][j % TG]: TG consecutive pieces
// of a lane are contiguous bytes), then the SUMMARIES: per lane and chunk of 64 steps (8 pieces) one 32-bit word, laid out
// [chunk][lane], that says of every cell and piece whether its word is "plain" -- eight diagonal steps, none the path's start:
// exactly (word & KP_PLAIN_MASK) == 0, the test the walk makes -- so that the walk need not fetch a piece to learn that one
// bit.  Cell k has byte k of the word; piece q of the chunk has bit 7 - q of that byte (set = NOT plain), so that the pieces a
// walk meets, going backwards, follow each other from a bit upwards.  Both parts are whole 128-byte lines (pieces: a multiple of
// four per lane and P >= 4; summaries: rounded up to eight units), so every block starts on one.
constexpr uint32_t KP_PLAIN_MASK = 0xAAAAAAAAu;  // the (inverted) D and L bits of a cell's eight steps
constexpr int KP_SUM_PIECES = 8;                 // pieces per summary word and lane

struct KpTraceBlock {
    int P;
    int pieces;     // per lane stream
    int sum_words;  // per lane stream
    __host__ __device__ uint32_t sum_off() const { return (uint32_t)P * (uint32_t)pieces; }  // 16-byte units from the block's start
    __host__ __device__ uint32_t units() const { return sum_off() + ((((uint32_t)P * (uint32_t)sum_words + 3u) / 4u + 7u) & ~7u); }
    __host__ __device__ size_t piece_at(int j, int l) const { return (size_t)(j / KP_TRACE_GROUP) * (KP_TRACE_GROUP * P) + KP_TRACE_GROUP * l + j % KP_TRACE_GROUP; }
    __host__ __device__ size_t sum_at(int chunk, int l) const { return (size_t)chunk * P + l; }  // 32-bit words from sum_off()
};
// steps = the steps the fill makes for the task: its rows (kp_task_rows) + P - 1, lane l works on row step - l; 0: no task
__host__ __device__ inline KpTraceBlock kp_trace_block(int P, int steps) {
    KpTraceBlock t;
    t.P = P;
    t.pieces = (((steps + 7) >> 3) + 3) & ~3;
    t.sum_words = (t.pieces + KP_SUM_PIECES - 1) / KP_SUM_PIECES;
    return t;
}
__host__ __device__ inline int kp_sum_bit(int cell, int piece) { return 8 * cell + 7 - (piece & 7); }

// ---- band tasks: one lane per task, whole waves together ---------------------------------------------------------------------
// Cell (row r, band index bi) sits on target position lo + r + bi; a diagonal step keeps bi, a step to the left (E, gap
// in the query) lowers it, a step up (F, gap in the target) raises it.  The nibble of (r, bi) is in lane stream bi / 4,
// step r + bi / 4: piece j = step / 8 (KpTraceBlock::piece_at), word bi % 4 (the cell); bit layout of a word: below.
//
// A path runs along a diagonal most of the time: it stays in one lane stream and cell and walks it backwards, through pieces
// that are plain.  Standing on the last step of a piece, the walk therefore asks the lane's summary word (it keeps the chunk's
// and the one below in registers) how many pieces from here down are plain and takes them all at once -- one bit scan, 8 n steps,
// one run for the visitor -- without fetching any of them.  What is not plain (the path's end piece, gaps, lane changes, the
// start) and tasks with an N, whose matches are counted base by base, goes step by step from 16-byte pieces held in registers.
// Pieces are fetched TG at a time (contiguous bytes: one trip to memory) and the next group the walk will need on this lane and
// cell -- the next one the summary calls not plain -- is requested as soon as the current one is, so the dependent fetches of a
// path overlap with its steps and with other waves' work.  With summaries = false (KAPTIVE_AMD_TRACE_SUMMARY=0: the A/B switch)
// the walk ignores them: it fetches every group on the path, the one before the current requested a group ahead, and learns
// "plain" from the piece itself.
// Matches: without an N in the gene or the window every diagonal step scores +2 or -4, so
// score = 6 * matches - 4 * diagonal_steps - gap_costs gives the matches in closed form; tasks that saw an N (flagged by
// the fill kernel) compare the bases of every diagonal step instead.
struct KpBandPath {
    int sr, sb;  // row and band index of the path's first cell
    int cols, matches /* counted base by base: has_n only */, diag, gap_cost, credit;
};

// Every lane of the wave calls it (walking = false: nothing to walk).  P = lanes of the task's band class, [q0, r_hi) = the rows
// the fill computed for the task (kp_task_rows), (er, eb) = its best cell, tw = the task's trace block.
template <class V>
__device__ __forceinline__ void kp_band_walk(bool walking, bool summaries, int lo, int P, int q0, int r_hi, int er, int eb, bool has_n,
                                             const uint4 *tw, const KpTaskSeqs &s, KpBandPath &out, V &v) {
    constexpr int TG = KP_TRACE_GROUP;
    constexpr int EX = KP_GAP_EXT;
    static_assert(KP_SUM_PIECES % TG == 0, "a group of pieces lies in one summary word");
    const KpTraceBlock blk = kp_trace_block(P, walking ? r_hi - q0 + P - 1 : 0);
    const uint32_t *sum = reinterpret_cast<const uint32_t *>(tw + blk.sum_off());
    int r = er, bi = eb, state = 0, cols = 0, matches = 0, diag = 0, gap_cost = 0, gap = 0, credit = 0;
    int sr = r, sb = bi;
    // curq = the TG pieces (contiguous bytes) of the lane stream the walk stands in, nxtq = the group requested ahead.
    // A group is fetched with loads in a row: one trip to memory --
    // with a load per piece the line had left the L2 by the time the walk came back for the next one (75 % misses,
    // one random 64-byte fetch per piece: the kernel ran at the rate HBM serves those, tools/microbench/l2_gather.hip)
    uint4 curq[TG], nxtq[TG];
#pragma unroll
    for (int i = 0; i < TG; ++i) curq[i] = nxtq[i] = make_uint4(0, 0, 0, 0);
    int cur_tag = -1, nxt_tag = -1;  // (stream << 20) | group index
    // the lane's summary words of the chunk the walk stands in and of the one below (all ones where there is none: nothing to skip)
    uint32_t s_cur = ~0u, s_low = ~0u;
    int s_tag = -1;  // (stream << 20) | chunk
    // plain pieces of cell k from piece `pc` of chunk `ch` downwards, as far as the two words in hand tell (the walk stands in
    // chunk ch or in the one above its first piece); `known` = false: all of them were plain, the run may go on below
    auto plain_run = [&](int k, int pc, bool &known) -> int {
        const int p = pc & 7;
        const uint32_t hi = ((s_cur >> (8 * k)) & 255u) >> (7 - p);  // bits 0 .. p: pieces p .. 0
        int n = __ffs((int)(hi | (1u << (p + 1)))) - 1;
        known = n <= p;
        if (!known) {
            const int m = __ffs((int)(((s_low >> (8 * k)) & 255u) | 256u)) - 1;  // pieces 7 .. 0 of the chunk below
            n += m;
            known = m < 8;
        }
        return n;
    };
    while (__any(walking)) {
        if (!walking) continue;
        const int l = bi >> 2, k = bi & 3, step = r - q0 + l;
        const int pc = step >> 3, grp = pc / TG, tag = (l << 20) | grp;
        if (summaries) {
            const int ch = pc / KP_SUM_PIECES, stag = (l << 20) | ch;
            if (stag != s_tag) {  // (the word below was requested when the walk entered the chunk above: it is here by now)
                s_cur = stag + 1 == s_tag && (s_tag & 0xFFFFF) != 0 ? s_low : sum[blk.sum_at(ch, l)];
                s_low = ch > 0 ? sum[blk.sum_at(ch - 1, l)] : ~0u;
                s_tag = stag;
            }
            if (state == 0 && !has_n && (step & 7) == 7) {
                bool known;
                // (a path's first piece is never plain -- above row q0 every H is 0, so its first step is a start or not diagonal --;
                // the run is kept off piece 0 all the same, so that no trace content can take the walk above its first step)
                const int n = min(plain_run(k, pc, known), pc);
                if (n > 0) {  // 8 n plain diagonal steps (a diagonal step stays on its lane and cell)
                    cols += 8 * n; diag += 8 * n; r -= 8 * n;
                    v.run(KP_COL_M, 8 * n);
                    continue;
                }
            }
        }
        if (tag != cur_tag) {
            if (tag == nxt_tag) {
#pragma unroll
                for (int i = 0; i < TG; ++i) curq[i] = nxtq[i];
            } else {
#pragma unroll
                for (int i = 0; i < TG; ++i) curq[i] = tw[blk.piece_at(grp * TG, l) + i];
            }
            cur_tag = tag;
            // ahead: the group before this one, or -- told by the summaries -- the next one below it that is not all plain
            int ahead = grp - 1;
            if (summaries && !has_n && grp > 0) {  // (a task with an N visits every piece: the group before)
                // (the first piece of a group is never the first of a chunk's upper neighbour: KP_SUM_PIECES % TG == 0, so the
                // pieces below the group start in this chunk or are the whole chunk below)
                bool known;
                const int first = grp * TG;  // the group's first piece
                int n;
                if (first & 7) n = plain_run(k, first - 1, known);
                else { n = __ffs((int)(((s_low >> (8 * k)) & 255u) | 256u)) - 1; known = n < 8; }
                ahead = known && first - 1 - n >= 0 ? (first - 1 - n) / TG : -1;
            }
            if (ahead >= 0) {
#pragma unroll
                for (int i = 0; i < TG; ++i) nxtq[i] = tw[blk.piece_at(ahead * TG, l) + i];
                nxt_tag = (l << 20) | ahead;
            }
        }
        uint4 cur = (pc & 1) ? curq[1] : curq[0];
        if (TG == 4) {
            const uint4 hi2 = (pc & 1) ? curq[TG - 1] : curq[TG - 2];
            cur = (pc & 2) ? hi2 : cur;
        }
        const uint32_t word = kp_piece_word(cur, k);
        if (!summaries && state == 0 && !has_n && (step & 7) == 7 && (word & KP_PLAIN_MASK) == 0u) {  // eight plain diagonal steps (D and L are stored inverted)
            cols += 8; diag += 8; r -= 8;
            v.run(KP_COL_M, 8);
            continue;
        }
        // a cell's word: steps 0-3 in the low half, 4-7 in the high half; per half a byte of [L, F opened] pairs below
        // a byte of [D, E opened] pairs, step j's pair at bits 2j+1, 2j
        const uint32_t half = word >> (16 * ((step >> 2) & 1)), sh = 2 * (step & 3);
        const uint32_t de = ((half >> (8 + sh)) & 3u) ^ 2u, lf = ((half >> sh) & 3u) ^ 2u;  // (D, L: stored inverted)
        const uint32_t nib = ((de & 2u) << 2) | ((lf & 2u) << 1) | ((de & 1u) << 1) | (lf & 1u);  // [D][L][EO][FO]
        // -> source 0 = diagonal, 1 = diagonal and the path starts here, 2 = E, 3 = F
        const uint32_t src = (nib & 8u) ? ((nib & 4u) ? 0u : 1u) : ((nib & 4u) ? 2u : 3u);
        if (state == 0) {
            if (src <= 1u) {  // diagonal: one column
                ++cols; ++diag;
                v.run(KP_COL_M, 1);
                if (has_n) {  // a match when both bases are the same unambiguous base
                    const int qc = s.q.code(r), tc = s.t.at(lo + r + bi);
                    matches += (qc == tc && qc < 4) ? 1 : 0;  // N against N scores KP_SC_N: not a match
                }
                if (src == 1u) { sr = r; sb = bi; walking = false; }
                --r;
            } else {
                state = (int)src - 1;  // 1 = E, 2 = F: the gap's columns are counted in that state
            }
        } else if (state == 1) {  // E: gap in the query; this cell's E came from H (opened) or E (extended) of the left cell
            ++cols; ++gap; gap_cost += EX;
            v.run(KP_COL_D, 1);
            --bi;
            if (nib & 2u) { state = 0; gap_cost += KP_GAP_OPEN; credit += max(gap - KP_GAP_LONG, 0); gap = 0; }
        } else {  // F: gap in the target
            ++cols; ++gap; gap_cost += EX;
            v.run(KP_COL_I, 1);
            --r; ++bi;
            if (nib & 1u) { state = 0; gap_cost += KP_GAP_OPEN; credit += max(gap - KP_GAP_LONG, 0); gap = 0; }
        }
    }
    out.sr = sr; out.sb = sb; out.cols = cols; out.matches = matches; out.diag = diag; out.gap_cost = gap_cost; out.credit = credit;
}

// ---- joins: one lane per join, a path from the best cell of piece k back through the cross gaps ----------------------------
// Direction byte of a cell: bits 0-2 the source of H (XT_*), bit 3 "E was extended", bit 4 "F was extended".
enum { XT_DIAG = 0, XT_E = 1, XT_F = 2, XT_RESTART = 3, XT_X1 = 4, XT_X2 = 5 };

struct KpJoinPath {
    bool rejected;  // by the drop test (kp_spec.h, THE JOINED PATH)
    int visited;    // mask of the pieces the path runs through
    int sr, sb, spk;  // row, band index and piece of the path's first cell
    int matches, cols, credit, bonus;
};

// A cross gap along a row (the later piece lies on higher diagonals) is a gap in the query: KP_COL_D; one down a column a
// gap in the target: KP_COL_I.
template <class V>
__device__ __forceinline__ void kp_join_walk(const KpJoin *J, int k, int P, const KpTaskSeqs &s, const uint4 *trace, KpJoinPath &out, V &v) {
    const int W = 4 * P;
    int pk = k, r = J->end_r[k], bi = J->end_b[k], state = 0, matches = 0, cols = 0, gap = 0, credit = 0;
    int sr = r, sb = bi, spk = k, suf = 0, sufmax = 0, gsum = 0, visited = 1 << k, bonus = 0;
    bool rejected = false;
    int lo = J->lo[pk], q0 = 0, r_hi = 0;
    kp_piece_rows(lo, W, s.t.cstart, s.t.cend, s.q.len, J->r0[pk], J->r1[pk], &q0, &r_hi);
    const uint32_t *tr = reinterpret_cast<const uint32_t *>(trace + J->trace_off[pk]);
    for (;;) {
        const int t = r + lo + bi;
        if (state == 0 && (r < q0 || r >= r_hi || bi < 0 || bi >= W || t < s.t.cstart || t >= s.t.cend)) break;
        const uint32_t byte = (tr[(size_t)(r - q0 + (bi >> 2)) * P + (bi >> 2)] >> (8 * (bi & 3))) & 255u;
        if (state == 0) {
            const uint32_t tb = byte & 7u;
            if (tb == XT_RESTART) break;
            // the drop test: at every cross gap, and at every cell once a gap has been crossed (cross-gap costs left out)
            if (suf + gsum > sufmax) sufmax = suf + gsum;
            else if ((tb >= XT_X1 || visited != (1 << k)) && sufmax - (suf + gsum) > KP_JOIN_DROP) { rejected = true; break; }
            if (tb == XT_DIAG) {
                sr = r; sb = bi; spk = pk; ++cols;
                v.run(KP_COL_M, 1);
                const int qc = s.q.code(r), tc = s.t.at(t);
                if (qc < 4 && qc == tc) ++matches;
                suf += kp_sub_score(qc, tc);
                --r;
            } else if (tb == XT_E || tb == XT_F) {
                state = (int)tb;
            } else {  // a cross gap: on to the cell of piece pk - 1 it came from
                const int lo_prev = J->lo[pk - 1];
                const bool horizontal = lo > lo_prev;
                const unsigned long long *exp = reinterpret_cast<const unsigned long long *>(trace + J->export_off[pk - 1]);
                const int xi = horizontal ? r : t - lo_prev;
                const unsigned long long key = exp[2 * xi + (tb == XT_X1 ? 0 : 1)];
                const int pos = (int)(0xFFFFFFFFu - (uint32_t)key);  // t' - lo_prev (horizontal) or r'
                const int ngap = horizontal ? (t - lo_prev) - pos : r - pos;
                cols += ngap;
                v.run(horizontal ? KP_COL_D : KP_COL_I, ngap);
                const int cost = tb == XT_X1 ? KP_GAP_OPEN + KP_GAP_EXT * ngap : KP_GAP_OPEN2 + KP_GAP_EXT2 * ngap;
                suf -= cost; gsum += cost;
                const int lg = KP_GAP_OPEN + kp_log2x2((uint32_t)ngap);
                if (cost > lg) bonus += cost - lg;
                if (horizontal) bi = pos - r;               // same row, column lo_prev + pos
                else { bi = t - pos - lo_prev; r = pos; }   // same column, row pos
                --pk; visited |= 1 << pk;
                lo = lo_prev;
                kp_piece_rows(lo, W, s.t.cstart, s.t.cend, s.q.len, J->r0[pk], J->r1[pk], &q0, &r_hi);
                tr = reinterpret_cast<const uint32_t *>(trace + J->trace_off[pk]);
            }
        } else if (state == XT_E) {
            ++cols; ++gap; --bi; suf -= KP_GAP_EXT;
            v.run(KP_COL_D, 1);
            if (!(byte & 8u)) { state = 0; suf -= KP_GAP_OPEN; credit += max(gap - KP_GAP_LONG, 0); gap = 0; }
        } else {
            ++cols; ++gap; --r; ++bi; suf -= KP_GAP_EXT;
            v.run(KP_COL_I, 1);
            if (!(byte & 16u)) { state = 0; suf -= KP_GAP_OPEN; credit += max(gap - KP_GAP_LONG, 0); gap = 0; }
        }
    }
    out.rejected = rejected; out.visited = visited; out.sr = sr; out.sb = sb; out.spk = spk;
    out.matches = matches; out.cols = cols; out.credit = credit; out.bonus = bonus;
}
