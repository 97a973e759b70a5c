// kp_rescue.hip -- translated search of the missing locus genes (kp_spec.h, RESCUE; made when the records are first asked for).
//
// On the reduction's stream, behind the kernels that finalise the summaries and the pieces.  The kernels read the summaries' missing
// masks, the pieces, the packed contigs with their N runs and the database's proteins: no hit table, no op, no trace.
//
//   kp_rescue_plan_kernel   one block per assembly: every subject (set bit of the missing mask, ascending) gets its record slot, filled
//                           with the "nothing found" record, and one unit per piece -- the window of the piece on its contig
//                           (kp_rescue.h).  A unit is six tasks: two strands x three frames.  ctl[KP_RS_CTL_ROWS] ends up as the longest
//                           frame text of any subject whose protein needs strips: the host sizes the boundary scratch from it.
//   kp_rescue_fill_kernel   one wave per block; the waves take tasks off a counter, as kp_protein_wide_kernel takes pairs.  Lane l
//                           holds NC adjacent COLUMNS of the protein (its residues stay in registers for the whole task) and works on
//                           row i = t - l + 1 of the frame text at step t: the left neighbour of its first column is what lane l - 1
//                           computed a step earlier (one DPP wave shift per value), every other neighbour is one of its own
//                           registers.  The frame text is never materialised: every 64 steps the wave translates the next 64 residues
//                           from the packed words, one per lane, into a ring of 128 in LDS.  A protein longer than 64 x 6 residues is
//                           cut into strips of 384 columns; the last column of a strip (M and I per row, with their path statistics
//                           where carried) goes through a scratch buffer in global memory, 64 rows at a time in both directions
//                           through LDS, as the row buffer of kp_prot.hip's strips does.
//                           <false>: the lean cell (prot_cell_lean: three scores, no path statistics) over all six frames of every
//                           unit; leaves score and best cell per task.
//                           <true>: one item per subject, after kp_rescue_pick_kernel: the winning task again with prot_cell's path
//                           statistics, over the rows and columns up to its best cell only (the first maximum of that rectangle is the
//                           same cell: every cell of it has the value it has in the whole matrix); then the derived fields, the
//                           stops of the aligned stretch counted by the lanes, and the record.
//   kp_rescue_pick_kernel   one thread per subject: the best task, ties to the lowest task index.
//
// Every loop is bounded by a length fixed before the launch (tasks, rows of a window, columns of a protein); no wave waits for
// another.  One record per subject is exact, so no buffer can overflow and nothing is retried.
#include <algorithm>

#include "kp_internal.h"
#include "kp_reduce_core.h"
#include "kp_rescue.h"
#include "kp_prot_cell.h"

namespace {

constexpr int RS_WAVE = KP_RS_LANES;
constexpr int RS_RING = 2 * RS_WAVE;  // residues of the frame text in LDS: the chunk being read and the one before it
constexpr int RS_FIELDS = KP_RS_SCRATCH_FIELDS;  // per row of a strip's last column: M, I, payload of M (2), payload of I (2)

// the set bit number s of the mask (s < its population count), KP_MAX_LOCUS_GENES otherwise
__device__ __forceinline__ int nth_missing(const uint64_t *mask, int s) {
    for (int w = 0; w < KP_MAX_LOCUS_GENES / 64; ++w) {
        const int c = __popcll(mask[w]);
        if (s < c) {
            uint64_t m = mask[w];
            for (int x = 0; x < s; ++x) m &= m - 1;  // (s < 64)
            return 64 * w + (__ffsll((long long)m) - 1);
        }
        s -= c;
    }
    return KP_MAX_LOCUS_GENES;
}

__global__ __launch_bounds__(RS_WAVE) void kp_rescue_plan_kernel(KpBatchView b, KpTypingDb db, const KpAsmSummary *__restrict__ summary,
                                                                 const KpPiece *__restrict__ pieces, int piece_cap, int flank,
                                                                 const int64_t *__restrict__ rec_off, const int64_t *__restrict__ unit_off,
                                                                 KpRescueUnit *__restrict__ units, int32_t *__restrict__ sub,
                                                                 kp_rescue *__restrict__ rec, int32_t *__restrict__ ctl) {
    const int a = blockIdx.x;
    if (a >= b.n_asm) return;
    const int64_t r0 = rec_off[a], u0 = unit_off[a];
    const int n_rec = (int)(rec_off[a + 1] - r0);
    if (n_rec <= 0) return;
    const int np = (int)((unit_off[a + 1] - u0) / n_rec);  // pieces of the assembly, as the host laid the units out
    const KpAsmSummary &S = summary[a];
    const int c0 = b.asm_first_ctg[a], n_ctg = b.asm_first_ctg[a + 1] - c0;
    const int g0 = (S.best_locus >= 0 && S.best_locus < db.n_loci) ? db.locus_gene_off[S.best_locus] : -1;
    int strip_rows = 0;
    for (int s = threadIdx.x; s < n_rec; s += RS_WAVE) {
        const int j = nth_missing(S.missing_mask, s);
        const int gene = (g0 >= 0 && j < KP_MAX_LOCUS_GENES && g0 + j < db.n_genes) ? g0 + j : -1;
        kp_rescue z{};
        z.gene = gene; z.piece = -1;
        rec[r0 + s] = z;
        int32_t *sb = sub + 4 * (r0 + s);
        sb[0] = (int32_t)(u0 + (int64_t)s * np); sb[1] = np; sb[2] = -1; sb[3] = 0;
        const bool strips = gene >= 0 && kp_rs_needs_strips(db.prot_len[gene]);
        for (int p = 0; p < np; ++p) {
            const KpPiece &pc = pieces[(size_t)a * piece_cap + p];
            KpRescueUnit u{a, (int32_t)(r0 + s), gene, p, pc.contig, 0, 0, 0};
            if (pc.contig >= 0 && pc.contig < n_ctg) {
                const int32_t cstart = b.ctg_start[c0 + pc.contig], clen = b.ctg_len[c0 + pc.contig];
                const int64_t words = b.asm_word_off[a + 1] - b.asm_word_off[a];
                // (a contig that does not lie inside the assembly's packed words has no window: nothing of it is read)
                if (cstart >= 0 && clen >= 0 && (int64_t)cstart + clen <= 16 * words && kp_rs_window(pc.start, pc.end, clen, flank, &u.ws, &u.we)) u.ctg_len = clen;
            }
            units[u0 + (int64_t)s * np + p] = u;
            if (strips) strip_rows = max(strip_rows, kp_rs_frame_len(u.ws, u.we, 0));
        }
    }
    if (strip_rows > 0) atomicMax(ctl + KP_RS_CTL_ROWS, strip_rows);
}

// the frame text of a task and where it is read from
struct RsText {
    KpTargetSeq t;
    int32_t ws, we;
    int strand, f;
    bool clear;
};

__device__ __forceinline__ RsText rs_text(const KpBatchView &b, const KpRescueUnit &u, int sf) {
    RsText q;
    const int a = u.asm_id, c0 = b.asm_first_ctg[a], r0 = b.asm_first_nrun[a];
    q.t.words = b.words + b.asm_word_off[a];
    q.t.n_words = (int)(b.asm_word_off[a + 1] - b.asm_word_off[a]);
    q.t.runs = b.n_runs + 2 * (size_t)r0;
    q.t.n_runs = b.asm_first_nrun[a + 1] - r0;
    q.t.cstart = b.ctg_start[c0 + u.contig];
    q.t.cend = q.t.cstart + u.ctg_len;
    q.ws = u.ws; q.we = u.we;
    q.strand = kp_rs_task_strand(sf); q.f = kp_rs_task_frame(sf);
    q.clear = kp_rs_clear_of_runs(q.t, u.ws, u.we);
    return q;
}

struct RsLds {
    uint16_t res[RS_RING];          // residues of the frame text: raw byte << 8 | BLOSUM index
    int in[RS_FIELDS][RS_WAVE];     // rows of the previous strip's last column, published a chunk at a time
    int out[RS_FIELDS][RS_WAVE];    // rows of this strip's last column, collected by lane 63
    int8_t mat[32 * 32];
    uint8_t idx[256];
    uint8_t codon[128];
};

// One strip of columns j0 + 1 .. j0 + 64 NC (those <= P exist) against rows 1 .. A.  `first`: no strip to the left (the boundary column
// is the matrix's: M = 0, I = -inf); `last`: none to the right (nothing is handed on).  bnd: the block's scratch, `stride` ints per field.
template <int NC, bool PAY, bool MULTI>
__device__ __forceinline__ void rs_strip(const RsText &q, const uint8_t *__restrict__ prot, int P, int A, int j0, bool first, bool last,
                                         int32_t *__restrict__ bnd, int stride, RsLds &L, int lane, Result &r, LeanBest &lb) {
    constexpr int NF = PAY ? RS_FIELDS : 2;
    unsigned c2[NC];
    int m[NC], dv[NC];
    Pay pm[NC], pd[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int j = j0 + NC * lane + c + 1;
        c2[c] = 0;
        if (j <= P) { const uint8_t x = prot[j - 1]; c2[c] = ((unsigned)x << 8) | L.idx[x]; }
        m[c] = 0; dv[c] = NEGP; pm[c] = Pay{0, 0}; pd[c] = Pay{0, 0};
    }
    int last_iv = NEGP, dm = 0;
    Pay last_pi{0, 0}, dpm{0, 0};
    int ahead[NF];
    auto fetch = [&](int row) {  // row `row` of the previous strip's last column, or the matrix's boundary
        ahead[0] = 0; ahead[1] = NEGP;
#pragma unroll
        for (int f = 2; f < NF; ++f) ahead[f] = 0;
        if (!first && row <= A) {
#pragma unroll
            for (int f = 0; f < NF; ++f) ahead[f] = bnd[(size_t)f * stride + row];
        }
    };
    fetch(1 + lane);
    const int n_steps = A + RS_WAVE - 1;
    for (int t = 0; t < n_steps; ++t) {
        if ((t & (RS_WAVE - 1)) == 0) {  // wave-uniform: the next 64 residues of the frame text, the next 64 rows of the boundary column
            const int a = t + lane;
            unsigned v = 0;
            if (a < A) { const uint8_t x = kp_rs_residue(q.t, L.codon, q.ws, q.we, q.strand, q.f, a, q.clear); v = ((unsigned)x << 8) | L.idx[x]; }
            __syncthreads();  // (a block is one wave: orders these stores after the reads of the chunk they replace)
            L.res[a & (RS_RING - 1)] = (uint16_t)v;
#pragma unroll
            for (int f = 0; f < NF; ++f) L.in[f][lane] = ahead[f];
            __syncthreads();
            fetch(t + RS_WAVE + 1 + lane);
        }
        const int i = t - lane + 1;
        const bool row_ok = i >= 1 && i <= A;
        const unsigned c1 = row_ok ? L.res[(i - 1) & (RS_RING - 1)] : 0u;
        // left neighbour of the lane's first column: lane l - 1's last column at this row (it was there a step ago)
        int lm = from_lower(m[NC - 1]), li = from_lower(last_iv);
        Pay lpm{0, 0}, lpi{0, 0};
        if constexpr (PAY) {
            lpm = Pay{(unsigned)from_lower((int)pm[NC - 1].a), (unsigned)from_lower((int)pm[NC - 1].g)};
            lpi = Pay{(unsigned)from_lower((int)last_pi.a), (unsigned)from_lower((int)last_pi.g)};
        }
        if (lane == 0) {
            const int s = t & (RS_WAVE - 1);
            lm = L.in[0][s]; li = L.in[1][s];
            if constexpr (PAY) { lpm = Pay{(unsigned)L.in[2][s], (unsigned)L.in[3][s]}; lpi = Pay{(unsigned)L.in[4][s], (unsigned)L.in[5][s]}; }
        }
        const int next_dm = lm;
        const Pay next_dpm = lpm;
        int diag_m = dm, left_m = lm, left_i = li;
        Pay diag_pm = dpm, left_pm = lpm, left_pi = lpi;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int j = j0 + NC * lane + c + 1;
            const bool in = row_ok && j <= P;
            const int up_m = m[c];
            if constexpr (PAY) {
                const Pay up_pm = pm[c];
                PCell x;
                x.m = diag_m; x.pm = diag_pm;
                prot_cell<!MULTI>(x, r, in, i, j, c1, c2[c], L.mat, left_m, left_i, left_pm, left_pi, up_m, dv[c], up_pm, pd[c]);
                diag_pm = up_pm;
                m[c] = x.m; dv[c] = x.dv; pm[c] = x.pm; pd[c] = x.pd;
                left_m = x.m; left_i = x.iv; left_pm = x.pm; left_pi = x.pi;
            } else {
                int xm = diag_m, xd, xi;
                prot_cell_lean<!MULTI>(xm, xd, xi, lb, in, i, j, c1, c2[c], L.mat, left_m, left_i, up_m, dv[c]);
                m[c] = xm; dv[c] = xd;
                left_m = xm; left_i = xi;
            }
            diag_m = up_m;
        }
        last_iv = left_i; last_pi = left_pi;
        dm = next_dm; dpm = next_dpm;
        // the strip's last column goes to the next strip: lane 63 collects its rows in LDS, every 64 rows (and at the last row) the
        // whole wave writes them out, one row per lane
        const int io = t - (RS_WAVE - 1) + 1;  // lane 63's row: wave-uniform
        if (!last && io >= 1 && io <= A) {
            const int slot = (io - 1) & (RS_WAVE - 1);
            if (lane == RS_WAVE - 1) {
                L.out[0][slot] = m[NC - 1]; L.out[1][slot] = last_iv;
                if constexpr (PAY) {
                    L.out[2][slot] = (int)pm[NC - 1].a; L.out[3][slot] = (int)pm[NC - 1].g;
                    L.out[4][slot] = (int)last_pi.a; L.out[5][slot] = (int)last_pi.g;
                }
            }
            if (slot == RS_WAVE - 1 || io == A) {
                __syncthreads();
                if (lane <= slot) {
#pragma unroll
                    for (int f = 0; f < NF; ++f) bnd[(size_t)f * stride + (io - slot + lane)] = L.out[f][lane];
                }
                __syncthreads();
            }
        }
    }
}

// the whole matrix of one task: rows 1 .. A of the frame text, columns 1 .. P of the protein
template <int NC, bool PAY, bool MULTI>
__device__ __forceinline__ void rs_matrix(const RsText &q, const uint8_t *__restrict__ prot, int P, int A, int32_t *__restrict__ bnd, int stride,
                                          RsLds &L, int lane, Result &r, LeanBest &lb) {
    constexpr int W = RS_WAVE * NC;
    for (int j0 = 0; j0 < P; j0 += W) {
        if (MULTI) {  // the previous strip's stores (every lane's) are visible to every lane's loads
            __threadfence_block();
            __syncthreads();
        }
        rs_strip<NC, PAY, MULTI>(q, prot, P, A, j0, j0 == 0, j0 + W >= P, bnd, stride, L, lane, r, lb);
    }
}

template <bool PAY>
__device__ __forceinline__ void rs_task(const RsText &q, const uint8_t *__restrict__ prot, int P, int A, int32_t *__restrict__ bnd, int stride,
                                        RsLds &L, int lane, Result &r, LeanBest &lb) {
    const int nc = kp_rs_cols_per_lane(P);
    if (nc == KP_RS_NC_SMALL) rs_matrix<KP_RS_NC_SMALL, PAY, false>(q, prot, P, A, bnd, stride, L, lane, r, lb);
    else if (nc == KP_RS_NC_MID) rs_matrix<KP_RS_NC_MID, PAY, false>(q, prot, P, A, bnd, stride, L, lane, r, lb);
    else if (!kp_rs_needs_strips(P)) rs_matrix<KP_RS_NC_WIDE, PAY, false>(q, prot, P, A, bnd, stride, L, lane, r, lb);
    else if (bnd && A < stride) rs_matrix<KP_RS_NC_WIDE, PAY, true>  // (stride: rows + 1 the scratch holds per field -- the plan sized it for every such task)
       (q, prot, P, A, bnd, stride, L, lane, r, lb);
}

// the lanes' best cells into one: the highest score, then the smallest row, then the smallest column
__device__ __forceinline__ Result rs_reduce(Result r) {
#pragma unroll
    for (int off = 1; off < RS_WAVE; off <<= 1) {
        const int b2 = __shfl_xor(r.best, off), i2 = __shfl_xor(r.bi, off), j2 = __shfl_xor(r.bj, off);
        const unsigned a2 = __shfl_xor(r.bp.a, off), g2 = __shfl_xor(r.bp.g, off);
        if (b2 > r.best || (b2 == r.best && b2 > 0 && (i2 < r.bi || (i2 == r.bi && j2 < r.bj)))) r = Result{b2, i2, j2, Pay{a2, g2}};
    }
    return r;
}

template <bool PAY>
__global__ __launch_bounds__(RS_WAVE) void kp_rescue_fill_kernel(KpBatchView b, KpTypingDb db, const int8_t *__restrict__ blosum,
                                                                 const KpRescueUnit *__restrict__ units, int32_t n_items,
                                                                 int32_t *__restrict__ cell, int32_t *__restrict__ sub, kp_rescue *__restrict__ rec,
                                                                 int32_t *__restrict__ queue, int32_t *__restrict__ scratch,
                                                                 size_t scratch_per_block, int stride, int edge_tol) {
    __shared__ RsLds L;
    const int lane = threadIdx.x;
    int32_t *const bnd = scratch ? scratch + (size_t)blockIdx.x * scratch_per_block : nullptr;
    bool staged = false;
    for (;;) {  // (at most n_items turns over all waves: the counter only rises)
        int item = 0;
        if (lane == 0) item = atomicAdd(queue, 1);
        item = __shfl(item, 0);
        if (item >= n_items) break;
        int task = item, rows_cap = 0x7FFFFFFF, cols_cap = 0x7FFFFFFF;
        if constexpr (PAY) {  // item: a subject; its winning task, up to its best cell
            task = sub[4 * (size_t)item + 2];
            if (task < 0) continue;
            rows_cap = cell[4 * (size_t)task + 1]; cols_cap = cell[4 * (size_t)task + 2];
        }
        const KpRescueUnit u = units[task / KP_RS_FRAMES];
        const int sf = task % KP_RS_FRAMES;
        const int A = min(kp_rs_frame_len(u.ws, u.we, kp_rs_task_frame(sf)), rows_cap);
        const int P = u.gene >= 0 ? min(db.prot_len[u.gene], cols_cap) : 0;
        Result r{0, 0, 0, Pay{0, 0}};
        LeanBest lb{0, 0, 0};
        RsText q{};
        if (A > 0 && P > 0) {
            if (!staged) {
                stage_blosum(blosum, L.mat, L.idx, lane);
                if (lane == 0) kp_fill_codon_table(L.codon);
                __syncthreads();
                staged = true;
            }
            q = rs_text(b, u, sf);
            rs_task<PAY>(q, db.prot + db.prot_off[u.gene], P, A, bnd, stride, L, lane, r, lb);
        }
        if constexpr (!PAY) {
            r = rs_reduce(Result{lb.best, lb.bi, lb.bj, Pay{0, 0}});
            if (lane == 0) {
                int32_t *o = cell + 4 * (size_t)task;
                o[0] = r.best; o[1] = r.bi; o[2] = r.bj; o[3] = 0;
            }
            continue;
        }
        r = rs_reduce(r);
        if (r.best <= 0) continue;  // (the plan's "nothing found" record stands)
        const int n_m = (int)(r.bp.a >> 16), n_mm = (int)(r.bp.a & 0xFFFFu), g_row = (int)(r.bp.g >> 16), g_col = (int)(r.bp.g & 0xFFFFu);
        const int a0 = r.bi - (n_m + n_mm + g_row), a1 = r.bi;
        int stops = 0;
        for (int a = a0 + lane; a < a1; a += RS_WAVE) stops += kp_rs_residue(q.t, L.codon, q.ws, q.we, q.strand, q.f, a, q.clear) == '*';
#pragma unroll
        for (int off = 1; off < RS_WAVE; off <<= 1) stops += __shfl_xor(stops, off);
        if (lane == 0) {
            kp_rescue z{};
            z.gene = u.gene; z.piece = u.piece; z.contig = u.contig;
            kp_rs_coords(u.ws, u.we, q.strand, q.f, a0, a1, &z.t_start, &z.t_end);
            z.score = r.best; z.matches = n_m; z.mismatches = n_mm; z.gaps = g_row + g_col;
            z.p_start = r.bj - (n_m + n_mm + g_col); z.p_end = r.bj;
            z.stops = stops; z.a_len = kp_rs_frame_len(u.ws, u.we, q.f);
            z.strand = (int8_t)q.strand; z.frame = (uint8_t)q.f;
            z.edge = kp_rs_edge(z.t_start, z.t_end, u.ctg_len, edge_tol);
            rec[u.rec] = z;
        }
    }
}

// best task of every subject: the highest score, ties to the lowest task index
__global__ __launch_bounds__(256) void kp_rescue_pick_kernel(const int32_t *__restrict__ cell, int32_t *__restrict__ sub, int64_t n_rec) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rec) return;
    int32_t *sb = sub + 4 * r;
    const int64_t t0 = (int64_t)sb[0] * KP_RS_FRAMES, n = (int64_t)sb[1] * KP_RS_FRAMES;
    int best = 0, win = -1;
    for (int64_t t = 0; t < n; ++t) {
        const int s = cell[4 * (t0 + t)];
        if (s > best) { best = s; win = (int32_t)(t0 + t); }
    }
    sb[2] = win;
}

}  // namespace

void kp_launch_rescue_plan(const KpBatchView &b, const KpTypingDb &db, const kp_asm_summary *summary, const kp_piece *pieces, int piece_cap, int flank,
                           const KpRescueTables &t, hipStream_t stream) {
    if (b.n_asm <= 0 || t.n_rec <= 0) return;
    hipLaunchKernelGGL(kp_rescue_plan_kernel, dim3((unsigned)b.n_asm), dim3(RS_WAVE), 0, stream, b, db, summary, pieces, piece_cap, flank, t.rec_off,
                       t.unit_off, t.units, t.sub, t.rec, t.ctl);
}

void kp_launch_rescue_fill(const KpBatchView &b, const KpTypingDb &db, const int8_t *blosum, int edge_tolerance, const KpRescueTables &t, int n_blocks,
                           hipStream_t stream) {
    if (t.n_rec <= 0 || t.n_units <= 0 || n_blocks <= 0) return;
    const int32_t n_tasks = (int32_t)(t.n_units * KP_RS_FRAMES);
    const int stride = t.scratch ? (int)(t.scratch_per_block / KP_RS_SCRATCH_FIELDS) : 0;  // ints between the fields of a block's scratch
    hipLaunchKernelGGL(kp_rescue_fill_kernel<false>, dim3((unsigned)std::min<int64_t>(n_blocks, n_tasks)), dim3(RS_WAVE), 0, stream, b, db, blosum, t.units,
                       n_tasks, t.cell, t.sub, t.rec, t.ctl + KP_RS_CTL_QUEUE, t.scratch, t.scratch_per_block, stride, edge_tolerance);
    hipLaunchKernelGGL(kp_rescue_pick_kernel, dim3((unsigned)((t.n_rec + 255) / 256)), dim3(256), 0, stream, t.cell, t.sub, t.n_rec);
    hipLaunchKernelGGL(kp_rescue_fill_kernel<true>, dim3((unsigned)std::min<int64_t>(n_blocks, t.n_rec)), dim3(RS_WAVE), 0, stream, b, db, blosum, t.units,
                       (int32_t)t.n_rec, t.cell, t.sub, t.rec, t.ctl + KP_RS_CTL_QUEUE2, t.scratch, t.scratch_per_block, stride, edge_tolerance);
}
