// kp_cigar.hip -- CIGARs of the finished hits (kp_spec.h, CIGAR; only with the `cigar` option).
//
// The reference asks its aligner for them (Aligner(..., do_cigar=True), src/kaptive/serotyping/core.py:148) and carries them as
// BAM-encoded ops (src/kaptive/core/alignment.py:872).  Here the paths exist on the device only, as the direction bits of the
// fill kernels; the tracebacks reduce every path to the fields of its hit.  These kernels run after the hit table is final
// (kp_hit_sort_kernel) and while the work set's trace buffer still holds the pass:
//
//   kp_cigar_locate_*   every source of a hit -- a band task above the score cut-off that no chain consumed, a joined path --
//                       rebuilds its record exactly as the hit compaction did and looks it up in its assembly's finished list
//                       (by gene: the list is sorted by it, and a gene has a few hits); sources that meet at one record settle
//                       by an atomic minimum on a key made of the data alone (the tie rule of kp_spec.h)
//   kp_cigar_walk       one lane per finished hit: the source's path is walked again by the SAME walks as the tracebacks
//                       (kp_walk.h) with a visitor that merges columns of one kind into run-length ops; first to count the ops
//                       of every hit, then -- after an exclusive scan of the counts -- to write them, last op first, since
//                       the walk runs from the path's end to its start and ops are listed along the target
//   kp_cigar_scan       the exclusive scan, one block (measured: 3.1-3.8 ms for 1.16 M hits -- DESIGN.md section 3; kp_cs.hip scans its byte counts with it)
//
// The ops buffer is sized by the policy of kp_caps.h; the writing pass checks every store against its end, so a buffer that is
// too small loses ops but nothing else, and the counts say how much room the repeat needs.
#include <algorithm>

#include "kp_hits.h"
#include "kp_internal.h"
#include "kp_reduce_core.h"
#include "kp_walk.h"

namespace {

constexpr unsigned long long SRC_NONE = ~0ull;
constexpr int LO_BIAS = 1 << 30;  // band origins are diagonals of an assembly: above -KP_MAX_GENE_LEN, below KP_MAX_ASM_LEN
constexpr int WALK_THREADS = 256;
constexpr int SCAN_THREADS = 1024;

// The tie rule: band tasks before joins, then the lower band origin (of the piece the path ends in), then the narrower band.
// What follows (the slot) only keeps two sources apart that share all three, i.e. fill the same band from the same rows.
__device__ __forceinline__ unsigned long long src_key(bool join, int lo, uint32_t ref) {
    return ((unsigned long long)(join ? 1u : 0u) << 63) | ((unsigned long long)(uint32_t)(lo + LO_BIAS) << 32) | ref;
}

// the finished record this source's raw record became, if it is the one its span kept
__device__ __forceinline__ void claim(const kp_hit *h, int n, const kp_hit &mine, unsigned long long key, unsigned long long *src) {
    for (int i = kp_lower_bound_gene(h, n, mine.gene); i < n && h[i].gene == mine.gene; ++i) {
        if (!kp_same_span(h[i], mine)) continue;
        if (h[i].score == KP_HIT_SCORE(mine.score) && h[i].matches == mine.matches && h[i].block_len == mine.block_len && h[i].n_seeds == mine.n_seeds)
            atomicMin(&src[i], key);
        return;  // (a span is in the list once)
    }
}

__global__ __launch_bounds__(256) void kp_cigar_locate_tasks_kernel(KpBatchView b, const int32_t *__restrict__ gene_len,
                                                                    const KpTask *__restrict__ tasks, const KpSwResult *__restrict__ results,
                                                                    const uint8_t *__restrict__ task_drop, const uint32_t *__restrict__ task_count,
                                                                    uint32_t task_cap, const kp_hit *__restrict__ hits,
                                                                    const uint32_t *__restrict__ n_hits, uint32_t hit_cap,
                                                                    unsigned long long *__restrict__ src) {
    const int cls = blockIdx.y;
    uint32_t n = task_count[cls];
    if (n > task_cap) n = task_cap;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const size_t at = (size_t)cls * task_cap + i;
        const KpTask t = tasks[at];
        kp_hit mine;
        if (!kp_task_hit(b, gene_len, t, results[at], task_drop[at] != 0, &mine)) continue;
        claim(hits + (size_t)t.asm_id * hit_cap, (int)min(n_hits[t.asm_id], hit_cap), mine, src_key(false, t.lo, KP_TASK_REF(cls, i)),
              src + (size_t)t.asm_id * hit_cap);
    }
}

// a join's reference: band class, slot in the class's list, piece the path ends in
__device__ __forceinline__ uint32_t join_ref(int cls, uint32_t ji, int k) { return ((uint32_t)cls << 28) | (ji << 3) | (uint32_t)k; }
static_assert(KP_JOIN_MAX_PIECES <= 8, "three bits of a join's reference name the piece");

__global__ __launch_bounds__(64) void kp_cigar_locate_joins_kernel(KpBatchView b, const int32_t *__restrict__ gene_len,
                                                                   const KpJoin *__restrict__ joins, const uint32_t *__restrict__ join_count,
                                                                   uint32_t join_cap, const kp_hit *__restrict__ hits,
                                                                   const uint32_t *__restrict__ n_hits, uint32_t hit_cap,
                                                                   unsigned long long *__restrict__ src) {
    const int cls = blockIdx.y;
    uint32_t n = join_count[cls];
    if (n > join_cap) n = join_cap;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const KpJoin &J = joins[(size_t)cls * join_cap + i];
        for (int k = 1; k < J.n_pieces; ++k) {
            kp_hit mine;
            if (!kp_join_piece_hit(b, gene_len, J, k, &mine)) continue;
            claim(hits + (size_t)J.asm_id * hit_cap, (int)min(n_hits[J.asm_id], hit_cap), mine, src_key(true, J.lo[k], join_ref(cls, i, k)),
                  src + (size_t)J.asm_id * hit_cap);
        }
    }
}

// Columns of one kind, as the walk meets them, merged into ops: a cross gap that touches an in-band gap of its kind is one op.
// The walk goes from the path's end to its start, so ops come out last first: `pos` counts down from the end of the hit's ops.
struct OpRuns {
    uint32_t *out;      // null: count only
    int64_t pos, cap;   // next op goes to out[pos - 1] if that lies below cap
    int op = -1;
    uint32_t len = 0, n = 0;
    __device__ __forceinline__ void flush() {
        if (op < 0) return;
        ++n;
        if (out) {
            --pos;
            if (pos >= 0 && pos < cap) out[pos] = (len << 4) | (uint32_t)op;
        }
    }
    __device__ __forceinline__ void run(int o, int k) {
        if (k <= 0) return;
        if (o == op) { len += (uint32_t)k; return; }
        flush();
        op = o; len = (uint32_t)k;
    }
};

template <bool EMIT>
__global__ __launch_bounds__(WALK_THREADS) void kp_cigar_walk_kernel(KpBatchView b, KpGenes genes, const KpTask *__restrict__ tasks,
                                                                     const KpSwEnd *__restrict__ ends, uint32_t task_cap,
                                                                     const KpJoin *__restrict__ joins, uint32_t join_cap,
                                                                     const uint4 *__restrict__ trace, bool summaries, const uint32_t *__restrict__ n_hits,
                                                                     uint32_t hit_cap, const int64_t *__restrict__ hit_off,
                                                                     const unsigned long long *__restrict__ src, uint32_t *__restrict__ cnt,
                                                                     const int64_t *__restrict__ off, uint32_t *__restrict__ ops, int64_t ops_cap) {
    for (int a = blockIdx.x; a < b.n_asm; a += gridDim.x) {
        const uint32_t n = min(n_hits[a], hit_cap);
        for (uint32_t i0 = 0; i0 < n; i0 += WALK_THREADS) {  // whole waves iterate together (kp_band_walk)
            const uint32_t i = i0 + threadIdx.x;
            const bool have = i < n;
            const unsigned long long key = have ? src[(size_t)a * hit_cap + i] : SRC_NONE;
            const bool is_join = key != SRC_NONE && (key >> 63) != 0, is_task = key != SRC_NONE && !is_join;
            const uint32_t ref = (uint32_t)key;
            const int cls = is_task || is_join ? (int)(ref >> 28) : 0, P = 4 << cls;
            const int64_t row = hit_off[a] + i;
            OpRuns v;
            v.out = EMIT ? ops : nullptr; v.cap = ops_cap; v.pos = EMIT && have ? off[row + 1] : 0;
            // a band task: its direction bits need no N test (matches are not counted here), so the fast path -- plain pieces skipped by their summaries -- serves every task
            KpTask tk;
            tk.asm_id = a; tk.gs = 0; tk.contig = 0; tk.lo = 0;
            KpSwEnd e;
            e.score = 0; e.er = 0; e.eb = 0; e.trace_off = 0;
            const KpJoin *J = joins + (size_t)cls * join_cap + (is_join ? (ref & 0x0FFFFFFFu) >> 3 : 0u);
            if (is_task) {
                const size_t at = (size_t)cls * task_cap + KP_REF_SLOT(ref);
                tk = tasks[at]; e = ends[at];
            }
            const KpTaskSeqs s = kp_task_seqs(b, genes, a, is_join ? J->gs : tk.gs, is_join ? J->contig : tk.contig);
            int q0 = 0, r_hi = 0;
            if (is_task) kp_task_rows(tk.lo, 4 * P, s.t.cstart, s.t.cend, s.q.len, &q0, &r_hi);
            KpBandPath bp;
            kp_band_walk(is_task, summaries, tk.lo, P, q0, r_hi, e.er, e.eb & 255, false, trace + e.trace_off, s, bp, v);
            if (is_join) {  // (rare: a lane each, after the wave's band tasks)
                KpJoinPath jp;
                kp_join_walk(J, (int)(ref & 7u), P, s, trace, jp, v);
            }
            v.flush();
            if (!EMIT && have) cnt[row] = v.n;
        }
    }
}

// off[0 .. n] = exclusive scan of cnt[0 .. n): one block, every thread a contiguous share
__global__ __launch_bounds__(SCAN_THREADS) void kp_cigar_scan_kernel(const uint32_t *__restrict__ cnt, int64_t n, int64_t *__restrict__ off) {
    __shared__ int64_t s_sum[SCAN_THREADS];
    const int tid = threadIdx.x;
    const int64_t per = (n + SCAN_THREADS - 1) / SCAN_THREADS;
    const int64_t lo = (int64_t)tid * per < n ? (int64_t)tid * per : n, hi = lo + per < n ? lo + per : n;
    int64_t mine = 0;
    for (int64_t i = lo; i < hi; ++i) mine += cnt[i];
    s_sum[tid] = mine;
    __syncthreads();
    for (int o = 1; o < SCAN_THREADS; o <<= 1) {  // inclusive scan
        const int64_t v = tid >= o ? s_sum[tid - o] : 0;
        __syncthreads();
        s_sum[tid] += v;
        __syncthreads();
    }
    int64_t at = s_sum[tid] - mine;
    for (int64_t i = lo; i < hi; ++i) { off[i] = at; at += cnt[i]; }
    if (tid == SCAN_THREADS - 1) off[n] = s_sum[tid];
}

}  // namespace

void kp_launch_cigar_locate(const KpBatchView &b, const int32_t *gene_len, const KpTasks &t, const KpJoins &j, const KpHitTable &hits,
                            unsigned long long *src, hipStream_t stream) {
    (void)hipMemsetAsync(src, 0xFF, (size_t)b.n_asm * hits.cap * sizeof(unsigned long long), stream);
    hipLaunchKernelGGL(kp_cigar_locate_tasks_kernel, dim3(256, KP_N_CLASSES), dim3(256), 0, stream, b, gene_len, t.tasks, t.results, t.drop, t.count,
                       t.cap, hits.rows, hits.count, hits.cap, src);
    hipLaunchKernelGGL(kp_cigar_locate_joins_kernel, dim3(16, KP_N_CLASSES), dim3(64), 0, stream, b, gene_len, j.list, j.count, j.cap, hits.rows,
                       hits.count, hits.cap, src);
}

// off[0 .. n] = exclusive scan of cnt[0 .. n): the scan above for any per-hit counts (kp_cs.hip: bytes of the cs strings)
void kp_launch_count_scan(const uint32_t *cnt, int64_t n, int64_t *off, hipStream_t stream) {
    hipLaunchKernelGGL(kp_cigar_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, cnt, n, off);
}

void kp_launch_cigar_walk(const KpBatchView &b, const KpGenes &genes, const KpTasks &t, const KpJoins &j, const KpTrace &trace, const KpHitTable &hits,
                          const KpHitRows &rows, const unsigned long long *src, const KpPerHit<uint32_t> &cig, bool emit, bool walk_summaries, hipStream_t stream) {
    const dim3 grid((unsigned)std::min(std::max(b.n_asm, 1), 4096)), block(WALK_THREADS);
    if (!emit) {
        hipLaunchKernelGGL(kp_cigar_walk_kernel<false>, grid, block, 0, stream, b, genes, t.tasks, t.ends, t.cap, j.list, j.cap, trace.units, walk_summaries, hits.count,
                           hits.cap, rows.hit_off, src, cig.cnt, (const int64_t *)nullptr, (uint32_t *)nullptr, (int64_t)0);
        return kp_launch_count_scan(cig.cnt, rows.total, cig.off, stream);
    }
    hipLaunchKernelGGL(kp_cigar_walk_kernel<true>, grid, block, 0, stream, b, genes, t.tasks, t.ends, t.cap, j.list, j.cap, trace.units, walk_summaries, hits.count,
                       hits.cap, rows.hit_off, src, (uint32_t *)nullptr, cig.off, cig.data, cig.cap);
}
