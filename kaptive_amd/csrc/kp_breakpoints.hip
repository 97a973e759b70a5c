// kp_breakpoints.hip -- breakpoint records of the kept lists (kp_spec.h, BREAKPOINTS; made when they are first asked for).
//
// On the reduction's stream, behind the kernels that finalise the kept list.  They read the kept records, the contig lengths and,
// for the inverted repeat of an insertion, the packed contigs: no hit table, no op, no trace.
//
//   kp_breakpoints_pair_kernel     one wave per assembly.  What a pair reads of a kept record (kp_breakpoints.h: KpBpFrag, eight
//                                  words) is staged in LDS, field by field, a tile of the list at a time -- the whole list at once
//                                  where it fits the tile, which it nearly always does.  Lanes take the b's in ascending chunks of
//                                  64; every lane scans every staged a (all lanes read the same LDS word: a broadcast) and keeps the
//                                  smallest key.  The lanes that have a record place it by a ballot, so the assembly's records ascend
//                                  in kept_b, from the assembly's first kept row on in a buffer of one record per kept row; the wave
//                                  leaves their number.
//   kp_launch_count_scan           the exclusive scan of those numbers (kp_cigar.hip's, as it is): bp_off[n_asm + 1]
//   kp_breakpoints_compact_kernel  moves the records of every assembly to its offset: one buffer, back to back
//
// One record per kept row is an upper bound (a record per b at the most), so no buffer can overflow and nothing is retried.
#include <algorithm>

#include "kp_internal.h"
#include "kp_breakpoints.h"

namespace {

constexpr int BP_THREADS = 64;     // one wave
constexpr int BP_MAX_TILE = 1024;  // kept records staged at a time: 32 KB of LDS

struct KpBpStaged {  // tile records [first, first + tile) of the list, field k of record i at s[k * tile + i - first]
    const int32_t *s;
    int tile, first;
    __device__ __forceinline__ KpBpFrag operator()(int i) const {
        const int32_t *p = s + (i - first);
        KpBpFrag f;
        f.gene = p[0]; f.contig = p[tile]; f.q_start = p[2 * tile]; f.q_end = p[3 * tile]; f.t_start = p[4 * tile]; f.t_end = p[5 * tile];
        f.ctg_len = p[6 * tile]; f.strand = p[7 * tile];
        return f;
    }
};

__global__ __launch_bounds__(BP_THREADS) void kp_breakpoints_pair_kernel(KpBatchView b, const kp_kept *__restrict__ kept, int kept_cap,
                                                                         const int64_t *__restrict__ kept_off, int tile,
                                                                         kp_breakpoint *__restrict__ out, uint32_t *__restrict__ cnt) {
    extern __shared__ int32_t s_frag[];  // KP_BP_FRAG_WORDS * tile
    const int lane = threadIdx.x;
    for (int a = blockIdx.x; a < b.n_asm; a += gridDim.x) {
        const int64_t row0 = kept_off[a];
        const int n = (int)min((int64_t)kept_cap, kept_off[a + 1] - row0);  // (the host lays the rows out from counts that fitted the kept list)
        const kp_kept *list = kept + (size_t)a * kept_cap;
        const int c0 = b.asm_first_ctg[a], n_ctg = b.asm_first_ctg[a + 1] - c0;
        const int32_t *ctg_len = b.ctg_len + c0;
        int first = -1;  // the tile that is staged
        unsigned n_out = 0;
        for (int b0 = 0; b0 < n; b0 += BP_THREADS) {
            const int ib = b0 + lane;
            KpBpFrag fb;
            fb.gene = -1;
            if (ib < n) fb = kp_bp_frag(list[ib], n_ctg, ctg_len);
            KpBpBest best;
            for (int t0 = 0; t0 < n; t0 += tile) {
                const int t1 = min(n, t0 + tile);
                if (first != t0) {  // (uniform: a list within one tile is staged once, a longer one tile by tile for every chunk of b's)
                    __syncthreads();
                    for (int i = t0 + lane; i < t1; i += BP_THREADS) {
                        const KpBpFrag f = kp_bp_frag(list[i], n_ctg, ctg_len);
                        int32_t *p = s_frag + (i - t0);
                        p[0] = f.gene; p[tile] = f.contig; p[2 * tile] = f.q_start; p[3 * tile] = f.q_end; p[4 * tile] = f.t_start;
                        p[5 * tile] = f.t_end; p[6 * tile] = f.ctg_len; p[7 * tile] = f.strand;
                    }
                    __syncthreads();
                    first = t0;
                }
                kp_bp_select(KpBpStaged{s_frag, tile, t0}, t0, t1, fb, ib, best);
            }
            const bool have = best.a >= 0;
            const unsigned long long mask = __ballot(have);
            if (have) {
                KpTargetSeq t;  // b's contig (a COLLINEAR record's a lies on the same one)
                const int r0 = b.asm_first_nrun[a];
                t.words = b.words + b.asm_word_off[a];
                t.n_words = (int)(b.asm_word_off[a + 1] - b.asm_word_off[a]);
                t.runs = b.n_runs + 2 * (size_t)r0;
                t.n_runs = b.asm_first_nrun[a + 1] - r0;
                t.cstart = b.ctg_start[c0 + fb.contig];
                t.cend = t.cstart + fb.ctg_len;
                const unsigned at = n_out + (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
                kp_breakpoint_store(out + row0 + at, kp_bp_record(best, ib, t));  // at <= ib < n: inside the assembly's rows
            }
            n_out += (unsigned)__popcll(mask);
        }
        if (lane == 0) cnt[a] = n_out;
    }
}

// the records of assembly a, tmp[kept_off[a] .. + bp_off[a + 1] - bp_off[a]), to out[bp_off[a] ..]: a thread per kept row
__global__ __launch_bounds__(256) void kp_breakpoints_compact_kernel(const kp_breakpoint *__restrict__ tmp, const int64_t *__restrict__ kept_off,
                                                                     const int64_t *__restrict__ bp_off, int n_asm, int64_t total,
                                                                     kp_breakpoint *__restrict__ out) {
    for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < total; row += (int64_t)gridDim.x * blockDim.x) {
        int a = 0;  // the last assembly with kept_off[a] <= row
        for (int z = n_asm; a + 1 < z;) {
            const int mid = (a + z) >> 1;
            if (kept_off[mid] <= row) a = mid; else z = mid;
        }
        const int64_t i = row - kept_off[a];
        if (i >= bp_off[a + 1] - bp_off[a]) continue;
        const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(tmp + row);
        ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(out + bp_off[a] + i);
        const ulonglong2 lo = src[0], hi = src[1];
        dst[0] = lo; dst[1] = hi;
    }
}

}  // namespace

void kp_launch_breakpoints(const KpBatchView &b, const KpKeptRows &kept, int max_kept, kp_breakpoint *tmp, uint32_t *cnt, int64_t *bp_off,
                           kp_breakpoint *out, hipStream_t stream) {
    if (b.n_asm <= 0) return;
    const int tile = std::min(std::max((max_kept + BP_THREADS - 1) / BP_THREADS * BP_THREADS, BP_THREADS), BP_MAX_TILE);
    hipLaunchKernelGGL(kp_breakpoints_pair_kernel, dim3((unsigned)std::min(b.n_asm, 1 << 20)), dim3(BP_THREADS),
                       (size_t)KP_BP_FRAG_WORDS * tile * sizeof(int32_t), stream, b, kept.kept, kept.kept_cap, kept.kept_off, tile, tmp, cnt);
    kp_launch_count_scan(cnt, b.n_asm, bp_off, stream);
    if (kept.total <= 0) return;
    const unsigned blocks = (unsigned)std::min<int64_t>((kept.total + 255) / 256, 4096);
    hipLaunchKernelGGL(kp_breakpoints_compact_kernel, dim3(blocks), dim3(256), 0, stream, tmp, kept.kept_off, bp_off, b.n_asm, kept.total, out);
}
