// kp_aligned.hip -- reference-anchored alignment rows of the KEPT hits (kp_spec.h, ALIGNED ROWS; only with the `aligned` option).
//
// On the reduction's stream, behind the kernels that finalise the kept list and behind kp_launch_kept_locate (kp_variants.hip), which
// leaves the hit row of every kept record in `src`.  They read the kept records, the final ops of the pass and the packed contigs
// with their N runs; the genes' lengths, never their bases.
//
//   kp_aligned_count_kernel  one lane per kept row: (Lq + 15) / 16 blocks.  kp_launch_count_scan turns the counts into block offsets;
//                            the host fetches the total and reserves exactly that -- no guessed capacity, nothing overflows.
//   kp_aligned_emit_kernel   one wave per kept row, grid-strided, four waves a block.
//       validity   the lanes add the ops' row and column advances; kp_aln_walk_ok (the variant walk's check) decides.  An invalid
//                  walk stores the all-GAP row and nothing else.
//       segments   lanes take the ops 64 at a time; a wave prefix sum (__shfl_up) of the gene advance (M + I) and of the contig
//                  advance (M + D) gives every M op its segment (kp_aln_segment); a wave-uniform carry links one chunk to the next.
//                  The M ops of up to two chunks lie compacted in the wave's LDS table (ALN_SEGS entries of 12 bytes, 6 KB a block).
//       blocks     block j of the row belongs to lane j % 64 for the whole kernel: plain 8-byte stores, nothing atomic.  The lane
//                  finds the first segment that reaches its block by binary search in the table, walks on while segments overlap,
//                  and places each overlap's columns (kp_aln_block_add: one or two packed words, shifted into place).  Columns no
//                  segment covers stay GAP.  A hit of at most ALN_SEGS ops -- nearly every one -- is done in one round and every
//                  block is stored once; a longer one first stores its row all GAP, then every round's lanes read back the blocks
//                  that round's segments reach (their own stores) and complete them.
//       N runs     one wave-uniform look at the N runs (kp_al_clear_of_runs) lets a hit that no run touches skip the mask.
//       record     covered is the wave sum of the columns placed, inserted / n_ins that of the D ops met; lane 0 stores the record.
//
// No lane reads an op outside [z0, z1) (clamped to the ops buffer), a packed word outside the contig (the walk was checked before
// the first read) or an LDS entry outside the table (a round ends before a chunk could overfill it).
#include <algorithm>

#include "kp_internal.h"
#include "kp_aligned.h"

namespace {

constexpr int ALN_THREADS = 256;  // four waves, each with rows of its own
constexpr int ALN_WAVE = 64;
constexpr int ALN_WAVES = ALN_THREADS / ALN_WAVE;
constexpr int ALN_SEGS = 128;     // segments of a round: two chunks of ops at the most

// the wave's LDS stores are visible to its own lanes' loads (rows differ in length from wave to wave: no block-wide barrier here)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int64_t min64(int64_t x, int64_t y) { return x < y ? x : y; }

template <class T>
__device__ __forceinline__ T wave_sum(T v) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ int wave_scan(int v, int lane) {  // inclusive
    for (int o = 1; o < ALN_WAVE; o <<= 1) {
        const int u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}

// the last a with off[a] <= row, a < n_asm
__device__ __forceinline__ int asm_of_row(const int64_t *__restrict__ off, int n_asm, int64_t row) {
    int a = 0;
    for (int z = n_asm; a + 1 < z;) {
        const int mid = (a + z) >> 1;
        if (off[mid] <= row) a = mid; else z = mid;
    }
    return a;
}

// Lq of the gene behind kept row `row` (0: a row beyond the kept list's capacity or a gene the context does not have)
__device__ __forceinline__ int row_gene_len(const kp_kept *__restrict__ kept, int kept_cap, int a, int i, int32_t gene_lo,
                                            const int32_t *__restrict__ gene_len, int32_t n_genes) {
    if (i >= kept_cap) return 0;
    const int64_t g = (int64_t)kept[(size_t)a * kept_cap + i].gene + gene_lo;
    if (g < 0 || g >= n_genes) return 0;
    const int L = gene_len[g];
    return L > 0 ? L : 0;
}

__global__ __launch_bounds__(ALN_THREADS) void kp_aligned_count_kernel(int32_t n_asm, const int32_t *__restrict__ gene_len, int32_t n_genes,
                                                                       const kp_kept *__restrict__ kept, int kept_cap,
                                                                       const int64_t *__restrict__ kept_off, int64_t total_kept, int32_t gene_lo,
                                                                       uint32_t *__restrict__ cnt) {
    for (int64_t row = (int64_t)blockIdx.x * ALN_THREADS + threadIdx.x; row < total_kept; row += (int64_t)gridDim.x * ALN_THREADS) {
        const int a = asm_of_row(kept_off, n_asm, row);
        cnt[row] = (uint32_t)kp_aln_blocks(row_gene_len(kept, kept_cap, a, (int)(row - kept_off[a]), gene_lo, gene_len, n_genes));
    }
}

// block j of the row with every segment of the table that reaches it placed
__device__ __forceinline__ uint64_t block_of_segments(uint64_t v, const KpAlnSeg *seg, int nseg, const KpTargetSeq &t, bool rev, int64_t j, bool clear,
                                                      int *covered) {
    const int64_t lo = j * KP_ALN_COLS, hi = lo + KP_ALN_COLS;
    // the table follows the walk: ascending columns for strand +1, descending ones for strand -1.  First segment that is not wholly
    // before the block in that order:
    int x = 0;
    for (int z = nseg; x < z;) {
        const int mid = (x + z) >> 1;
        const bool before = rev ? seg[mid].col >= hi : (int64_t)seg[mid].col + seg[mid].len <= lo;
        if (before) x = mid + 1; else z = mid;
    }
    for (; x < nseg; ++x) {
        const KpAlnSeg s = seg[x];
        if (rev ? (int64_t)s.col + s.len <= lo : s.col >= hi) break;  // wholly behind it: so are the rest
        v = kp_aln_block_add(v, t, s, rev, j, clear, covered);
    }
    return v;
}

__global__ __launch_bounds__(ALN_THREADS) void kp_aligned_emit_kernel(KpBatchView b, const int32_t *__restrict__ gene_len, int32_t n_genes,
                                                                      const uint32_t *__restrict__ ops, const int64_t *__restrict__ cigar_off,
                                                                      int64_t ops_cap, const kp_kept *__restrict__ kept, int kept_cap,
                                                                      const int64_t *__restrict__ kept_off, int64_t total_kept, int32_t gene_lo,
                                                                      const int64_t *__restrict__ src, int64_t n_hit_rows,
                                                                      const int64_t *__restrict__ off, uint64_t *blocks,
                                                                      kp_aligned_row *__restrict__ rows_out) {
    __shared__ KpAlnSeg s_seg[ALN_WAVES][ALN_SEGS];
    const int lane = threadIdx.x & (ALN_WAVE - 1);
    KpAlnSeg *const seg = s_seg[threadIdx.x / ALN_WAVE];
    const int64_t n_waves = (int64_t)gridDim.x * ALN_WAVES;
    for (int64_t row = (int64_t)blockIdx.x * ALN_WAVES + threadIdx.x / ALN_WAVE; row < total_kept; row += n_waves) {
        // everything down to the chunk loop is the same in every lane: the whole wave reads one row
        const int a = asm_of_row(kept_off, b.n_asm, row);
        const int i = (int)(row - kept_off[a]);
        const int Lq = row_gene_len(kept, kept_cap, a, i, gene_lo, gene_len, n_genes);
        const int64_t base = off[row];
        const int64_t nb = min64(kp_aln_blocks(Lq), off[row + 1] - base);  // (equal: the counts came from the same lengths)
        bool ok = Lq > 0;
        int q_start = 0, q_end = 0, t_start = 0, contig = -1;
        bool rev = false;
        if (ok) {
            const kp_kept &k = kept[(size_t)a * kept_cap + i];
            q_start = k.q_start; q_end = k.q_end; t_start = k.t_start; contig = k.contig; rev = k.strand < 0;
        }
        const int c0 = b.asm_first_ctg[a], n_ctg = b.asm_first_ctg[a + 1] - c0;
        const int64_t at = ok ? src[row] : -1;
        ok = ok && at >= 0 && at < n_hit_rows && contig >= 0 && contig < n_ctg;
        int64_t z0 = 0, z1 = 0;
        KpTargetSeq t{};
        if (ok) {
            z0 = cigar_off[at]; z1 = cigar_off[at + 1];
            if (z1 > ops_cap) z1 = ops_cap;  // (the ops are final when this runs: their buffer held them all)
            if (z0 < 0) z0 = 0;
            if (z0 > z1) z0 = z1;
            const int r0 = b.asm_first_nrun[a];
            t.words = b.words + b.asm_word_off[a];
            t.n_words = (int)(b.asm_word_off[a + 1] - b.asm_word_off[a]);
            t.runs = b.n_runs + 2 * (size_t)r0;
            t.n_runs = b.asm_first_nrun[a + 1] - r0;
            t.cstart = b.ctg_start[c0 + contig];
            t.cend = t.cstart + b.ctg_len[c0 + contig];
        }
        const int q0 = rev ? Lq - q_end : q_start;
        int64_t cols = 0;
        if (ok) {
            int64_t rs = 0, cs = 0;
            for (int64_t z = z0 + lane; z < z1; z += ALN_WAVE) { rs += kp_aln_op_rows(ops[z]); cs += kp_aln_op_cols(ops[z]); }
            rs = wave_sum(rs); cols = wave_sum(cs);
            ok = kp_aln_walk_ok(t, Lq, q0, t_start, rs, cols);
        }
        if (!ok) {  // the all-GAP row and nothing else
            for (int64_t j = lane; j < nb; j += ALN_WAVE) blocks[base + j] = kp_aln_gap_block(Lq, j);
            if (lane == 0) kp_aligned_row_store(rows_out + row, base, Lq, 0, 0, 0);
            continue;
        }
        const int t0 = t.cstart + t_start;
        const bool clear = kp_al_clear_of_runs(t, t0, (int32_t)(t0 + cols));
        const bool single = z1 - z0 <= ALN_SEGS;  // one round: every block is stored once, nothing is read back
        if (!single)
            for (int64_t j = lane; j < nb; j += ALN_WAVE) blocks[base + j] = kp_aln_gap_block(Lq, j);
        int r_carry = q0, t_carry = t0, nseg = 0;  // wave-uniform
        int covered = 0, inserted = 0, n_ins = 0;  // the lane's share
        int64_t c = z0;
        bool last;
        do {
            // ---- segments of the ops c .. c + 63
            const int64_t z = c + lane;
            const uint32_t op = z < z1 ? ops[z] : 15u;  // (kind 15, length 0: moves nothing)
            const uint32_t kind = op & 15u;
            const int len = (int)(op >> KP_CIGAR_SHIFT);
            const int ga = (kind == KP_CIGAR_M || kind == KP_CIGAR_I) ? len : 0, ta = (kind == KP_CIGAR_M || kind == KP_CIGAR_D) ? len : 0;
            const int gi = wave_scan(ga, lane), ti = wave_scan(ta, lane);
            const bool is_m = kind == KP_CIGAR_M && len > 0;
            const unsigned long long ms = __ballot(is_m);
            if (is_m) seg[nseg + __popcll(ms & ((1ull << lane) - 1ull))] = kp_aln_segment(r_carry + gi - ga, t_carry + ti - ta, len, Lq, rev);
            if (kind == KP_CIGAR_D) { inserted += len; n_ins += 1; }
            nseg += __popcll(ms);
            r_carry += __shfl(gi, ALN_WAVE - 1); t_carry += __shfl(ti, ALN_WAVE - 1);
            c += ALN_WAVE;
            last = c >= z1;
            if (!last && nseg <= ALN_SEGS - ALN_WAVE) continue;  // the next chunk still fits
            // ---- blocks of this round
            wave_sync();
            if (single) {
                for (int64_t j = lane; j < nb; j += ALN_WAVE)
                    blocks[base + j] = block_of_segments(kp_aln_gap_block(Lq, j), seg, nseg, t, rev, j, clear, &covered);
            } else if (nseg > 0) {
                const KpAlnSeg first = seg[0], end = seg[nseg - 1];
                const int64_t lo = rev ? end.col : first.col, hi = rev ? (int64_t)first.col + first.len : (int64_t)end.col + end.len;
                const int64_t jlo = lo / KP_ALN_COLS, jhi = min64((hi - 1) / KP_ALN_COLS, nb - 1);
                for (int64_t j = jlo + ((lane - jlo) & (ALN_WAVE - 1)); j <= jhi; j += ALN_WAVE)  // (j % 64 == lane: the block's owner)
                    blocks[base + j] = block_of_segments(blocks[base + j], seg, nseg, t, rev, j, clear, &covered);
            }
            nseg = 0;
            wave_sync();  // (the next round's segments overwrite the table)
        } while (!last);
        covered = wave_sum(covered); inserted = wave_sum(inserted); n_ins = wave_sum(n_ins);
        if (lane == 0) kp_aligned_row_store(rows_out + row, base, Lq, covered, inserted, n_ins);
    }
}

}  // namespace

void kp_launch_aligned_count(const KpBatchView &b, const KpGenes &genes, const KpKeptRows &kept, uint32_t *cnt, int64_t *off, hipStream_t stream) {
    if (kept.total <= 0) return;
    const unsigned grid = (unsigned)std::min<int64_t>((kept.total + ALN_THREADS - 1) / ALN_THREADS, 1024);
    hipLaunchKernelGGL(kp_aligned_count_kernel, dim3(grid), dim3(ALN_THREADS), 0, stream, b.n_asm, genes.len, genes.n_genes, kept.kept, kept.kept_cap,
                       kept.kept_off, kept.total, kept.gene_lo, cnt);
    kp_launch_count_scan(cnt, kept.total, off, stream);
}

void kp_launch_aligned_emit(const KpBatchView &b, const KpGenes &genes, const KpHitRows &rows, const KpPerHit<uint32_t> &cig, const KpKeptRows &kept,
                            const int64_t *src, const int64_t *off, uint64_t *blocks, kp_aligned_row *out, hipStream_t stream) {
    if (kept.total <= 0) return;
    const unsigned grid = (unsigned)std::min<int64_t>((kept.total + ALN_WAVES - 1) / ALN_WAVES, 4096);
    hipLaunchKernelGGL(kp_aligned_emit_kernel, dim3(grid), dim3(ALN_THREADS), 0, stream, b, genes.len, genes.n_genes, cig.data, cig.off, cig.cap, kept.kept,
                       kept.kept_cap, kept.kept_off, kept.total, kept.gene_lo, src, rows.total, off, blocks, out);
}
